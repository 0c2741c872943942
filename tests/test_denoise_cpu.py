"""First-hit G-buffer and a-trous denoiser, the parts that need no GPU: the C ABI's symbols, struct
size, defaults and argument checks (which return before any device call), the properties of the numpy
restatement the GPU tests compare against (tests/denoise_ref.py), and the preview's
`denoise` setting driven with a stand-in render context."""
import ctypes as C
import math
from pathlib import Path

import numpy as np
import pytest

import cuda_pathtracer_amd as P
from cuda_pathtracer_amd import _native as N
from cuda_pathtracer_amd import preview as V

import sys
sys.path.insert(0, str(Path(__file__).resolve().parent))
import denoise_ref as R  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
SCENES = ROOT / "tests" / "scenes"
F = np.float32
PT_ERR_ARG = 1

NEW_SYMBOLS = ("pt_gbuffer", "pt_get_gbuffer", "pt_denoise_params_default", "pt_denoiser_create",
               "pt_denoiser_destroy", "pt_denoiser_run", "pt_denoise_host", "pt_denoise_image")


def test_new_symbols_and_struct_size():
    L = P.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert name in N.SIGNATURES
    assert C.sizeof(N.DenoiseParams) == 32
    for name in ("DenoiseParams", "denoise"):
        assert name in P.__all__ and hasattr(P, name)
    for name in ("gbuffer", "denoised"):
        assert callable(getattr(P.PathTracer, name))


def test_defaults_are_as_documented():
    raw = (C.c_uint8 * 32)(*([0xAB] * 32))
    p = N.DenoiseParams.from_buffer(raw)
    P.lib().pt_denoise_params_default(C.byref(p))
    assert p.levels == 5 and p.demodulate == 1 and list(p.reserved) == [0, 0, 0]
    assert (p.sigma_c, p.sigma_n, p.sigma_p) == (F(1.0), F(0.3), F(0.2))
    q = N.DenoiseParams.default()
    assert bytes(q) == bytes(p)


def _host_call(w=4, h=3, samples=1.0, prm=None, rgb=True, gA=True, gB=True, alb=True, out=True, alias=False):
    n = w * h if w > 0 and h > 0 else 1
    a3, a4 = np.zeros(n * 3, F), np.zeros(n * 4, F)
    o = np.zeros(n * 3, F)
    ptr = lambda on, a: a.ctypes.data if on else None   # noqa: E731
    prm = prm if prm is not None else N.DenoiseParams.default()
    return P.lib().pt_denoise_host(w, h, ptr(rgb, a3), samples, ptr(gA, a4), ptr(gB, a4), ptr(alb, a4),
                                   C.byref(prm) if prm is not False else None,
                                   a3.ctypes.data if alias else ptr(out, o))


def _prm(**kw):
    p = N.DenoiseParams.default()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("kw", [
    dict(prm=_prm(levels=9)), dict(prm=_prm(levels=-1)),
    dict(prm=_prm(sigma_c=0.0)), dict(prm=_prm(sigma_n=math.inf)), dict(prm=_prm(sigma_p=math.nan)),
    dict(prm=_prm(sigma_n=-1.0)), dict(samples=0.0), dict(samples=math.nan), dict(w=0), dict(h=0), dict(rgb=False),
    dict(gA=False), dict(gB=False), dict(alb=False), dict(out=False), dict(prm=False), dict(alias=True)],
    ids=lambda kw: ",".join(f"{k}" for k in kw))
def test_denoise_host_argument_errors_need_no_device(kw):
    assert _host_call(**kw) == PT_ERR_ARG
    assert P.lib().pt_last_error()


def test_denoiser_object_argument_errors_need_no_device():
    L = P.lib()
    h = C.c_void_p()
    assert L.pt_denoiser_create(0, 4, C.byref(h)) == PT_ERR_ARG
    assert L.pt_denoiser_create(4, 0, C.byref(h)) == PT_ERR_ARG
    assert L.pt_denoiser_create(4, 4, None) == PT_ERR_ARG
    prm = N.DenoiseParams.default()
    one = C.c_void_p(16)   # (never dereferenced: the NULL denoiser is refused first)
    assert L.pt_denoiser_run(None, one, 1.0, one, one, one, C.byref(prm), C.c_void_p(32), None) == PT_ERR_ARG
    assert L.pt_denoise_image(None, 1.0, C.byref(prm), one) == PT_ERR_ARG
    assert L.pt_gbuffer(None, one, one, one, None, None) == PT_ERR_ARG
    assert L.pt_get_gbuffer(None, one, one, one, None) == PT_ERR_ARG
    assert L.pt_denoiser_destroy(None) == 0


# ---- the restatement's own properties -----------------------------------------------------------
def _guides(h, w, rng, miss_frac=0.0):
    gA = np.zeros((h, w, 4), F)
    gA[..., :3] = (0, 0, 1)
    mat = np.zeros((h, w), np.int32)
    mat[rng.random((h, w)) < miss_frac] = -1
    gA[..., 3] = mat.view(F)
    gB = np.zeros((h, w, 4), F)
    gB[..., 0], gB[..., 1] = np.meshgrid(np.arange(w, dtype=F), np.arange(h, dtype=F))
    gB[..., 3] = 5
    alb = np.ones((h, w, 4), F)
    return gA, gB, alb


def test_ref_levels0_is_rgb_over_samples_bitwise():
    rng = np.random.default_rng(1)
    rgb = (rng.random((9, 13, 3)) * 40).astype(F)
    gA, gB, alb = _guides(9, 13, rng)
    out = R.atrous_ref(rgb, 7.0, gA, gB, alb, 0, 0.5, 0.1, 0.05, demodulate=False)
    assert np.array_equal(out.view(np.uint32), (rgb / F(7.0)).view(np.uint32))


def test_ref_miss_pixels_pass_through():
    rng = np.random.default_rng(2)
    rgb = (rng.random((17, 19, 3)) * 4).astype(F)
    gA, gB, alb = _guides(17, 19, rng, miss_frac=0.2)
    miss = gA[..., 3].view(np.int32) < 0
    assert miss.any() and not miss.all()
    out = R.atrous_ref(rgb, 2.0, gA, gB, alb, 3, 0.5, 0.1, 0.05)
    assert np.array_equal(out[miss].view(np.uint32), (rgb / F(2.0))[miss].view(np.uint32))
    assert not np.array_equal(out[~miss], (rgb / F(2.0))[~miss])   # (the hit pixels are filtered)


def test_ref_edges_in_the_guides_stop_the_filter():
    """Every neighbour on another plane (depth steps of 10 along the normal) or with another normal:
    with sigma_n = sigma_p = 1e-3 each foreign tap weighs <= 1e-6 / (1 + ...) of the centre's, so the
    centre values survive to 1e-3 relative."""
    rng = np.random.default_rng(3)
    h, w = 12, 14
    rgb = (rng.random((h, w, 3)) * 3 + 0.5).astype(F)
    gA, gB, alb = _guides(h, w, rng)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    gB[..., 2] = (10 * ((xx * 7 + yy * 13) % 31)).astype(F)     # another plane for every tap in reach (2 levels)
    out = R.atrous_ref(rgb, 1.0, gA, gB, alb, 2, 0.5, 1e-3, 1e-3)
    np.testing.assert_allclose(out, rgb, rtol=1e-3)
    gA2, gB2, _ = _guides(h, w, rng)
    ang = ((xx * 5 + yy * 11) % 23).astype(F) * F(0.27)
    gA2[..., 0], gA2[..., 1], gA2[..., 2] = np.sin(ang) * F(0.8), np.cos(ang) * F(0.8), F(0.6)
    gB2[..., :3] = 0                                             # one point: only the normals differ
    out2 = R.atrous_ref(rgb, 1.0, gA2, gB2, alb, 2, 0.5, 1e-3, 1e-3)
    np.testing.assert_allclose(out2, rgb, rtol=1e-3)


# ---- the preview's setting ------------------------------------------------------------------------
class FakeCtx:
    def __init__(self, h, w, log):
        self.h, self.w, self.log = h, w, log
        self.freed = False

    def set_flags(self, gui):
        self.log.append(("flags", gui.SSAA, gui.DoF, gui.aperture, gui.sortbyMaterial))

    def render_pass(self, it):
        self.log.append(("pass", it))

    def image(self):
        return np.full((self.h, self.w, 3), 0.5, np.float32)

    def free(self):
        self.freed = True


class FakeDenoisingCtx(FakeCtx):
    def denoised(self, samples, params=None):
        self.log.append(("denoised", samples))
        img = np.full((self.h, self.w, 3), 0.25, np.float32)
        img[:, 0, 1] = 1.0   # column x = 0: shown at the window's right edge
        return img

    def gbuffer(self):
        self.log.append(("gbuffer",))
        raise AssertionError("the preview does not need the planes themselves")


def _session(tmp_path, ctx_type):
    s = P.Scene(str(SCENES / "cornell.json"))
    log, made = [], []

    def factory(scene, gui):
        c = ctx_type(scene.camera().res[1], scene.camera().res[0], log)
        made.append(c)
        return c

    def read(ctx, it):
        a = np.zeros((ctx.h, ctx.w, 4), np.uint8)
        a[..., 0] = it
        return a

    return V.PreviewSession(s, out_dir=str(tmp_path), tracer_factory=factory, read_preview=read), log, made


def test_preview_denoise_setting_toggles_without_restart(tmp_path):
    ses, log, made = _session(tmp_path, FakeDenoisingCtx)
    assert ses.state()["settings"]["denoise"] is False
    ses.run_cuda()
    ses.run_cuda()
    assert not [e for e in log if e[0] in ("denoised", "gbuffer")]      # off: the new methods are not called
    assert ses.rgba[0, 0, 0] == 2
    ses.set_setting("denoise", True)
    assert not ses.visual_changed and not ses.camchanged
    ses.run_cuda()
    assert ses.iteration == 3 and len(made) == 1                          # no restart
    assert log[-1] == ("denoised", 3.0)
    shown = ses.display_rgb()
    assert shown.shape == (ses.height, ses.width, 3)
    assert (shown[:, -1, 1] == 255).all() and (shown[:, :-1, 1] == 63).all()   # tonemapped; x = 0 at the right edge
    assert ses.state()["settings"]["denoise"] is True
    ses.key("S")                                                          # saving: the raw accumulator
    assert len(ses.saved) == 1 and ses.saved[0].endswith(".3samp.png")
    ses.set_setting("denoise", False)
    ses.run_cuda()
    assert ses.iteration == 4 and len(made) == 1 and ses.rgba[0, 0, 0] == 4
    assert len([e for e in log if e[0] == "denoised"]) == 1


def test_preview_off_never_touches_a_tracer_without_the_methods(tmp_path):
    ses, log, made = _session(tmp_path, FakeCtx)
    for _ in range(3):
        ses.run_cuda()
    assert ses.iteration == 3 and not hasattr(made[0], "denoised")
