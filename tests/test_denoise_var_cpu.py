"""Per-pixel variance and the variance-guided a-trous filter, the parts that need no GPU: the C ABI's
symbols, struct size, defaults and argument checks (which return before any device call: on a machine
without a GPU a device call would fail with another code), the properties of the numpy restatement the
GPU tests compare against (tests/denoise_var_ref.py), and the preview's
`denoise_variance` setting driven with stand-in render contexts.

(`batch_samples` changed between two updates needs a first update that succeeds, so that one is in
tests/test_denoise_var_gpu.py.)"""
import ctypes as C
import math
import sys
from pathlib import Path

import numpy as np
import pytest

import cuda_pathtracer_amd as P
from cuda_pathtracer_amd import _native as N
from cuda_pathtracer_amd import preview as V

sys.path.insert(0, str(Path(__file__).resolve().parent))
import denoise_ref as R  # noqa: E402
import denoise_var_ref as RV  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
SCENES = ROOT / "tests" / "scenes"
F = np.float32
PT_ERR_ARG = 1

NEW_SYMBOLS = ("pt_moments_create", "pt_moments_destroy", "pt_moments_reset", "pt_moments_update", "pt_moments_info",
               "pt_moments_variance", "pt_moments_get", "pt_denoise_var_params_default", "pt_denoiser_run_var",
               "pt_denoise_var_host", "pt_track_variance", "pt_variance_update", "pt_variance_info", "pt_get_variance",
               "pt_denoise_image_var")


def test_new_symbols_and_struct_size():
    L = P.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert name in N.SIGNATURES
    assert C.sizeof(N.DenoiseVarParams) == 32
    assert C.sizeof(N.DenoiseParams) == 32                       # (unchanged)
    for name in ("DenoiseVarParams", "denoise_variance"):
        assert name in P.__all__ and hasattr(P, name)
    for name in ("track_variance", "variance_update", "variance", "denoised_variance"):
        assert callable(getattr(P.PathTracer, name))


def test_defaults_are_as_documented():
    raw = (C.c_uint8 * 32)(*([0xAB] * 32))
    p = N.DenoiseVarParams.from_buffer(raw)
    P.lib().pt_denoise_var_params_default(C.byref(p))
    assert p.levels == 5 and p.demodulate == 1 and list(p.reserved) == [0, 0, 0]
    assert (p.sigma_l, p.sigma_n, p.sigma_p) == (F(1.0), F(0.3), F(0.2))   # sigma_l: DESIGN.md §11's grid
    assert bytes(N.DenoiseVarParams.default()) == bytes(p)


def _host_call(w=4, h=3, samples=1.0, prm=None, rgb=True, var=True, gA=True, gB=True, alb=True, out=True, alias=False,
               alias_var=False):
    n = w * h if w > 0 and h > 0 else 1
    a3, a4, a1 = np.zeros(n * 3, F), np.zeros(n * 4, F), np.zeros(n, F)
    o, ov = np.zeros(n * 3, F), np.zeros(n, F)
    ptr = lambda on, a: a.ctypes.data if on else None   # noqa: E731
    prm = prm if prm is not None else N.DenoiseVarParams.default()
    return P.lib().pt_denoise_var_host(w, h, ptr(rgb, a3), samples, ptr(var, a1), ptr(gA, a4), ptr(gB, a4), ptr(alb, a4),
                                       C.byref(prm) if prm is not False else None,
                                       a3.ctypes.data if alias else ptr(out, o),
                                       a1.ctypes.data if alias_var else ov.ctypes.data)


def _prm(**kw):
    p = N.DenoiseVarParams.default()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("kw", [
    dict(prm=_prm(levels=9)), dict(prm=_prm(levels=-1)),
    dict(prm=_prm(sigma_l=0.0)), dict(prm=_prm(sigma_l=math.nan)), dict(prm=_prm(sigma_n=math.inf)),
    dict(prm=_prm(sigma_p=math.nan)), dict(prm=_prm(sigma_n=-1.0)), dict(samples=0.0), dict(samples=-2.0),
    dict(samples=math.nan), dict(w=0), dict(h=0), dict(rgb=False), dict(var=False), dict(gA=False), dict(gB=False),
    dict(alb=False), dict(out=False), dict(prm=False), dict(alias=True), dict(alias_var=True)],
    ids=lambda kw: ",".join(f"{k}" for k in kw))
def test_denoise_var_host_argument_errors_need_no_device(kw):
    assert _host_call(**kw) == PT_ERR_ARG
    assert P.lib().pt_last_error()


def test_object_and_context_argument_errors_need_no_device():
    L = P.lib()
    prm = N.DenoiseVarParams.default()
    one, two = C.c_void_p(16), C.c_void_p(32)   # (never dereferenced: the checks come first)
    assert L.pt_denoiser_run_var(None, one, 1.0, one, one, one, one, C.byref(prm), two, None, None) == PT_ERR_ARG
    # moments: an object holds no device memory before its first reset or update
    h = C.c_void_p()
    assert L.pt_moments_create(0, 4, C.byref(h)) == PT_ERR_ARG
    assert L.pt_moments_create(4, 0, C.byref(h)) == PT_ERR_ARG
    assert L.pt_moments_create(4, 4, None) == PT_ERR_ARG
    assert L.pt_moments_create(4, 4, C.byref(h)) == 0 and h.value
    try:
        n, bs = C.c_int32(-1), C.c_float(-1)
        assert L.pt_moments_info(h, C.byref(n), C.byref(bs)) == 0 and n.value == 0 and bs.value == 0.0
        for bad in (0.0, -1.0, math.nan, math.inf):
            assert L.pt_moments_update(h, one, bad, None, None) == PT_ERR_ARG, bad
        assert L.pt_moments_update(h, None, 1.0, None, None) == PT_ERR_ARG
        assert L.pt_moments_variance(h, 4.0, one, None) == PT_ERR_ARG          # fewer than 2 batches
        assert b"2 batches" in L.pt_last_error()
        assert L.pt_moments_variance(h, 4.0, None, None) == PT_ERR_ARG
    finally:
        assert L.pt_moments_destroy(h) == 0
    assert L.pt_moments_destroy(None) == 0
    assert L.pt_moments_reset(None, None, None) == PT_ERR_ARG
    assert L.pt_moments_update(None, one, 1.0, None, None) == PT_ERR_ARG
    assert L.pt_moments_variance(None, 1.0, one, None) == PT_ERR_ARG
    assert L.pt_moments_info(None, None, None) == PT_ERR_ARG
    assert L.pt_moments_get(None, None, None, None) == PT_ERR_ARG
    # the context calls
    on = C.c_int32()
    assert L.pt_track_variance(None, 1) == PT_ERR_ARG
    assert L.pt_variance_update(None, 1.0, 1, None) == PT_ERR_ARG
    assert L.pt_variance_info(None, C.byref(on), None, None) == PT_ERR_ARG
    assert L.pt_get_variance(None, 1.0, one) == PT_ERR_ARG
    assert L.pt_denoise_image_var(None, 1.0, C.byref(prm), one) == PT_ERR_ARG


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


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_ref_levels0_is_rgb_over_samples_and_the_input_variance_bitwise():
    rng = np.random.default_rng(1)
    rgb = (rng.random((9, 13, 3)) * 40).astype(F)
    var = (rng.random((9, 13)) * 3).astype(F)
    gA, gB, alb = _guides(9, 13, rng)
    c, v = RV.atrous_var_ref(rgb, 7.0, var, gA, gB, alb, 0, 1.0, 0.1, 0.05, demodulate=False)
    assert np.array_equal(_bits(c), _bits(rgb / F(7.0)))
    assert np.array_equal(_bits(v), _bits(var))


def test_ref_miss_pixels_pass_through_in_both_outputs():
    rng = np.random.default_rng(2)
    rgb = (rng.random((17, 19, 3)) * 4).astype(F)
    var = (rng.random((17, 19)) * 0.5).astype(F)
    gA, gB, alb = _guides(17, 19, rng, miss_frac=0.2)
    miss = gA[..., 3].view(np.int32) < 0
    assert miss.any() and not miss.all()
    c, v = RV.atrous_var_ref(rgb, 2.0, var, gA, gB, alb, 3, 1.0, 0.1, 0.05)
    assert np.array_equal(_bits(c[miss]), _bits((rgb / F(2.0))[miss]))
    assert np.array_equal(_bits(v[miss]), _bits(var[miss]))
    assert not np.array_equal(c[~miss], (rgb / F(2.0))[~miss])     # (the hit pixels are filtered)
    assert not np.array_equal(v[~miss], var[~miss])


@pytest.mark.parametrize("demod", [False, True])
@pytest.mark.parametrize("levels", [1, 3, 5])
def test_ref_huge_variance_is_the_plain_filter_without_a_colour_term_bitwise(levels, demod):
    """Variance 1e30 everywhere (it stays above 1e24 through 5 levels), colours below 4 and albedo in
    [0.5, 1], so a demodulated colour stays below 8: rl < 1e-12 makes xl < 8e-12, and sigma_c = 1e6
    makes xc <= 3 * 8^2 * 1e-12 * 4^4 = 4.9e-8; both are below 2^-24, so both colour terms round 1 + x to
    exactly 1, and the colour outputs are the same bits."""
    rng = np.random.default_rng(100 + levels)
    h, w = 29, 37
    rgb = (rng.random((h, w, 3)) * 4).astype(F)
    gA, gB, alb = _guides(h, w, rng, miss_frac=0.1)
    n = np.array([0, 0, 1]) + rng.normal(0, 0.2, (h, w, 3))
    gA[..., :3] = (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(F)
    gB[..., 2] = rng.normal(0, 0.3, (h, w)).astype(F)
    alb[..., :3] = (rng.random((h, w, 3)) * 0.5 + 0.5).astype(F)
    var = np.full((h, w), 1e30, F)
    c, v = RV.atrous_var_ref(rgb, 1.0, var, gA, gB, alb, levels, 1.0, 0.3, 0.2, demod)
    want = R.atrous_ref(rgb, 1.0, gA, gB, alb, levels, 1e6, 0.3, 0.2, demod)
    assert np.array_equal(_bits(c), _bits(want))
    assert np.isfinite(v).all()


def test_ref_zero_variance_keeps_an_edge_the_guides_cannot_see():
    """Zero variance, flat guides, a noise-free step from 0.8 to 0.2, defaults but sigma_l = 1, 5 levels.
    rl = 2^15, so a tap across the step (|dlum| = 0.6) weighs 1 / (1 + 19661) of one on the same side.
    Measured on the restatement: the largest deviation from the step is 6.652e-05; the bound is 4x that,
    2.7e-4.  (The plain filter at its defaults moves the pixels at the step by 9.6e-2.)"""
    h, w = 24, 32
    rng = np.random.default_rng(5)
    gA, gB, alb = _guides(h, w, rng)
    step = np.where(np.arange(w) < w // 2, F(0.8), F(0.2)).astype(F)
    rgb = np.broadcast_to(step[None, :, None], (h, w, 3)).astype(F).copy()
    c, v = RV.atrous_var_ref(rgb, 1.0, np.zeros((h, w), F), gA, gB, alb, 5, 1.0, 0.3, 0.2)
    dev = float(np.abs(c.astype(np.float64) - rgb).max())
    plain = R.atrous_ref(rgb, 1.0, gA, gB, alb, 5, 1.0, 0.3, 0.2)
    print(f"zero-variance step: max deviation {dev:.3e} (plain filter {np.abs(plain - rgb).max():.3e})")
    assert dev <= 2.7e-4
    assert not v.any()


def test_ref_constant_variance_shrinks_by_the_kernels_square_sum_per_level():
    """Constant colour and variance, flat guides on one plane, huge sigma_l: every weight is h_x h_y
    exactly, so an interior pixel's variance shrinks by sum(h^2)^2 = (70/256)^2 per level.  25 products
    and sums and two divisions per level: measured on the restatement 2.6e-8 relative after 3 levels
    (under half an ulp: the weights are powers of two times small integers); the bound is 4 ulp."""
    h, w = 40, 40
    rng = np.random.default_rng(6)
    gA, gB, alb = _guides(h, w, rng)
    gB[..., :2] = 0      # one point: the plane term is exactly 0
    rgb = np.full((h, w, 3), 0.5, F)
    v0 = F(0.37)
    levels = 3
    c, v = RV.atrous_var_ref(rgb, 1.0, np.full((h, w), v0, F), gA, gB, alb, levels, 1e20, 0.3, 0.2)
    m = 2 * (2 ** levels - 1)                                   # reach of the boundary
    inner = v[m:h - m, m:w - m]
    assert inner.size > 0
    want = float(v0) * (70.0 / 256.0) ** (2 * levels)
    rel = float(np.abs(inner.astype(np.float64) / want - 1).max())
    print(f"variance shrink after {levels} levels: max relative error {rel:.3e}")
    assert rel <= 4 * 2.0 ** -23
    assert np.array_equal(_bits(c), _bits(rgb))


def test_ref_batch_means_estimate_the_variance_of_the_mean():
    """64 batches of 4 samples of Gaussian luminance noise (sigma = 0.3 per sample, grey pixels): the
    estimate of the variance of the 256-sample mean is sigma^2 / 256 per pixel up to the estimator's own
    spread (sqrt(2 / 63) = 18% per pixel); its median over 4096 pixels must be within 15% of that (the
    median of a chi-square with 63 degrees lies 1% below its mean)."""
    rng = np.random.default_rng(7)
    h, w, nb, bs, sigma = 64, 64, 64, 4, 0.3
    mom = RV.Moments(h, w)
    acc = np.zeros((h, w, 3), F)
    for _ in range(nb):
        batch = rng.normal(1.0, sigma / math.sqrt(bs), (h, w, 1)) * bs      # sum of bs samples
        acc = (acc + np.broadcast_to(batch, (h, w, 3)).astype(F)).astype(F)
        mom.update(acc, bs)
    assert mom.batches == nb
    var = mom.variance(nb * bs)
    want = sigma ** 2 / (nb * bs)
    med = float(np.median(var))
    print(f"batch-means estimator: median {med:.4e}, sigma^2 / N {want:.4e}, ratio {med / want:.3f}")
    assert abs(med / want - 1) <= 0.15
    # the issue's case as stated: batches of one sample, sigma^2 / 64
    mom1 = RV.Moments(h, w)
    acc = np.zeros((h, w, 3), F)
    for _ in range(64):
        acc = (acc + np.broadcast_to(rng.normal(1.0, sigma, (h, w, 1)), (h, w, 3)).astype(F)).astype(F)
        mom1.update(acc, 1)
    med1 = float(np.median(mom1.variance(64)))
    assert abs(med1 / (sigma ** 2 / 64) - 1) <= 0.15


def test_ref_moments_demodulate_and_reset():
    rng = np.random.default_rng(8)
    h, w = 5, 7
    a = (rng.random((h, w, 3)) * 2).astype(F)
    alb = np.full((h, w, 4), 0.5, F)
    alb[0, 0, 0] = F(2.0 ** -11)      # below the threshold: not divided
    m = RV.Moments(h, w, base=a)
    m.update(a, 2.0, alb)
    assert not m.m1.any() and not m.m2.any() and np.array_equal(m.prev, a)
    b = (a + F(1)).astype(F)
    m.update(b, 2.0, alb)
    d = (b - a) / F(2)
    dd = d / F(0.5)
    dd[0, 0, 0] = d[0, 0, 0]
    assert np.array_equal(_bits(m.m1), _bits(RV.lum(dd)))
    m.reset(h, w)
    assert m.batches == 0 and not m.prev.any()


# ---- the preview's setting ------------------------------------------------------------------------
class FakeCtx:
    spp = 1

    def __init__(self, h, w, log):
        self.h, self.w, self.log = h, w, log

    def set_flags(self, gui):
        self.log.append(("flags",))

    def render_pass(self, it):
        self.log.append(("pass", it))

    def image(self):
        return np.full((self.h, self.w, 3), 0.5, np.float32)

    def free(self):
        pass


class FakeVarianceCtx(FakeCtx):
    def __init__(self, h, w, log):
        super().__init__(h, w, log)
        self.tracking, self.batches = False, 0

    def denoised(self, samples, params=None):
        self.log.append(("denoised", samples))
        return np.full((self.h, self.w, 3), 0.25, np.float32)

    def track_variance(self, on=True):
        self.log.append(("track", bool(on)))
        self.tracking, self.batches = bool(on), 0

    def variance_update(self, batch_samples=None, demodulate=True, stream=None):
        assert self.tracking
        self.batches += 1
        self.log.append(("update", self.batches))

    def variance_info(self):
        return {"on": self.tracking, "batches": self.batches, "batch_samples": 1.0 if self.batches else 0.0}

    def denoised_variance(self, samples, params=None):
        assert self.tracking and self.batches >= 2
        self.log.append(("denoised_variance", samples))
        return np.full((self.h, self.w, 3), 0.75, np.float32)


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


def test_preview_setting_toggles_without_restart_and_falls_back_below_two_batches(tmp_path):
    ses, log, made = _session(tmp_path, FakeVarianceCtx)
    assert ses.state()["settings"]["denoise_variance"] is False
    ses.run_cuda()
    ses.run_cuda()
    assert not [e for e in log if e[0] not in ("flags", "pass")]          # off: none of the new methods
    ses.set_setting("denoise_variance", True)
    assert not ses.visual_changed and not ses.camchanged
    ses.run_cuda()                                                        # iteration 3: tracking starts, 1 batch
    assert ses.iteration == 3 and len(made) == 1                          # no restart
    tail = [e for e in log if e[0] not in ("flags",)][-4:]
    assert tail == [("track", True), ("pass", 3), ("update", 1), ("denoised", 3.0)]     # one batch: the plain filter
    assert (ses.display_rgb() == 63).all()
    ses.run_cuda()                                                        # iteration 4: two batches
    assert log[-1] == ("denoised_variance", 4.0) and log[-2] == ("update", 2)
    assert (ses.display_rgb() == 191).all()
    assert ses.state()["settings"]["denoise_variance"] is True and ses.state()["settings"]["denoise"] is False
    ses.key("S")                                                          # saving: the raw accumulator
    assert len(ses.saved) == 1 and ses.saved[0].endswith(".4samp.png")
    ses.set_setting("denoise_variance", False)
    ses.run_cuda()
    assert ses.iteration == 5 and len(made) == 1 and ses.rgba[0, 0, 0] == 5
    assert ("track", False) in log and log[-1] == ("pass", 5)
    assert len([e for e in log if e[0] == "track"]) == 2


def test_preview_restart_tracks_the_new_context(tmp_path):
    ses, log, made = _session(tmp_path, FakeVarianceCtx)
    ses.set_setting("denoise_variance", True)
    ses.run_cuda()
    ses.set_setting("SSAA", False)            # a visual setting: the accumulation restarts in a new context
    ses.run_cuda()
    assert len(made) == 2 and ses.iteration == 1
    assert made[1].tracking and made[1].batches == 1


def test_preview_off_never_touches_a_tracer_without_the_methods(tmp_path):
    ses, log, made = _session(tmp_path, FakeCtx)
    for _ in range(3):
        ses.run_cuda()
    assert ses.iteration == 3 and not hasattr(made[0], "track_variance")
    assert ses.rgba[0, 0, 0] == 3
