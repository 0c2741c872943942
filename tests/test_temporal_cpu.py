"""Temporal reprojection, the parts that need no GPU: the C ABI's symbols, struct size,
defaults and argument checks (which return before any device call: on a machine without a GPU a device
call would fail with another code), the properties of the numpy restatement the GPU tests compare against
(tests/temporal_ref.py), and the preview's `denoise_temporal` setting driven with stand-in render contexts
and a stand-in history that enforces pt_temporal_frame's batch rule.

(A batch size that differs from the first frame's, and a context of another size, need a first frame or a
context that succeeds, so those two are in tests/test_temporal_gpu.py; here the restatement's own refusal
of a mismatched batch is checked, and the size check of the Python host variant.)"""
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
import temporal_ref as T  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
SCENES = ROOT / "tests" / "scenes"
F = np.float32
PT_ERR_ARG = 1

NEW_SYMBOLS = ("pt_temporal_params_default", "pt_temporal_create", "pt_temporal_destroy", "pt_temporal_reset",
               "pt_temporal_info", "pt_temporal_frame", "pt_temporal_resolve", "pt_temporal_frame_host", "pt_temporal_get",
               "pt_temporal_frame_ctx", "pt_temporal_image")


def test_new_symbols_struct_size_and_exports():
    L = P.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert name in N.SIGNATURES
    assert C.sizeof(N.TemporalParams) == 32
    for name in ("TemporalParams", "TemporalHistory"):
        assert name in P.__all__ and hasattr(P, name)
    for name in ("frame", "frame_arrays", "image", "info", "reset", "free"):
        assert callable(getattr(P.TemporalHistory, name))


def test_defaults_are_as_documented():
    raw = (C.c_uint8 * 32)(*([0xAB] * 32))
    p = N.TemporalParams.from_buffer(raw)
    P.lib().pt_temporal_params_default(C.byref(p))
    assert p.demodulate == 1 and p.min_frames == 4 and list(p.reserved) == [0, 0, 0]
    assert (p.max_history, p.min_ndot, p.plane_tol) == (F(32.0), F(0.9), F(0.02))   # DESIGN.md §12's grid
    assert bytes(N.TemporalParams.default()) == bytes(p)
    assert {k: getattr(p, k) for k in T.DEFAULTS} == {k: F(v) if isinstance(v, float) else v for k, v in T.DEFAULTS.items()}


def _prm(**kw):
    p = N.TemporalParams.default()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("kw", [
    dict(max_history=-1.0), dict(max_history=math.nan), dict(max_history=math.inf), dict(min_ndot=math.nan),
    dict(min_ndot=1.5), dict(min_ndot=-1.5), dict(plane_tol=-0.1), dict(plane_tol=math.nan), dict(plane_tol=math.inf),
    dict(min_frames=-1), dict(min_frames=(1 << 20) + 1)], ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_create_refuses_parameters_out_of_range(kw):
    h = C.c_void_p()
    assert P.lib().pt_temporal_create(8, 8, C.byref(_prm(**kw)), C.byref(h)) == PT_ERR_ARG
    assert not h.value and P.lib().pt_last_error()


def _cam(**kw):
    c = N.Camera()
    c.res[:] = [4, 3]
    c.position[:] = [0, 0, 5]
    c.view[:] = [0, 0, -1]
    c.up[:] = [0, 1, 0]
    c.right[:] = [1, 0, 0]
    c.pixel_length[:] = [0.01, 0.01]
    for k, v in kw.items():
        getattr(c, k)[:] = v
    return c


def test_argument_errors_need_no_device():
    L = P.lib()
    h = C.c_void_p()
    one, two = C.c_void_p(16), C.c_void_p(32)   # (never dereferenced: the checks come first)
    assert L.pt_temporal_create(0, 4, None, C.byref(h)) == PT_ERR_ARG
    assert L.pt_temporal_create(4, 0, None, C.byref(h)) == PT_ERR_ARG
    assert L.pt_temporal_create(1 << 16, 1 << 16, None, C.byref(h)) == PT_ERR_ARG
    assert L.pt_temporal_create(4, 3, None, None) == PT_ERR_ARG
    assert L.pt_temporal_create(4, 3, None, C.byref(h)) == 0 and h.value        # NULL parameters: the defaults
    cam = _cam()
    try:
        n, bs, k = C.c_int32(-1), C.c_float(-1), C.c_int32(-1)
        assert L.pt_temporal_info(h, C.byref(n), C.byref(bs), C.byref(k)) == 0
        assert (n.value, bs.value, k.value) == (0, 0.0, 0)
        # null pointers
        for args in ((None, one, 1.0, one, one, one), (C.byref(cam), None, 1.0, one, one, one),
                     (C.byref(cam), one, 1.0, None, one, one), (C.byref(cam), one, 1.0, one, None, one),
                     (C.byref(cam), one, 1.0, one, one, None)):
            assert L.pt_temporal_frame(h, *args, None) == PT_ERR_ARG
            assert L.pt_temporal_frame_host(h, *args) == PT_ERR_ARG
        # samples
        for bad in (0.0, -1.0, math.nan, math.inf):
            assert L.pt_temporal_frame(h, C.byref(cam), one, bad, one, one, one, None) == PT_ERR_ARG, bad
            assert L.pt_temporal_frame_host(h, C.byref(cam), one, bad, one, one, one) == PT_ERR_ARG, bad
        # a camera the mapping cannot be inverted for
        for bad in (_cam(view=[0, 0, 0]), _cam(right=[0, 0, 0]), _cam(up=[math.nan, 1, 0]), _cam(pixel_length=[0, 0.01]),
                    _cam(position=[math.inf, 0, 0])):
            assert L.pt_temporal_frame(h, C.byref(bad), one, 1.0, one, one, one, None) == PT_ERR_ARG
        # nothing to resolve, get or show before the first frame; aliasing outputs
        assert L.pt_temporal_resolve(h, one, None, None, None) == PT_ERR_ARG
        assert b"no frame" in L.pt_last_error()
        assert L.pt_temporal_get(h, one, None, None, None, None, None) == PT_ERR_ARG
        assert L.pt_temporal_image(h, None, one, None, None) == PT_ERR_ARG
        for outs in ((one, one, None), (one, None, one), (None, one, one)):
            assert L.pt_temporal_resolve(h, *outs, None) == PT_ERR_ARG
            assert b"alias" in L.pt_last_error()
            assert L.pt_temporal_image(h, None, *outs) == PT_ERR_ARG
            assert b"alias" in L.pt_last_error()
        assert L.pt_temporal_image(h, None, None, None, None) == PT_ERR_ARG
        bad = N.DenoiseVarParams.default()
        bad.sigma_l = 0.0
        assert L.pt_temporal_image(h, C.byref(bad), one, two, None) == PT_ERR_ARG
        assert L.pt_temporal_frame_ctx(h, None, 1.0, None) == PT_ERR_ARG
        assert L.pt_temporal_reset(h) == 0
    finally:
        assert L.pt_temporal_destroy(h) == 0
    # max_history below one batch
    assert L.pt_temporal_create(4, 3, C.byref(_prm(max_history=2.0)), C.byref(h)) == 0
    try:
        assert L.pt_temporal_frame(h, C.byref(cam), one, 4.0, one, one, one, None) == PT_ERR_ARG
        assert b"max_history" in L.pt_last_error()
    finally:
        assert L.pt_temporal_destroy(h) == 0
    # null objects
    assert L.pt_temporal_destroy(None) == 0
    assert L.pt_temporal_reset(None) == PT_ERR_ARG
    assert L.pt_temporal_info(None, None, None, None) == PT_ERR_ARG
    assert L.pt_temporal_frame(None, C.byref(cam), one, 1.0, one, one, one, None) == PT_ERR_ARG
    assert L.pt_temporal_frame_host(None, C.byref(cam), one, 1.0, one, one, one) == PT_ERR_ARG
    assert L.pt_temporal_resolve(None, one, None, None, None) == PT_ERR_ARG
    assert L.pt_temporal_get(None, one, None, None, None, None, None) == PT_ERR_ARG
    assert L.pt_temporal_image(None, None, one, None, None) == PT_ERR_ARG
    assert L.pt_temporal_frame_ctx(None, one, 1.0, None) == PT_ERR_ARG


def test_python_host_variant_refuses_another_size():
    hist = P.TemporalHistory(4, 3)
    try:
        g = {"mat": np.zeros((3, 5), np.int32), "normal": np.zeros((3, 5, 3), F), "position": np.zeros((3, 5, 3), F),
             "t": np.ones((3, 5), F), "albedo": np.ones((3, 5, 3), F)}
        with pytest.raises(ValueError, match="shape"):
            hist.frame_arrays(_cam(), np.zeros((3, 5, 3), F), 1.0, g)
        assert hist.info() == {"frames": 0, "batch_samples": 0.0, "last_case": None}
    finally:
        hist.free()


# ---- the restatement's own properties -----------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


W, H = 48, 40
CAM_A = T.look_at_camera((0.3, 1.0, 4.0), (0.0, -0.2, -3.0), 25.0, W, H)
CAM_B = T.look_at_camera((0.55, 1.05, 3.9), (0.05, -0.2, -3.0), 25.0, W, H)


def _noise(rng, samples, h=H, w=W):
    return (rng.random((h, w, 3)) * 2 * samples).astype(F)


def test_ref_same_camera_reprojects_every_pixel_centre_onto_itself_and_keeps_its_history():
    """The planar G-buffer's positions are the float32 roundings of float64 hits at t <= 12 (error
    2^-24 * 12 in world units, against a pixel footprint of t * pixel_length >= 0.02): the reprojected
    centre lies within 2^-10 pixel of the pixel, and its own tap (weight >= 1 - 2^-9) survives."""
    gA, gB, alb = T.crease_gbuffer(CAM_A, W, H)
    hit = gA[..., 3].view(np.int32) >= 0
    assert hit.all()
    fx, fy, z = T.reproject_coords(CAM_A, gB, W, H)
    xs, ys = np.meshgrid(np.arange(W), np.arange(H))
    dev = max(float(np.abs(fx - xs).max()), float(np.abs(fy - ys).max()))
    print(f"same-camera reprojection: max deviation {dev:.3e} pixel")
    assert dev <= 2.0 ** -10 and (z > 0).all()
    rng = np.random.default_rng(1)
    t = T.Temporal(H, W, max_history=0.0)
    assert t.frame(CAM_A, _noise(rng, 1), 1.0, gA, gB, alb) == T.EMPTY
    assert t.frame(CAM_A, _noise(rng, 1), 1.0, gA, gB, alb) == T.NEW_VIEW     # same camera, samples not larger
    assert t.kept.all()
    assert np.abs(t.h - 2).max() <= 2.0 ** -20


@pytest.mark.parametrize("b", [1, 4])
def test_ref_same_view_frames_count_exactly_and_average(b):
    """n same-view frames, max_history = 0: h = n * b exactly, and the mean is the running average, within
    n * 2^-22 relative of the float64 mean (per frame one division, one product, a subtraction and an
    addition, each half an ulp of a value no larger than the colours' bound)."""
    rng = np.random.default_rng(2)
    gA, gB, alb = T.crease_gbuffer(CAM_A, W, H)
    t = T.Temporal(H, W, max_history=0.0, demodulate=0)
    n = 24
    acc = np.zeros((H, W, 3), F)
    for i in range(n):
        acc = (acc + (rng.random((H, W, 3)) * b + b).astype(F)).astype(F)
        assert t.frame(CAM_A, acc, float((i + 1) * b), gA, gB, alb) == (T.EMPTY if i == 0 else T.SAME_VIEW)
    assert np.array_equal(t.h, np.full((H, W), n * b, F))
    want = acc.astype(np.float64) / (n * b)
    rel = float(np.abs(t.mean / want - 1).max())
    print(f"{n} same-view frames of {b}: mean within {rel:.3e} relative of the float64 mean")
    assert rel <= n * 2.0 ** -22


def test_ref_first_frame_is_the_batch_mean_exactly_and_misses_keep_no_history():
    rng = np.random.default_rng(3)
    gA, gB, alb = T.crease_gbuffer(CAM_A, W, H, miss_rows=(0, 1, 2))
    miss = gA[..., 3].view(np.int32) < 0
    assert miss.any() and not miss.all()
    t = T.Temporal(H, W)
    rgb = _noise(rng, 4)
    t.frame(CAM_A, rgb, 4.0, gA, gB, alb)
    c = (rgb / F(4)).astype(F)
    c = np.where(alb[..., :3] >= F(2.0 ** -10), c / alb[..., :3], c).astype(F)
    assert np.array_equal(_bits(t.mean), _bits(c))                      # 0 + 1 * (c - 0)
    assert np.array_equal(t.h, np.full((H, W), 4, F))
    rgb2 = (rgb + _noise(rng, 4)).astype(F)
    t.frame(CAM_A, rgb2, 8.0, gA, gB, alb)
    assert (t.h[miss] == 4).all() and (t.h[~miss] == 8).all()
    _, var, _ = t.resolve()
    assert not var[miss].any()


def _moved(**params):
    rng = np.random.default_rng(4)
    gA, gB, alb = T.crease_gbuffer(CAM_A, W, H)
    t = T.Temporal(H, W, **params)
    t.frame(CAM_A, _noise(rng, 1), 1.0, gA, gB, alb)
    t.frame(CAM_A, _noise(rng, 2), 2.0, gA, gB, alb)
    return t, rng


def test_ref_taps_of_another_material_a_turned_normal_or_off_the_plane_are_dropped():
    gA2, gB2, alb2 = T.crease_gbuffer(CAM_B, W, H)
    t, rng = _moved()
    t.frame(CAM_B, _noise(rng, 1), 1.0, gA2, gB2, alb2)
    base = t.kept.copy()
    assert base.mean() > 0.5
    # another material in the new frame: no tap of the old frame matches
    t, rng = _moved()
    g = gA2.copy()
    g[..., 3] = np.where(g[..., 3].view(np.int32) == 1, 7, g[..., 3].view(np.int32)).astype(np.int32).view(F)
    t.frame(CAM_B, _noise(rng, 1), 1.0, g, gB2, alb2)
    was_floor = gA2[..., 3].view(np.int32) == 1
    assert not t.kept[was_floor].any() and (t.h[was_floor] == 1).all()
    assert np.array_equal(t.kept[~was_floor], base[~was_floor])
    # normals turned by 60 degrees (cos = 0.5 < min_ndot = 0.9) on the floor
    t, rng = _moved()
    g = gA2.copy()
    g[was_floor, :3] = (0.0, 0.5, math.sqrt(0.75))
    t.frame(CAM_B, _noise(rng, 1), 1.0, g, gB2, alb2)
    assert not t.kept[was_floor].any()
    # positions lifted off the plane by 5% of the hit distance (plane_tol = 2%)
    t, rng = _moved()
    g = gB2.copy()
    g[was_floor, 1] += F(0.05) * g[was_floor, 3]
    t.frame(CAM_B, _noise(rng, 1), 1.0, gA2, g, alb2)
    fx, fy, _ = T.reproject_coords(CAM_A, g, W, H)
    inside = (fx >= 0) & (fx < W - 1) & (fy >= 0) & (fy < H - 1)
    assert (inside & was_floor).any() and not t.kept[was_floor].any()
    # ... and kept with a tolerance above the lift
    t, rng = _moved(plane_tol=0.2)
    t.frame(CAM_B, _noise(rng, 1), 1.0, gA2, g, alb2)
    assert t.kept[was_floor].any()


def test_ref_no_surviving_tap_gives_h_equal_b_and_the_clamp_holds():
    gA2, gB2, alb2 = T.crease_gbuffer(CAM_B, W, H)
    t, rng = _moved(max_history=2.5)
    assert t.h.max() == 2.0
    rgb = _noise(rng, 1)
    t.frame(CAM_B, rgb, 1.0, gA2, gB2, alb2)
    lost = ~t.kept
    assert lost.any() and t.kept.any()
    assert (t.h[lost] == 1).all()
    c = np.where(alb2[..., :3] >= F(2.0 ** -10), rgb / alb2[..., :3], rgb).astype(F)
    assert np.array_equal(_bits(t.mean[lost]), _bits(c[lost]))
    assert t.h.max() == F(2.5)                                           # 2 + 1, clamped
    with pytest.raises(ValueError):
        t.frame(CAM_A, _noise(rng, 3), 3.0, gA2, gB2, alb2)             # another batch size
    with pytest.raises(ValueError):
        T.Temporal(H, W, max_history=2.0).frame(CAM_A, _noise(rng, 3), 3.0, gA2, gB2, alb2)


def test_ref_variance_is_temporal_with_history_and_spatial_without():
    """Grey noise of sigma = 0.3 per sample on one surface.  Without history (one frame) the 5 x 5
    estimate sees 25 independent pixels: its mean over the image is 24/25 sigma^2 within 5%.  After 16
    same-view frames the temporal estimate of the variance of the mean is sigma^2 * (15/16) / 16 within
    10% (its own spread, sqrt(2/15) per pixel, averages out over 1,920 pixels)."""
    rng = np.random.default_rng(5)
    gA, gB, alb = T.crease_gbuffer(CAM_A, W, H)
    gA[..., :3], gA[..., 3] = (0, 0, 1), np.ones((H, W), np.int32).view(F)   # one material throughout
    t = T.Temporal(H, W, max_history=0.0, demodulate=0)
    acc = np.zeros((H, W, 3), F)
    sigma = 0.3
    for i in range(16):
        acc = (acc + np.broadcast_to(rng.normal(1.0, sigma, (H, W, 1)), (H, W, 3)).astype(F)).astype(F)
        t.frame(CAM_A, acc, float(i + 1), gA, gB, alb)
        if i == 0:
            _, var, _ = t.resolve()
            assert not t.on_temporal.any()
            inner = float(var[2:-2, 2:-2].mean())
            assert abs(inner / (sigma ** 2 * 24 / 25) - 1) <= 0.05, inner
    _, var, h = t.resolve()
    assert t.on_temporal.all() and (h == 16).all()
    got = float(var.mean())
    assert abs(got / (sigma ** 2 * (15 / 16) / 16) - 1) <= 0.10, got


# ---- the preview's setting ------------------------------------------------------------------------
class FakeCtx:
    spp = 1

    def __init__(self, h, w, log, cam):
        self.h, self.w, self.log, self.cam, self.passes = h, w, log, cam, 0

    def set_flags(self, gui):
        self.log.append(("flags",))

    def render_pass(self, it):
        self.passes = it
        self.log.append(("pass", it))

    def image(self):
        return np.full((self.h, self.w, 3), 0.5 * self.passes, np.float32)

    def gbuffer(self):
        return {"mat": np.zeros((self.h, self.w), np.int32)}

    def free(self):
        self.log.append(("ctx_free",))


class FakeHistory:
    """Counts frames and enforces pt_temporal_frame's batch rule (temporal_case): a frame of the stored
    camera with more samples is a batch of the difference, any other a batch of its samples, and every
    batch since the last reset has the size of the first."""

    def __init__(self, w, h, log):
        self.w, self.h, self.log = w, h, log
        self.frames, self.length, self.freed = 0, 0, False
        self.cam, self.samples, self.batch = None, 0, None

    def _take(self, cam, samples):
        assert not self.freed and samples > 0
        same = self.frames > 0 and cam == self.cam and samples > self.samples
        b = samples - self.samples if same else samples
        if self.frames > 0 and b != self.batch:
            raise P.PtError(PT_ERR_ARG, "the frame's batch size differs from the first frame's since the last reset")
        self.cam, self.samples, self.batch = cam, samples, b
        self.frames += 1
        self.length += 1

    def frame(self, tracer, samples, stream=None):
        self._take(tracer.cam, samples)
        self.log.append(("frame", id(tracer), samples))

    def frame_arrays(self, camera, image, samples, gbuffer):
        assert image.shape == (self.h, self.w, 3) and "mat" in gbuffer
        self._take(bytes(camera), samples)
        self.log.append(("frame_arrays", samples, float(image[0, 0, 0])))

    def image(self, var_params=None, return_variance=False, return_history=False):
        assert var_params is not None and return_history and not return_variance
        self.log.append(("image",))
        return np.full((self.h, self.w, 3), 0.75, np.float32), np.full((self.h, self.w), self.length, np.float32)

    def info(self):
        return {"frames": self.frames, "batch_samples": 1.0, "last_case": "same_view"}

    def reset(self):
        self.frames = self.length = 0
        self.cam, self.samples, self.batch = None, 0, None
        self.log.append(("reset",))

    def free(self):
        self.freed = True
        self.log.append(("history_free",))


def _session(tmp_path):
    s = P.Scene(str(SCENES / "cornell.json"))
    log, made, hists = [], [], []

    def factory(scene, gui):
        c = FakeCtx(scene.camera().res[1], scene.camera().res[0], log, bytes(scene.camera()))
        made.append(c)
        return c

    def read(ctx, it):
        a = np.zeros((ctx.h, ctx.w, 4), np.uint8)
        a[..., 0] = it
        return a

    def history(w, h):
        hists.append(FakeHistory(w, h, log))
        return hists[-1]

    ses = V.PreviewSession(s, out_dir=str(tmp_path), tracer_factory=factory, read_preview=read, history_factory=history)
    return ses, log, made, hists


def test_preview_setting_is_off_by_default_and_then_nothing_changes(tmp_path):
    ses, log, made, hists = _session(tmp_path)
    assert ses.state()["settings"]["denoise_temporal"] is False and "temporal" not in ses.state()
    for _ in range(3):
        ses.run_cuda()
    assert ses.iteration == 3 and ses.rgba[0, 0, 0] == 3 and not hists
    assert not [e for e in log if e[0] not in ("flags", "pass")]
    assert "denoise_temporal" in V._PAGE
    with pytest.raises(ValueError, match="unknown setting"):
        ses.set_setting("denoise_temporally", True)
    ses.close()


def test_preview_keeps_one_history_across_a_camera_restart(tmp_path):
    ses, log, made, hists = _session(tmp_path)
    ses.set_setting("denoise_temporal", True)
    assert not ses.visual_changed                                         # display only
    ses.run_cuda()
    ses.run_cuda()
    ses.run_cuda()
    assert ses.iteration == 3 and len(made) == 1 and len(hists) == 1
    assert [e for e in log if e[0] in ("frame", "image")][-2:] == [("frame", id(made[0]), 3), ("image",)]
    assert (ses.display_rgb() == 191).all()                               # the history's image, tonemapped
    assert ses.state()["temporal"] == {"frames": 3, "mean_history": 3.0}
    ses.mouse_button(V.MOUSE_LEFT, V.PRESS)
    ses.mouse_move(10.0, 10.0)
    ses.mouse_move(14.0, 12.0)                                            # an orbit: camchanged
    assert ses.camchanged
    ses.run_cuda()
    assert len(made) == 2 and ses.iteration == 1 and len(hists) == 1      # a new context, the same history
    assert ("reset",) not in log and not hists[0].freed
    assert log[-2] == ("frame", id(made[1]), 1)
    assert ses.state()["temporal"] == {"frames": 4, "mean_history": 4.0}
    ses.key("S")                                                          # saving: the raw accumulator
    assert len(ses.saved) == 1 and ses.saved[0].endswith(".1samp.png")
    ses.close()
    assert hists[0].freed


def test_preview_resets_the_history_on_a_visual_setting_and_frees_it_when_switched_off(tmp_path):
    ses, log, made, hists = _session(tmp_path)
    ses.set_setting("denoise_temporal", True)
    ses.run_cuda()
    ses.run_cuda()
    ses.set_setting("SSAA", False)                                        # a visual setting: another image
    ses.run_cuda()
    assert len(made) == 2 and ses.iteration == 1 and len(hists) == 1
    assert log.count(("reset",)) == 1 and log.index(("reset",)) < log.index(("frame", id(made[1]), 1))
    assert ses.state()["temporal"] == {"frames": 1, "mean_history": 1.0}
    ses.set_setting("russianRoulette", False)                             # a general setting: nothing
    ses.run_cuda()
    assert log.count(("reset",)) == 1 and len(made) == 2
    ses.set_setting("denoise_temporal", False)
    assert hists[0].freed and "temporal" not in ses.state()
    ses.run_cuda()
    assert ses.iteration == 3 and len(made) == 2 and ses.rgba[0, 0, 0] == 3   # the PBO again, no restart
    ses.set_setting("denoise_temporal", True)
    ses.run_cuda()
    ses.run_cuda()
    assert len(hists) == 2 and hists[1].frames == 2
    ses.close()


def test_preview_switched_on_mid_accumulation_feeds_one_sample_batches(tmp_path):
    """Switched on after k passes, the history gets what the context accumulates from then on (the
    accumulator's gain, samples counted from k), so its batches are of one sample like every other frame's;
    a frame of the whole accumulator would be a batch of k + 1 followed by batches of 1, which it refuses."""
    ses, log, made, hists = _session(tmp_path)
    for _ in range(3):
        ses.run_cuda()
    ses.set_setting("denoise_temporal", True)
    for _ in range(3):
        ses.run_cuda()
    assert ses.iteration == 6 and len(made) == 1 and len(hists) == 1      # no restart
    fed = [e for e in log if e[0] in ("frame", "frame_arrays")]
    assert fed == [("frame_arrays", 1, 0.5), ("frame_arrays", 2, 1.0), ("frame_arrays", 3, 1.5)]
    assert ses.state()["temporal"] == {"frames": 3, "mean_history": 3.0}
    ses.key("S")                                                          # saving: the whole accumulator
    assert ses.saved[0].endswith(".6samp.png")
    ses.set_setting("denoise_temporal", False)                            # off and on again, still mid-accumulation
    ses.run_cuda()
    ses.set_setting("denoise_temporal", True)
    ses.run_cuda()
    ses.run_cuda()
    assert len(hists) == 2 and [e for e in log if e[0] == "frame_arrays"][-2:] == [("frame_arrays", 1, 0.5), ("frame_arrays", 2, 1.0)]
    ses.mouse_button(V.MOUSE_LEFT, V.PRESS)                               # a camera move: a new context, the
    ses.mouse_move(10.0, 10.0)                                            # whole accumulator again
    ses.mouse_move(14.0, 12.0)
    ses.run_cuda()
    ses.run_cuda()
    assert len(made) == 2 and [e for e in log if e[0] in ("frame", "frame_arrays")][-2:] == \
        [("frame", id(made[1]), 1), ("frame", id(made[1]), 2)]
    assert hists[1].frames == 4
    ses.close()
