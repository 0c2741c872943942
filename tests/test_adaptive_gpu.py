"""Adaptive sampling and region rendering on the GPU.

The object (pt_adaptive) is compared bit for bit with the numpy float32 restatement
(tests/adaptive_ref.py); a NaN equals a NaN whatever its payload.  The render oracle needs no reference
renderer: under rng_key_pixel a pass traced through a block mask must give every pixel of an active block
the bits of the same pass traced in full, and must leave every other pixel's accumulator as it was."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

import cuda_pathtracer_amd as P
from cuda_pathtracer_amd import _native as N

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "scripts"))
import adaptive_ref as A  # noqa: E402
import denoise_var_ref as RV  # noqa: E402
from test_adaptive_cpu import E2E  # noqa: E402
from test_denoise_var_gpu import _accumulators, _albedo  # noqa: E402  (the moments tests' data)

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
SCENES = ROOT / "tests" / "scenes"
F = np.float32
PT_ERR_ARG = 1
SHAPES = [(1, 1), (70, 1), (72, 40), (64, 64), (130, 67)]   # (width, height)


def _same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype == F:
        bad = (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))
    else:
        bad = got != want
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4], want[bad][:4])


class _Ad:
    def __init__(self, w, h):
        self.L, self.w, self.h = P.lib(), w, h
        self.a = C.c_void_p()
        N.check_pt(self.L.pt_adaptive_obj_create(w, h, C.byref(self.a)))
        self.nblk = A.nblocks(h, w)

    def close(self):
        self.L.pt_adaptive_obj_destroy(self.a)

    def get(self):
        h, w = self.h, self.w
        m1, m2, prev = np.empty((h, w), F), np.empty((h, w), F), np.empty((h, w, 3), F)
        nb, act, hot = np.empty(self.nblk, np.uint32), np.empty(self.nblk, np.uint32), np.empty((h, w), np.uint8)
        N.check_pt(self.L.pt_adaptive_obj_get(self.a, m1.ctypes.data, m2.ctypes.data, prev.ctypes.data, nb.ctypes.data,
                                              act.ctypes.data, hot.ctypes.data))
        return dict(m1=m1, m2=m2, prev=prev, nb=nb, act=act, hot=hot)

    def check(self, ref, what, hot=True):
        got = self.get()
        for k in ("m1", "m2", "prev", "nb", "act") + (("hot",) if hot else ()):
            _same(got[k], getattr(ref, k), (what, k))


def _prm(threshold, floor, min_batches, dilate):
    p = N.AdaptiveParams.default()
    p.threshold, p.floor, p.min_batches, p.dilate = threshold, floor, min_batches, dilate
    return p


# ---- the object against the restatement -------------------------------------------------------------------
@pytest.mark.parametrize("use_alb", [False, True], ids=["plain", "albedo"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_object_equals_the_restatement_bitwise(gpu_device, shape, use_alb):
    import torch
    w, h = shape
    bs = 4.0
    rng = np.random.default_rng(900 + 7 * w + h)
    acc = _accumulators(h, w, rng, 6, bs)
    for b in range(3, 7):
        acc[b][0, 0, 1] = np.nan                       # NaN moments in block 0 from the third batch on
    alb = _albedo(h, w, rng) if use_alb else None
    d_alb = torch.from_numpy(alb).to(gpu_device) if use_alb else None
    st = torch.cuda.current_stream().cuda_stream
    ad = _Ad(w, h)
    nblk = ad.nblk
    try:
        N.check_pt(ad.L.pt_adaptive_obj_reset(ad.a, torch.from_numpy(acc[0]).to(gpu_device).data_ptr(), st))
        ref = A.Adaptive(h, w, acc[0])
        ad.check(ref, "reset")
        for b in range(1, 7):
            mask = (rng.random(nblk) < 0.6).astype(np.uint8)
            if b == 1:
                mask[:] = 1
            mask[0] = b != 5                               # block 0 is mostly on (its NaN reaches the moments)
            N.check_pt(ad.L.pt_adaptive_obj_set_mask(ad.a, mask.ctypes.data, nblk, st))
            ref.set_mask(mask)
            rgb = acc[b].copy()
            rgb[A.expand(mask, h, w) == 0] = np.nan        # the input of inactive blocks is not read
            d_rgb = torch.from_numpy(rgb).to(gpu_device)
            N.check_pt(ad.L.pt_adaptive_obj_update(ad.a, d_rgb.data_ptr(), bs, d_alb.data_ptr() if use_alb else None, st))
            ref.update(rgb, bs, alb)
            ad.check(ref, ("update", b), hot=False)
        assert np.isnan(ref.m1[0, 0])
        if nblk > 2:
            assert (ref.nb < 4).any() and (ref.nb >= 4).any() and ref.nb.max() <= 6
        nbk, nup, gbs = C.c_int32(), C.c_int32(), C.c_float()
        N.check_pt(ad.L.pt_adaptive_obj_info(ad.a, C.byref(nbk), C.byref(nup), C.byref(gbs)))
        assert (nbk.value, nup.value, gbs.value) == (nblk, 6, bs)
        # a changed batch size is refused, and the object goes on as it was
        assert ad.L.pt_adaptive_obj_update(ad.a, d_rgb.data_ptr(), bs + 1.0, None, st) == PT_ERR_ARG
        ad.check(ref, "after the refused update", hot=False)
        # resolve: per-block counts
        d_acc = torch.from_numpy(acc[6]).to(gpu_device)
        d_out = torch.full((h, w, 3), 7.0, dtype=torch.float32, device=gpu_device)
        d_var = torch.full((h, w), 7.0, dtype=torch.float32, device=gpu_device)
        N.check_pt(ad.L.pt_adaptive_obj_resolve(ad.a, d_acc.data_ptr(), d_out.data_ptr(), d_var.data_ptr(), st))
        torch.cuda.synchronize()
        r_out, r_var = ref.resolve(acc[6])
        _same(d_out.cpu().numpy(), r_out, "resolve rgb")
        _same(d_var.cpu().numpy(), r_var, "resolve var")
        N.check_pt(ad.L.pt_adaptive_obj_resolve(ad.a, d_acc.data_ptr(), None, d_var.data_ptr(), st))   # either alone
        N.check_pt(ad.L.pt_adaptive_obj_resolve(ad.a, d_acc.data_ptr(), d_out.data_ptr(), None, st))
        torch.cuda.synchronize()
        _same(d_out.cpu().numpy(), r_out, "resolve rgb alone")
        _same(d_var.cpu().numpy(), r_var, "resolve var alone")
        # apply
        cm = rng.integers(0, 2 ** 32, nblk, dtype=np.uint64).astype(np.uint32)
        cm[rng.random(nblk) < 0.3] = 0
        d_cm = torch.from_numpy(cm.view(np.int32)).to(gpu_device)
        d_eff = torch.full((nblk,), -1, dtype=torch.int32, device=gpu_device)
        N.check_pt(ad.L.pt_adaptive_obj_apply(ad.a, d_cm.data_ptr(), d_eff.data_ptr(), st))
        torch.cuda.synchronize()
        _same(d_eff.cpu().numpy().view(np.uint32), ref.apply(cm), "apply")
        # select from the same moments at every dilation, the threshold exactly on a pixel's e
        e = ref.error(0.05)
        ok = np.isfinite(e) & (A.expand(ref.nb, h, w) >= 4) & (e > 0)
        tau = float(np.median(e[ok])) if ok.any() else 0.25
        if ok.any():
            tau = float(e[ok][np.argmin(np.abs(e[ok] - tau))])         # one pixel has e == tau: not hot
        for r in (0, 1, 2):
            for t in (tau, 0.0, 1e30):
                act, nb_out = C.c_int32(-1), C.c_int32(-1)
                N.check_pt(ad.L.pt_adaptive_obj_select(ad.a, C.byref(_prm(t, 0.05, 4, r)), st, C.byref(act), C.byref(nb_out)))
                n = ref.select(t, 0.05, 4, r)
                assert (act.value, nb_out.value) == (n, nblk), (r, t)
                ad.check(ref, ("select", r, t))
                if t == 0.0:                                        # the NaN pixel (block 0 has 5 batches) is not hot
                    assert ref.nb[0] == 5 and np.isnan(e[0, 0]) and ref.hot[0, 0] == 0
                if ok.any() and t == tau:
                    at = ok & (e == F(tau))
                    assert at.any() and not ref.hot[at].any() and ref.hot[ok & (e > F(tau))].all()
    finally:
        ad.close()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_resolve_with_zero_one_and_more_batches_in_one_image(gpu_device, shape):
    import torch
    w, h = shape
    rng = np.random.default_rng(40 + w)
    acc = _accumulators(h, w, rng, 3, 1.0)
    st = torch.cuda.current_stream().cuda_stream
    ad = _Ad(w, h)
    try:
        ref = A.Adaptive(h, w)
        N.check_pt(ad.L.pt_adaptive_obj_reset(ad.a, None, st))
        want = np.array(([0, 1] + [3] * ad.nblk)[:ad.nblk]) if ad.nblk > 1 else np.array([3])
        for b in range(1, 4):
            mask = (want >= b).astype(np.uint8)
            N.check_pt(ad.L.pt_adaptive_obj_set_mask(ad.a, mask.ctypes.data, ad.nblk, st))
            ref.set_mask(mask)
            d_rgb = torch.from_numpy(acc[b]).to(gpu_device)
            N.check_pt(ad.L.pt_adaptive_obj_update(ad.a, d_rgb.data_ptr(), 1.0, None, st))
            ref.update(acc[b], 1.0)
        assert ref.nb.tolist() == want.tolist()
        d_out = torch.empty((h, w, 3), dtype=torch.float32, device=gpu_device)
        d_var = torch.empty((h, w), dtype=torch.float32, device=gpu_device)
        N.check_pt(ad.L.pt_adaptive_obj_resolve(ad.a, d_rgb.data_ptr(), d_out.data_ptr(), d_var.data_ptr(), st))
        torch.cuda.synchronize()
        r_out, r_var = ref.resolve(acc[3])
        _same(d_out.cpu().numpy(), r_out, "rgb")
        _same(d_var.cpu().numpy(), r_var, "var")
        nbp = A.expand(ref.nb, h, w)
        assert not r_out[nbp == 0].any() and not r_var[nbp < 2].any()
        ad.check(ref, "state")
    finally:
        ad.close()


@pytest.mark.parametrize("aligned", [True, False], ids=["vector", "one-pixel"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_all_blocks_active_equals_pt_moments_bitwise(gpu_device, shape, aligned):
    import torch
    w, h = shape
    bs = 4.0
    rng = np.random.default_rng(77 + w + h)
    acc = _accumulators(h, w, rng, 5, bs)
    alb = _albedo(h, w, rng)
    d_alb = torch.from_numpy(alb).to(gpu_device)
    st = torch.cuda.current_stream().cuda_stream
    L = P.lib()
    ad = _Ad(w, h)
    mom = C.c_void_p()
    N.check_pt(L.pt_moments_create(w, h, C.byref(mom)))
    try:
        for b in range(1, 6):
            buf = torch.zeros(h * w * 3 + 4, dtype=torch.float32, device=gpu_device)
            view = buf[0:h * w * 3] if aligned else buf[1:h * w * 3 + 1]
            view.copy_(torch.from_numpy(acc[b].reshape(-1)))
            assert view.data_ptr() % 16 == (0 if aligned else 4)
            N.check_pt(L.pt_adaptive_obj_update(ad.a, view.data_ptr(), bs, d_alb.data_ptr(), st))
            N.check_pt(L.pt_moments_update(mom, view.data_ptr(), bs, d_alb.data_ptr(), st))
        m1, m2, prev = np.empty((h, w), F), np.empty((h, w), F), np.empty((h, w, 3), F)
        N.check_pt(L.pt_moments_get(mom, m1.ctypes.data, m2.ctypes.data, prev.ctypes.data))
        got = ad.get()
        _same(got["m1"], m1, "m1")
        _same(got["m2"], m2, "m2")
        _same(got["prev"], prev, "prev")
        assert (got["nb"] == 5).all() and (got["act"] == 1).all()
        d_var = torch.empty((h, w), dtype=torch.float32, device=gpu_device)
        d_mvar = torch.empty((h, w), dtype=torch.float32, device=gpu_device)
        N.check_pt(L.pt_adaptive_obj_resolve(ad.a, view.data_ptr(), None, d_var.data_ptr(), st))
        N.check_pt(L.pt_moments_variance(mom, 5 * bs, d_mvar.data_ptr(), st))
        torch.cuda.synchronize()
        _same(d_var.cpu().numpy(), d_mvar.cpu().numpy(), "variance")
        ref = RV.Moments(h, w)
        for b in range(1, 6):
            ref.update(acc[b], bs, alb)
        _same(got["m1"], ref.m1, "m1 against the restatement")
    finally:
        ad.close()
        L.pt_moments_destroy(mom)


# ---- the render oracle ------------------------------------------------------------------------------------
def _scene(w, h, name="cornell.json"):
    s = P.Scene(str(SCENES / name))
    s.set_camera((w, h), 45.0, (0, 5, 10.5), (0, 5, 0), (0, 1, 0))
    s.finalize()
    return s


def _gui(key=True, sort=False, aperture=None):
    g = P.GuiDataContainer()
    g.rngKeyPixel, g.sortbyMaterial = key, sort
    if aperture is not None:
        g.aperture = aperture
    return g


def _masks(nblk, seed):
    rng = np.random.default_rng(seed)
    half = np.zeros(nblk, np.uint8)
    half[rng.permutation(nblk)[:nblk // 2]] = 1
    tile = np.ones(nblk, np.uint8)
    tile[4:8] = 0                                            # pixels 256..511: one aligned 256-pixel tile
    return {"random-half": half, "checkerboard": (np.arange(nblk) % 2).astype(np.uint8), "tile-off": tile,
            "all-off": np.zeros(nblk, np.uint8), "all-on": np.ones(nblk, np.uint8)}


def _split(img, mask):
    h, w = img.shape[:2]
    on = A.expand(mask, h, w) != 0
    return on, ~on


def _oracle(full_final, masked, before, mask, what):
    """Every pixel is in one of the two sets: active == the full render's, inactive == its own from before."""
    on, off = _split(full_final, mask)
    assert int(on.sum()) + int(off.sum()) == on.size
    _same(masked[on], full_final[on], (what, "active pixels"))
    _same(masked[off], before[off], (what, "inactive pixels"))


@pytest.mark.parametrize("skip", ["0", "1"], ids=["noskip", "skip"])
@pytest.mark.parametrize("sort", [False, True], ids=["fused", "sorted"])
@pytest.mark.parametrize("spp", [1, 4])
@pytest.mark.parametrize("res", [(72, 40), (64, 64)], ids=lambda r: f"{r[0]}x{r[1]}")
def test_masked_passes_equal_full_passes_on_active_pixels_and_leave_the_rest(gpu_device, monkeypatch, res, spp, sort, skip):
    monkeypatch.setenv("PT_AMD_SKIP_EMPTY", skip)
    w, h = res
    scene = _scene(w, h)
    nblk = A.nblocks(h, w)
    ctx_a = P.PathTracer(scene, _gui(sort=sort), spp=spp)
    assert ctx_a.cmask_info()["on"] and ctx_a.cmask_info()["skip_fused"] == (skip == "1")
    for k in range(2):
        ctx_a.render_pass(1 + k * spp)
    a_half, live_half = ctx_a.image(), ctx_a.stats()["bounce_live"]
    for k in range(2, 4):
        ctx_a.render_pass(1 + k * spp)
    a_final, live_final = ctx_a.image(), ctx_a.stats()["bounce_live"]
    a_live1 = live_final[1] - live_half[1]
    ctx_a.free()
    assert a_live1 > 0
    for name, mask in _masks(nblk, 5 * w + spp).items():
        ctx_b = P.PathTracer(scene, _gui(sort=sort), spp=spp)
        ctx_b.adaptive(True)
        for k in range(2):
            ctx_b.render_pass(1 + k * spp)
            ctx_b.adaptive_update()
        before = ctx_b.image()
        _same(before, a_half, (name, "the first half"))
        st0 = ctx_b.stats()["bounce_live"]
        ctx_b.adaptive_set_mask(mask)
        info = ctx_b.adaptive_info()
        assert (info["on"], info["blocks"], info["active_blocks"]) == (True, nblk, int(mask.sum()))
        assert ctx_b.cmask_info()["skip_fused"] == (skip == "1")           # PT_AMD_SKIP_EMPTY still decides
        for k in range(2, 4):
            ctx_b.render_pass(1 + k * spp)
            ctx_b.adaptive_update()
        st1 = ctx_b.stats()["bounce_live"]
        _oracle(a_final, ctx_b.image(), before, mask, name)
        b_live1 = st1[1] - st0[1]
        assert st1[0] - st0[0] == 2 * spp * w * h                          # bounce_live[0] counts every pixel
        if name == "all-off":
            assert b_live1 == 0
        elif name == "all-on":
            assert b_live1 == a_live1
        else:
            assert 0 < b_live1 < a_live1
        state = ctx_b.adaptive_state()
        assert np.array_equal(state["act"], mask) and np.array_equal(state["nb"], 2 + 2 * mask.astype(np.uint32))
        ctx_b.free()


@pytest.mark.parametrize("sort", [False, True], ids=["fused", "sorted"])
def test_all_blocks_on_without_pixel_keys_equals_an_ordinary_context(gpu_device, sort):
    w, h, spp = 72, 40, 4
    scene = _scene(w, h)
    plain = P.PathTracer(scene, _gui(key=False, sort=sort), spp=spp)
    ad = P.PathTracer(scene, _gui(key=False, sort=sort), spp=spp)
    ad.adaptive(True)
    for k in range(4):
        if k == 2:
            ad.adaptive_set_mask(np.ones(A.nblocks(h, w), np.uint8))
        plain.render_pass(1 + k * spp)
        ad.render_pass(1 + k * spp)
        ad.adaptive_update()
    _same(ad.image(), plain.image(), "image")
    assert ad.stats() == plain.stats()
    ad.adaptive(False)                                       # and off again: the camera masks are back
    assert not ad.adaptive_info()["on"] and ad.cmask_info() == plain.cmask_info()
    plain.render_pass(17)
    ad.render_pass(17)
    _same(ad.image(), plain.image(), "image after adaptive(False)")
    plain.free()
    ad.free()


# ---- glue ---------------------------------------------------------------------------------------------------
def _refused(fn, *words):
    with pytest.raises(P.PtError) as e:
        fn()
    assert e.value.code == PT_ERR_ARG
    for wd in words:
        assert wd in str(e.value), str(e.value)


def test_enable_is_refused_where_a_zeroed_word_would_not_gate_the_first_bounce(gpu_device, monkeypatch):
    mesh = P.Scene(str(SCENES / "room.json"))
    ctx = P.PathTracer(mesh, _gui())
    _refused(lambda: ctx.adaptive(True), "camera masks")
    ctx.free()
    scene = _scene(72, 40)
    ctx = P.PathTracer(scene, _gui(), rank=0, world=2)
    _refused(lambda: ctx.adaptive(True), "world == 1")
    ctx.free()
    ctx = P.PathTracer(scene, _gui())
    ctx.track_variance(True)
    _refused(lambda: ctx.adaptive(True), "pt_track_variance")
    ctx.track_variance(False)
    ctx.adaptive(True)
    ctx.adaptive(True)                                       # (a no-op when already on)
    _refused(lambda: ctx.track_variance(True), "adaptive")
    _refused(lambda: ctx.set_image(ctx.image()), "pt_set_accum")
    _refused(lambda: ctx.adaptive_set_mask(np.ones(A.nblocks(40, 72) + 1, np.uint8)), "mask length")
    _refused(lambda: ctx.adaptive_select(_prm(-1.0, 0.01, 4, 1)), "threshold")
    _refused(lambda: ctx.adaptive_image(), "update")
    ctx.free()
    with monkeypatch.context() as m:
        m.setenv("PT_PIPELINE", "split")
        ctx = P.PathTracer(scene, _gui())
        _refused(lambda: ctx.adaptive(True), "split")
        ctx.free()
        ctx = P.PathTracer(scene, _gui(sort=True))           # (the sorted pipeline runs whatever PT_PIPELINE says)
        ctx.adaptive(True)
        _refused(lambda: ctx.set_flags(_gui(sort=False)), "split")
        ctx.free()
    with monkeypatch.context() as m:
        m.setenv("PT_AMD_NO_CMASK", "1")
        ctx = P.PathTracer(scene, _gui())
        _refused(lambda: ctx.adaptive(True), "PT_AMD_NO_CMASK")
        ctx.free()
    with monkeypatch.context() as m:
        m.setenv("PT_AMD_VERIFY_BOUNDS", "1")
        ctx = P.PathTracer(scene, _gui(sort=True))
        _refused(lambda: ctx.adaptive(True), "PT_AMD_VERIFY_BOUNDS")
        ctx.free()


def test_mask_survives_a_camera_mask_rebuild(gpu_device):
    w, h, spp = 72, 40, 1
    scene = _scene(w, h)
    mask = (np.arange(A.nblocks(h, w)) % 2).astype(np.uint8)
    full = P.PathTracer(scene, _gui(), spp=spp)
    part = P.PathTracer(scene, _gui(), spp=spp)
    part.adaptive(True)
    for it in (1, 2):
        full.render_pass(it)
        part.render_pass(it)
    before = part.image()
    part.adaptive_set_mask(mask)
    builds = part.counters()["mask_builds"]
    for c in (full, part):
        c.set_flags(_gui(aperture=0.4))
    assert part.counters()["mask_builds"] == builds + 1
    assert np.array_equal(part.adaptive_state()["act"], mask) and part.adaptive_info()["active_blocks"] == int(mask.sum())
    for it in (3, 4):
        full.render_pass(it)
        part.render_pass(it)
    _oracle(full.image(), part.image(), before, mask, "after an aperture change")
    full.free()
    part.free()


def test_reset_image_makes_every_block_active_again(gpu_device):
    w, h = 72, 40
    ctx = P.PathTracer(_scene(w, h), _gui(), spp=4)
    ctx.adaptive(True)
    ctx.render_pass(1)
    ctx.adaptive_update()
    ctx.adaptive_set_mask(np.zeros(A.nblocks(h, w), np.uint8))
    ctx.reset_image()
    s = ctx.adaptive_state()
    assert (s["act"] == 1).all() and (s["nb"] == 0).all() and not s["m1"].any() and not s["prev"].any()
    info = ctx.adaptive_info()
    assert info["active_blocks"] == info["blocks"] and info["updates"] == 0
    fresh = P.PathTracer(_scene(w, h), _gui(), spp=4)
    ctx.render_pass(1)
    fresh.render_pass(1)
    _same(ctx.image(), fresh.image(), "the pass after the reset")
    ctx.free()
    fresh.free()


def test_render_ahead_queued_before_a_mask_change_is_dropped(gpu_device):
    w, h = 72, 40
    scene = _scene(w, h)
    mask = (np.arange(A.nblocks(h, w)) % 3 == 0).astype(np.uint8)
    ahead, plain = (P.PathTracer(scene, _gui()) for _ in range(2))
    for c in (ahead, plain):
        c.adaptive(True)
        c.render_pass(1)
    ahead.render_ahead(2)                                    # traced through the full mask: must not be claimed
    for c in (ahead, plain):
        c.adaptive_set_mask(mask)
        c.render_pass(2)
    _same(ahead.image(), plain.image(), "image")
    assert ahead.stats() == plain.stats()
    ahead.free()
    plain.free()


def test_adaptive_image_equals_resolve_and_the_host_filter(gpu_device):
    w, h, spp = 72, 40, 4
    ctx = P.PathTracer(_scene(w, h), _gui(), spp=spp)
    ctx.adaptive(True)
    want = np.array(([0, 1] + [3] * 64)[:A.nblocks(h, w)])
    ctx.adaptive_set_mask(want >= 1)
    for b in range(1, 4):
        ctx.adaptive_set_mask(want >= b)
        ctx.render_pass(1 + (b - 1) * spp)
        ctx.adaptive_update()
    s = ctx.adaptive_state()
    assert s["nb"].tolist() == want.tolist()
    ref = A.Adaptive(h, w)
    ref.m1, ref.m2, ref.nb, ref.batch_samples = s["m1"], s["m2"], s["nb"], float(spp)
    acc = ctx.image()
    r_out, r_var = ref.resolve(acc)
    out, var = ctx.adaptive_image(return_variance=True)
    _same(out, r_out, "resolved image")
    _same(var, r_var, "resolved variance")
    prm = N.DenoiseVarParams.default()
    f_out, f_var = P.denoise_variance(r_out, 1.0, r_var, ctx.gbuffer(), prm, return_variance=True)
    g_out, g_var = ctx.adaptive_image(prm, return_variance=True)
    _same(g_out, f_out, "filtered image")
    _same(g_var, f_var, "filtered variance")
    ctx.free()


def test_variance_tracking_and_adaptive_sampling_in_turn_on_one_context(gpu_device):
    """The two features exclude each other and share the context's first-hit planes and their valid flag.
    One context that tracks variance, then samples adaptively, then tracks variance again reads, at every
    step, the bits that fresh contexts read which only ever use one of the two: a plane buffer freed or
    allocated with its flag left set would demodulate by stale or unwritten albedo.  (The last phase runs
    a second pass so that its moments can be read too: a variance needs two batches.)"""
    w, h, spp = 72, 40, 4
    scene = _scene(w, h)
    prm = N.DenoiseVarParams.default()

    def passes(ctx, iters, update):
        for it in iters:
            ctx.render_pass(it)
            update()

    def adaptive_reads(ctx):
        passes(ctx, (1, 5), ctx.adaptive_update)
        state = ctx.adaptive_state()
        return state, ctx.adaptive_image(return_variance=True), ctx.adaptive_image(prm, return_variance=True)

    def tail_reads(ctx):
        ctx.track_variance(True)
        passes(ctx, (9,), ctx.variance_update)
        acc = ctx.image()
        passes(ctx, (13,), ctx.variance_update)
        return acc, ctx.variance(float(2 * spp)), ctx.image()

    mix = P.PathTracer(scene, _gui(), spp=spp)
    mix.track_variance(True)
    passes(mix, (1, 5), mix.variance_update)
    mix_var = mix.variance(float(2 * spp))
    mix.track_variance(False)
    mix.reset_image()
    mix.adaptive(True)
    mix_ad = adaptive_reads(mix)
    mix.adaptive(False)
    mix_tail = tail_reads(mix)
    mix.free()

    var_only = P.PathTracer(scene, _gui(), spp=spp)
    var_only.track_variance(True)
    passes(var_only, (1, 5), var_only.variance_update)
    _same(mix_var, var_only.variance(float(2 * spp)), "variance before adaptive sampling")
    var_only.free()

    ad_only = P.PathTracer(scene, _gui(), spp=spp)
    ad_only.adaptive(True)
    state, resolved, filtered = adaptive_reads(ad_only)
    ad_only.free()
    for k in ("m1", "m2", "prev", "nb", "act", "hot"):
        _same(mix_ad[0][k], state[k], ("adaptive state", k))
    for got, want, what in zip(mix_ad[1] + mix_ad[2], resolved + filtered,
                               ("resolved image", "resolved variance", "filtered image", "filtered variance")):
        _same(got, want, what)

    tail = P.PathTracer(scene, _gui(), spp=spp)
    passes(tail, (1, 5), lambda: None)
    want_tail = tail_reads(tail)
    tail.free()
    for got, want, what in zip(mix_tail, want_tail, ("accumulator after one more pass", "variance after adaptive sampling",
                                                     "final accumulator")):
        _same(got, want, what)


# ---- end to end ---------------------------------------------------------------------------------------------
def test_first_selection_on_the_scene_the_oracle_chose(gpu_device):
    """E2E (tests/test_adaptive_cpu.py) was chosen so that the first selection turns some blocks off and
    keeps some on; the counts are the ones the CPU oracle and the restatement gave."""
    w, h = E2E["res"]
    ctx = P.PathTracer(_scene(w, h), _gui(), spp=E2E["spp"])
    ctx.adaptive(True)
    for b in range(E2E["batches"]):
        ctx.render_pass(1 + b * E2E["spp"])
        ctx.adaptive_update(demodulate=False)
    sel = ctx.adaptive_select(_prm(E2E["threshold"], E2E["floor"], E2E["min_batches"], E2E["dilate"]))
    act = ctx.adaptive_state()["act"]
    assert (act == 0).any() and (act == 1).any()
    assert sel == {"active_blocks": E2E["active"], "blocks": E2E["blocks"]} and int(act.sum()) == E2E["active"]
    ctx.free()


def test_render_adaptive_traces_fewer_segments_and_resolves_per_block(gpu_device, tmp_path):
    import json
    iters = 12
    prm = _prm(0.5, 0.01, 4, 0)
    gui = _gui()
    spec = json.loads((SCENES / "cornell.json").read_text())
    spec["Camera"]["RES"] = [160, 120]                       # (about 260 of its 300 blocks see light in 4 samples)
    scene_path = tmp_path / "cornell_small.json"
    scene_path.write_text(json.dumps(spec))
    img, path, rep = P.render(str(scene_path), iterations=iters, out_dir=str(tmp_path), gui=gui, adaptive=prm,
                              adaptive_every=4)
    assert path.endswith(f".{iters}samp.adaptive.png") and Path(path).exists()
    scene = P.Scene(str(scene_path))
    uni = P.PathTracer(scene, gui)
    for it in range(1, iters + 1):
        uni.render_pass(it)
    seg_uniform = uni.stats()["segments"]
    uni.free()
    h, w = img.shape[:2]
    spb = rep["samples_per_block"]
    print(f"segments adaptive {rep['segments']} uniform {seg_uniform}; active after each selection {rep['active_blocks']} "
          f"of {spb.size}; samples per block min {spb.min()} mean {spb.mean():.2f} max {spb.max()}")
    assert rep["passes"] == iters and len(rep["active_blocks"]) == 2
    assert 0 < rep["active_blocks"][0] < spb.size
    assert rep["segments"] < seg_uniform
    assert spb.min() >= 4 and spb.max() == iters and spb.min() < iters
    n = A.expand(spb, h, w).astype(F)
    with np.errstate(all="ignore"):
        want = np.where((n != 0)[..., None], img / n[..., None], F(0)).astype(F)
    _same(rep["resolved"], want, "resolved image")


# RMSE(adaptive) / RMSE(uniform 64 spp), Cornell 200 x 200, the default parameters, as
# scripts/adaptive_tune.py measured it on an MI355X (profiles/adaptive_tune.jsonl): 0.9663,
# with 8,213,028 segments against uniform's 7,729,404 (its 17th batch took it 6.3% past the budget).
MEASURED_RAW_RATIO = 0.9663


def test_rmse_ratio_against_uniform_at_equal_segments(gpu_device):
    import adaptive_tune as T
    scene = T.cornell()
    uni = T.uniform(scene)
    row = T.ratios(scene, uni, N.AdaptiveParams.default())
    print("adaptive against uniform 64 spp at equal segments:", row)
    assert row["segments"] >= row["budget"] or row["active"][-1] == 0
    assert row["raw_ratio"] <= 1.5 * MEASURED_RAW_RATIO
