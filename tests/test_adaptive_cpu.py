"""Adaptive sampling, the parts that need no GPU: the C ABI's symbols, struct size,
defaults and argument checks (which return before any device call: on a machine without a GPU a device
call would fail with another code), the block geometry of the numpy restatement the GPU tests compare
against (tests/adaptive_ref.py) checked with per-pixel loops, and the choice of the end-to-end scene of
tests/test_adaptive_gpu.py, made with the CPU oracle and recorded in E2E below.

(`batch_samples` changed between two updates needs a first update that succeeds, which needs a device, so
that check is in tests/test_adaptive_gpu.py, as pt_moments' is in tests/test_denoise_var_gpu.py.)"""
import ctypes as C
import math
import sys
from pathlib import Path

import numpy as np
import pytest

import cuda_pathtracer_amd as P
from cuda_pathtracer_amd import _native as N

sys.path.insert(0, str(Path(__file__).resolve().parent))
import adaptive_ref as A  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
SCENES = ROOT / "tests" / "scenes"
F = np.float32
PT_ERR_ARG = 1

NEW_SYMBOLS = ("pt_adaptive_params_default", "pt_adaptive_obj_create", "pt_adaptive_obj_destroy", "pt_adaptive_obj_info",
               "pt_adaptive_obj_reset", "pt_adaptive_obj_update", "pt_adaptive_obj_select", "pt_adaptive_obj_set_mask",
               "pt_adaptive_obj_apply", "pt_adaptive_obj_resolve", "pt_adaptive_obj_get", "pt_adaptive_enable",
               "pt_adaptive_update", "pt_adaptive_select", "pt_adaptive_set_mask", "pt_adaptive_info", "pt_adaptive_get",
               "pt_adaptive_image")

# The end-to-end scene of tests/test_adaptive_gpu.py, chosen here with the CPU oracle (whose passes the
# GPU's equal bit for bit) and the restatement: Cornell at 64 x 48, rng_key_pixel, 8 batches of 4 samples,
# no demodulation.  At that count a pixel's e is 0 (no path of it reached the light yet) or about 0.94
# (one batch did), so any threshold in between separates the blocks that saw light from the 4 that did
# not: 44 of the 48 blocks stay active.
E2E = dict(res=(64, 48), spp=4, batches=8, threshold=0.5, floor=0.01, min_batches=4, dilate=0, active=44, blocks=48)


def test_new_symbols_and_struct_size():
    L = P.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert name in N.SIGNATURES
    assert C.sizeof(N.AdaptiveParams) == 32
    assert "AdaptiveParams" in P.__all__ and P.AdaptiveParams is N.AdaptiveParams
    for name in ("adaptive", "adaptive_update", "adaptive_select", "adaptive_set_mask", "adaptive_state", "adaptive_image"):
        assert callable(getattr(P.PathTracer, name))


def test_defaults_are_as_documented():
    raw = (C.c_uint8 * 32)(*([0xAB] * 32))
    p = N.AdaptiveParams.from_buffer(raw)
    P.lib().pt_adaptive_params_default(C.byref(p))
    assert list(p.reserved) == [0, 0, 0, 0]
    assert (p.threshold, p.floor, p.min_batches, p.dilate) == (F(0.4), F(0.1), 4, 0)   # DESIGN.md §13's grid
    assert bytes(N.AdaptiveParams.default()) == bytes(p)
    P.lib().pt_adaptive_params_default(None)


def _prm(**kw):
    p = N.AdaptiveParams.default()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


BAD_PARAMS = [dict(threshold=-0.5), dict(threshold=math.nan), dict(threshold=math.inf), dict(threshold=-math.inf),
              dict(floor=0.0), dict(floor=-1.0), dict(floor=math.nan), dict(floor=math.inf), dict(min_batches=1),
              dict(min_batches=0), dict(min_batches=-3), dict(dilate=3), dict(dilate=-1)]


@pytest.fixture()
def obj():
    h = C.c_void_p()
    assert P.lib().pt_adaptive_obj_create(130, 67, C.byref(h)) == 0 and h.value
    yield h
    assert P.lib().pt_adaptive_obj_destroy(h) == 0


@pytest.mark.parametrize("kw", BAD_PARAMS, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_select_parameter_errors_need_no_device(obj, kw):
    L = P.lib()
    assert L.pt_adaptive_obj_select(obj, C.byref(_prm(**kw)), None, None, None) == PT_ERR_ARG
    assert L.pt_last_error()


def test_object_argument_errors_need_no_device(obj):
    L = P.lib()
    one, two = C.c_void_p(16), C.c_void_p(64)   # (never dereferenced: the checks come first)
    h = C.c_void_p()
    for w, hh in ((0, 4), (4, 0), (-1, 4), (1 << 16, 1 << 15)):
        assert L.pt_adaptive_obj_create(w, hh, C.byref(h)) == PT_ERR_ARG, (w, hh)
    assert L.pt_adaptive_obj_create(4, 4, None) == PT_ERR_ARG
    nblk, n, bs = C.c_int32(-1), C.c_int32(-1), C.c_float(-1)
    assert L.pt_adaptive_obj_info(obj, C.byref(nblk), C.byref(n), C.byref(bs)) == 0
    assert (nblk.value, n.value, bs.value) == ((130 * 67 + 63) // 64, 0, 0.0)
    for bad in (0.0, -1.0, math.nan, math.inf):
        assert L.pt_adaptive_obj_update(obj, one, bad, None, None) == PT_ERR_ARG, bad
    assert L.pt_adaptive_obj_update(obj, None, 1.0, None, None) == PT_ERR_ARG
    assert L.pt_adaptive_obj_select(obj, None, None, None, None) == PT_ERR_ARG
    mask = np.ones(nblk.value + 1, np.uint8)
    for bad_len in (nblk.value - 1, nblk.value + 1, 0, -1):
        assert L.pt_adaptive_obj_set_mask(obj, mask.ctypes.data, bad_len, None) == PT_ERR_ARG, bad_len
        assert b"mask length" in L.pt_last_error()
    assert L.pt_adaptive_obj_set_mask(obj, None, nblk.value, None) == PT_ERR_ARG
    assert L.pt_adaptive_obj_apply(obj, None, two, None) == PT_ERR_ARG
    assert L.pt_adaptive_obj_apply(obj, one, None, None) == PT_ERR_ARG
    assert L.pt_adaptive_obj_resolve(obj, None, two, None, None) == PT_ERR_ARG
    assert L.pt_adaptive_obj_resolve(obj, one, None, None, None) == PT_ERR_ARG          # no output at all
    assert L.pt_adaptive_obj_resolve(obj, one, one, None, None) == PT_ERR_ARG           # aliases
    assert L.pt_adaptive_obj_resolve(obj, one, two, one, None) == PT_ERR_ARG
    assert L.pt_adaptive_obj_resolve(obj, one, two, two, None) == PT_ERR_ARG
    assert L.pt_adaptive_obj_resolve(obj, one, two, None, None) == PT_ERR_ARG           # no update yet
    assert b"update" in L.pt_last_error()
    # null objects and contexts
    prm = N.AdaptiveParams.default()
    assert L.pt_adaptive_obj_destroy(None) == 0
    assert L.pt_adaptive_obj_info(None, None, None, None) == PT_ERR_ARG
    assert L.pt_adaptive_obj_reset(None, None, None) == PT_ERR_ARG
    assert L.pt_adaptive_obj_update(None, one, 1.0, None, None) == PT_ERR_ARG
    assert L.pt_adaptive_obj_select(None, C.byref(prm), None, None, None) == PT_ERR_ARG
    assert L.pt_adaptive_obj_set_mask(None, mask.ctypes.data, 1, None) == PT_ERR_ARG
    assert L.pt_adaptive_obj_apply(None, one, two, None) == PT_ERR_ARG
    assert L.pt_adaptive_obj_resolve(None, one, two, None, None) == PT_ERR_ARG
    assert L.pt_adaptive_obj_get(None, None, None, None, None, None, None) == PT_ERR_ARG
    assert L.pt_adaptive_enable(None, 1) == PT_ERR_ARG
    assert L.pt_adaptive_update(None, 1, None) == PT_ERR_ARG
    assert L.pt_adaptive_select(None, C.byref(prm), None, None) == PT_ERR_ARG
    assert L.pt_adaptive_set_mask(None, mask.ctypes.data, 1) == PT_ERR_ARG
    assert L.pt_adaptive_info(None, None, None, None, None, None) == PT_ERR_ARG
    assert L.pt_adaptive_get(None, None, None, None, None, None, None) == PT_ERR_ARG
    assert L.pt_adaptive_image(None, None, one, None) == PT_ERR_ARG


# ---- the restatement's block geometry against per-pixel loops -------------------------------------------
WIDTHS = [1, 63, 64, 65, 72, 130]


@pytest.mark.parametrize("w", WIDTHS)
def test_block_membership_and_partial_last_block(w):
    for h in (1, 3, 7):
        nblk = A.nblocks(h, w)
        blk = A.block_of(h, w)
        seen = 0
        for b in range(nblk):
            px = A.block_pixels_brute(h, w, b)
            assert len(px) == (64 if b < nblk - 1 else h * w - 64 * (nblk - 1)), (h, w, b)
            assert 1 <= len(px) <= 64
            assert all(blk[y, x] == b for y, x in px)
            flat = [y * w + x for y, x in px]
            assert flat == list(range(64 * b, 64 * b + len(px)))        # consecutive in image order
            seen += len(px)
        assert seen == h * w and blk.max() == nblk - 1
        assert np.array_equal(A.expand(np.arange(nblk), h, w), blk)


@pytest.mark.parametrize("r", [0, 1, 2])
@pytest.mark.parametrize("w", WIDTHS)
def test_dilation_box_equals_the_per_pixel_loop(w, r):
    rng = np.random.default_rng(100 * w + r)
    for h in (1, 2, 5):
        for density in (0.0, 0.02, 0.3, 1.0):
            hot = rng.random((h, w)) < density
            assert np.array_equal(A.dilate_blocks(hot, r), A.dilate_blocks_brute(hot, r)), (h, w, r, density)
    # one hot pixel in a corner, at a block seam and at a row end reaches exactly the loop's blocks
    h = 4
    for i in {0, w - 1, h * w - 1, min(63, h * w - 1), min(64, h * w - 1), (h - 1) * w}:
        hot = np.zeros(h * w, bool)
        hot[i] = True
        hot = hot.reshape(h, w)
        assert np.array_equal(A.dilate_blocks(hot, r), A.dilate_blocks_brute(hot, r)), (w, r, i)


def test_restatement_update_select_resolve_properties():
    h, w = 5, 72
    rng = np.random.default_rng(3)
    a = A.Adaptive(h, w)
    mask = np.array([1, 0, 1, 1, 0, 1], np.uint8)
    acc = np.zeros((h, w, 3), F)
    for b in range(5):
        if b == 2:
            a.set_mask(mask)
        acc = (acc + rng.random((h, w, 3)).astype(F)).astype(F)
        poisoned = acc.copy()
        if b >= 2:
            poisoned[A.expand(mask, h, w) == 0] = np.nan                 # inactive rgb is not used
        a.update(poisoned, 1.0)
    assert a.nb.tolist() == [5, 2, 5, 5, 2, 5]
    assert np.isfinite(a.m1).all() and np.isfinite(a.prev).all()
    out, var = a.resolve(acc)
    nbp = A.expand(a.nb, h, w).astype(F)
    assert np.array_equal(out, (acc / nbp[..., None]).astype(F))
    assert (var >= 0).all()
    # select: blocks below min_batches stay active whatever the threshold; NaN moments are not hot
    a.m1[0, 0] = np.nan
    n = a.select(1e30, 0.01, 4, 0)
    assert a.act.tolist() == [0, 1, 0, 0, 1, 0] and n == 2
    assert a.hot[0, 0] == 0
    assert np.array_equal(a.apply(np.arange(1, 7)), [0, 2, 0, 0, 5, 0])


def test_end_to_end_scene_is_chosen_with_the_oracle():
    """E2E's threshold leaves some blocks active and some not after the first selection, on the CPU oracle's
    passes (which the GPU's equal bit for bit): the GPU end-to-end test cannot pass vacuously."""
    from oracle import binding as O
    o = O.OracleScene.from_json(str(SCENES / "cornell.json"))
    w, h = E2E["res"]
    o.set_camera((w, h), 45.0, (0, 5, 10.5), (0, 5, 0), (0, 1, 0))
    fl = O.flags(rng_key_pixel=True)
    img = np.zeros((h, w, 3), F)
    a = A.Adaptive(h, w)
    for b in range(E2E["batches"]):
        img, _ = O.render_pass(o, fl, 1 + b * E2E["spp"], E2E["spp"], image=img)
        a.update(img.copy(), E2E["spp"])
    e = a.error(E2E["floor"])
    n = a.select(E2E["threshold"], E2E["floor"], E2E["min_batches"], E2E["dilate"])
    print("e2e: active", n, "of", a.act.size, "max e per block", np.sort(np.nanmax(
        np.where(np.isnan(e), -1, e).reshape(-1)[:a.act.size * 64].reshape(-1, 64), axis=1))[[0, 4, -1]])
    assert a.act.size == E2E["blocks"] and n == E2E["active"]
    assert 0 < n < a.act.size
