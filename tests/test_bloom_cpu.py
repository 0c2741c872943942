"""The bloom's definition without a GPU: every refusal of pt_bloom_create (no device needed), the
level sizes, properties of the numpy restatement (tests/bloom_ref.py: a constant image, flip symmetry, the edge
values), the restatement against the same definition in float64 built from dense matrices, and the preview's new
settings."""
import numpy as np
import pytest

from tests import bloom_cases as K
from tests import bloom_ref as R

F = np.float32


@pytest.fixture(autouse=True)
def _defaults_are_the_products():
    """The restatement's defaults are the product's: every test of this file stands on both."""
    from cuda_pathtracer_amd import BloomParams
    p, d = BloomParams.default(), R.Params()
    assert (p.threshold, p.strength, p.spread, p.clamp, p.levels) == (d.threshold, d.strength, d.spread, d.clamp, d.levels)


def _params(**kw):
    from cuda_pathtracer_amd import BloomParams
    p = BloomParams.default()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


# ---- the interface -------------------------------------------------------------------------------------
def test_abi_and_exports():
    import cuda_pathtracer_amd as P
    from cuda_pathtracer_amd import _native as N
    for name in ("pt_bloom_params_default", "pt_bloom_create", "pt_bloom_destroy", "pt_bloom_apply", "pt_bloom_host",
                 "pt_bloom_info", "pt_preview_bloom"):
        assert name in N.SIGNATURES and hasattr(P.lib(), name)
    for name in ("BloomParams", "Bloom", "bloom"):
        assert name in P.__all__ and hasattr(P, name)
    assert hasattr(P.PathTracer, "preview_bloom")


def test_defaults():
    p = _params()
    assert (p.threshold, p.strength, p.spread, p.clamp, p.levels, list(p.reserved)) == (1.0, 0.25, 0.75, 65504.0, 0, [0, 0, 0])
    d = R.Params()
    assert (d.threshold, d.strength, d.spread, d.clamp, d.levels) == (1.0, 0.25, 0.75, 65504.0, 0)


NAN, INF = float("nan"), float("inf")
REFUSED = [dict(threshold=NAN), dict(threshold=INF), dict(threshold=-1.0), dict(threshold=-1e-30),
           dict(strength=NAN), dict(strength=INF), dict(strength=-0.5),
           dict(spread=0.0), dict(spread=-0.5), dict(spread=1.0000001), dict(spread=NAN), dict(spread=INF),
           dict(clamp=0.0), dict(clamp=-1.0), dict(clamp=65505.0), dict(clamp=INF), dict(clamp=NAN),
           dict(levels=-1), dict(levels=13), dict(levels=1 << 20)]


@pytest.mark.parametrize("kw", REFUSED, ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_create_refuses_parameters(kw):
    from cuda_pathtracer_amd import Bloom, PtError
    with pytest.raises(PtError) as ei:
        Bloom(8, 8, _params(**kw))
    assert ei.value.code == 1


def test_create_refuses_reserved_sizes_and_nulls():
    import ctypes as C
    from cuda_pathtracer_amd import Bloom, PtError, lib
    for k in range(3):
        p = _params()
        p.reserved[k] = 1
        with pytest.raises(PtError) as ei:
            Bloom(8, 8, p)
        assert ei.value.code == 1
    for w, h in [(0, 8), (8, 0), (-1, 8), (8, -3), (65536, 32768), (1 << 30, 2)]:
        with pytest.raises(PtError) as ei:
            Bloom(w, h)
        assert ei.value.code == 1, (w, h)
    h, p = C.c_void_p(), _params()
    assert lib().pt_bloom_create(8, 8, None, C.byref(h)) == 1
    assert lib().pt_bloom_create(8, 8, C.byref(p), None) == 1
    assert lib().pt_bloom_info(None, None, None, None) == 1
    assert lib().pt_bloom_destroy(None) == 0


def test_create_accepts_the_ends_of_the_ranges():
    from cuda_pathtracer_amd import Bloom
    for kw in [dict(threshold=0.0), dict(strength=0.0), dict(spread=1.0), dict(spread=1e-30), dict(clamp=65504.0), dict(clamp=1e-30),
               dict(levels=1), dict(levels=12)]:
        Bloom(8, 8, _params(**kw)).free()
    Bloom(46340, 46340).free()   # (below 2^31 pixels; nothing is allocated before the first use)


@pytest.mark.parametrize("w,h", K.SIZES + [(3840, 2160), (800, 800), (1, 4096)])
@pytest.mark.parametrize("levels", [0, 1, 2, 12])
def test_level_sizes(w, h, levels):
    from cuda_pathtracer_amd import Bloom
    b = Bloom(w, h, _params(levels=levels))
    try:
        i = b.info()
    finally:
        b.free()
    k = R.levels_of(w, h, levels)
    assert i["levels"] == k and list(zip(i["widths"], i["heights"])) == R.sizes(w, h, k)[1:]


def test_default_levels():
    assert [R.levels_of(*s) for s in [(1, 1), (2, 1), (3, 2), (5, 7), (65, 33), (130, 67), (3840, 2160)]] == [1, 1, 1, 2, 5, 6, 6]


# ---- the restatement's properties ----------------------------------------------------------------------
def test_gain_by_hand():
    """strength / (1 + spread + .. + spread^(K-1)), worked out by hand (apply64 shares gain() with the float32 form)."""
    assert R.gain(R.Params(strength=1.0, spread=0.5), 3) == F(1 / 1.75)
    assert R.gain(R.Params(strength=1.0, spread=1.0), 4) == F(0.25)
    assert R.gain(R.Params(strength=0.25, spread=0.75), 1) == F(0.25)
    assert R.gain(R.Params(strength=3.0, spread=0.25), 2) == F(2.4)
    assert R.gain(R.Params(), 6) == F(0.25 / (1 + 0.75 + 0.5625 + 0.421875 + 0.31640625 + 0.2373046875))


def test_constant_image():
    """threshold 0, strength 1, spread 1: w is exactly 1, every filter sums to one, the K levels add up to K c and the
    gain is 1 / K: the output is exactly 2 c."""
    acc = K.constant(37, 53)
    for levels in (4, 0, 1):
        out = R.apply(acc, 1.0, R.Params(threshold=0.0, strength=1.0, spread=1.0, levels=levels))
        assert np.array_equal(out, F(2) * acc), levels
    out = R.apply(acc * F(4), 4.0, R.Params(threshold=0.0, strength=1.0, spread=1.0, levels=4))
    assert np.array_equal(out, F(8) * acc)


@pytest.mark.parametrize("w,h,levels", [(64, 32, 5), (96, 80, 4), (16, 16, 0)])
def test_flip_symmetry(w, h, levels):
    """Bit for bit where the sizes are multiples of 2^K: the expressions are symmetric under tap reversal.  (At odd
    sizes the clamping is at the far edge only, and the flipped image's output is not the flipped output.)"""
    acc = K.noisy(w, h)
    prm = R.Params(threshold=0.7, levels=levels)
    assert w % (1 << R.levels_of(w, h, levels)) == 0 and h % (1 << R.levels_of(w, h, levels)) == 0
    out = R.apply(acc, 2.0, prm)
    assert np.array_equal(R.apply(acc[:, ::-1], 2.0, prm), out[:, ::-1])
    assert np.array_equal(R.apply(acc[::-1], 2.0, prm), out[::-1])


@pytest.mark.parametrize("samples", [1.0, 3.0])
def test_edge_values(samples):
    acc = K.edge_image()
    for prm in (R.Params(), R.Params(threshold=0.0, strength=1.0, spread=1.0), R.Params(clamp=2.0, levels=12)):
        g = R.glare(acc, samples, prm)
        assert np.isfinite(g).all() and (g >= 0).all() and not np.signbit(g).any()
        assert g.max() > 0
        out = R.apply(acc, samples, prm)
        nan, inf = np.isnan(acc), np.isinf(acc)
        assert np.array_equal(np.isnan(out), nan) and np.array_equal(out[inf], acc[inf])
        fin = ~nan & ~inf
        assert (out[fin] >= acc[fin]).all()
        neg_zero = (acc == 0) & np.signbit(acc)
        assert neg_zero.any() and not np.signbit(out[neg_zero]).any()


def test_threshold_zero_passes_everything_positive():
    acc = K.edge_image()
    b = R.bright(acc, 1.0, R.Params(threshold=0.0))
    c = R.clamped(acc, 1.0, R.Params())
    lit = R.luminance(c) > 0
    assert np.array_equal(b[lit], c[lit]) and (b[~lit] == 0).all()


# ---- against float64 -----------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,levels", K.SIZES_64)
def test_restatement_against_float64(w, h, levels):
    """Every operand is non-negative, so rounding errors only add up: the relative error is at most the number of
    roundings on the longest chain times 2^-24.  Bright pass 6 (the division by samples, three roundings of L with
    its products, L - threshold and its division, the product c w: counted as 6), 9 per down level (a + d, b + c, the
    product by 3 and the sum, twice, and the product by 1/64, exact but counted), 8 per up level (the product by 3,
    the sum and the product by 0.25, twice; the product by spread and the sum with B_k), 3 for the composition (the
    gain, the samples, the sum with v): 9 + 17 K."""
    k = R.levels_of(w, h, levels)
    worst = 0.0
    for seed, (t, s, sp) in enumerate([(1.0, 0.25, 0.75), (0.0, 1.0, 1.0), (0.3, 2.0, 0.5)]):
        for samples in (1.0, 3.0):
            acc = K.noisy(w, h, seed)
            prm = R.Params(threshold=t, strength=s, spread=sp, levels=levels)
            got, want = R.apply(acc, samples, prm).astype(np.float64), R.apply64(acc, samples, prm)
            assert (want > 0).all()
            worst = max(worst, float((np.abs(got - want) / want).max()))
    print(f"bloom float32 against float64 at {w} x {h}, K = {k}: largest relative difference {worst:.3g}, "
          f"bound {(9 + 17 * k) * 2.0 ** -24:.3g}")
    assert worst <= (9 + 17 * k) * 2.0 ** -24


# ---- the preview's settings ----------------------------------------------------------------------------
class _Ctx:
    def set_flags(self, gui):
        pass

    def render_pass(self, it):
        pass

    def free(self):
        pass


def test_preview_settings(tmp_path):
    import cuda_pathtracer_amd as P
    from cuda_pathtracer_amd import preview as V
    from tests.conftest import SCENES
    s = P.Scene(str(SCENES / "cornell.json"))
    s.set_camera((48, 32), 45.0, (0, 5, 10.5), (0, 5, 0), (0, 1, 0))
    s.finalize()
    ses = V.PreviewSession(s, out_dir=str(tmp_path), tracer_factory=lambda sc, g: _Ctx(),
                           read_preview=lambda ctx, it: np.zeros((32, 48, 4), np.uint8))
    assert {k: ses.state()["settings"][k] for k in ("bloom", "bloom_threshold")} == {"bloom": 0.0, "bloom_threshold": 1.0}
    assert not ses._display_on() and ses._bloom_obj() is None
    ses.run_cuda()
    for name, good, bads in [("bloom", 0.5, [-0.1, 4.5, "on", None, True, float("nan")]),
                             ("bloom_threshold", 0.0, [-1.0, float("inf"), "x", None]), ("bloom_threshold", 2.5, [])]:
        ses.handle_event({"kind": "setting", "name": name, "value": good})
        assert ses.visual_changed is False and ses.camchanged is False
        for bad in bads:
            with pytest.raises(ValueError):
                ses.set_setting(name, bad)
        assert ses.state()["settings"][name] == good
    ses.run_cuda()
    assert ses.iteration == 2   # (display only: the accumulation goes on)
    p = ses._bloom_params()
    assert (p.strength, p.threshold, p.spread, p.levels) == (0.5, 2.5, 0.75, 0) and ses._display_on()
    assert "bloom_threshold" in V._PAGE
    ses.set_setting("bloom", 0)
    assert not ses._display_on()
    ses.close()
