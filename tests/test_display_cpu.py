"""The display transform's definition without a GPU: the library's tables against the numpy
restatement (tests/display_ref.py), the defaults against pt_tonemap, properties of the restatement's curves, resolve
and adaptation, the argument checks of pt_display_create (no device needed), and the preview's new settings."""
import math

import numpy as np
import pytest

from tests import display_cases as K
from tests import display_ref as R

F = np.float32


def _ulps(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


@pytest.fixture(scope="module")
def lib_tables():
    from cuda_pathtracer_amd import display_tables
    return display_tables()


@pytest.fixture(scope="module")
def ref_tables():
    return R.tables()


# ---- tables --------------------------------------------------------------------------------------------
def test_library_tables_against_the_restatement(lib_tables, ref_tables):
    assert lib_tables["srgb"][0] == 0.0
    assert _ulps(lib_tables["srgb"][1:], ref_tables["srgb"][1:]).max() <= 1   # (pow may differ between libms)
    assert _ulps(lib_tables["pow2"], ref_tables["pow2"]).max() <= 1
    assert lib_tables["pow2"][0] == 1.0
    assert lib_tables["hable_white"].tobytes() == ref_tables["hable_white"].tobytes()


@pytest.mark.parametrize("which", ["library", "restatement"])
def test_srgb_table_is_the_correctly_rounded_byte(lib_tables, ref_tables, which):
    srgb = (lib_tables if which == "library" else ref_tables)["srgb"]
    assert (np.diff(srgb[1:]) > 0).all()
    rng = np.random.default_rng(11)
    x = np.concatenate([rng.uniform(0, 1, 150000), np.exp2(rng.uniform(-14, 0, 50000)), [0.0, 1.0]]).astype(np.float32)
    x = np.concatenate([x, srgb[1:], np.nextafter(srgb[1:], F(0))])
    want = np.floor(255.0 * R.srgb_oetf(x.astype(np.float64)) + 0.5).astype(np.uint8)
    assert np.array_equal(R.to_bytes(x, R.SRGB, srgb), want)


# ---- the defaults are pt_tonemap -----------------------------------------------------------------------
@pytest.mark.parametrize("case", ["noisy", "noisy-large", "edge"])
def test_defaults_reproduce_tonemap(ref_tables, case):
    from cuda_pathtracer_amd import tonemap
    acc = {"noisy": lambda: K.noisy(65, 3, lo=-10, hi=2), "noisy-large": lambda: K.noisy(257, 5), "edge": K.edge_image}[case]()
    for samples in (1.0, 3.0):
        got = R.apply(acc, samples, R.Params(mirror_x=1), ref_tables)
        assert np.array_equal(got, tonemap(acc, samples))


def test_library_defaults():
    from cuda_pathtracer_amd import DisplayParams
    p, r = DisplayParams.default(), R.Params()
    for name in ("exposure_mode", "exposure", "compensation_ev", "min_ev", "max_ev", "pct_lo", "pct_hi", "rate", "curve", "white",
                 "transfer", "mirror_x"):
        assert getattr(p, name) == getattr(r, name), name
    assert F(p.key_value) == F(r.key_value)
    assert list(p.reserved) == [0, 0, 0]


# ---- properties of the restatement ---------------------------------------------------------------------
@pytest.mark.parametrize("curve", [R.NONE, R.REINHARD, R.ACES, R.HABLE])
def test_curves_map_zero_to_zero_and_do_not_decrease(ref_tables, curve):
    rng = np.random.default_rng(curve)
    x = np.sort(np.concatenate([[0.0, 65504.0], rng.uniform(0, 65504, 20000), np.exp2(rng.uniform(-20, 16, 20000))]))
    x = x.astype(np.float32).reshape(1, -1, 1).repeat(3, axis=2)
    prm = R.Params(curve=curve)
    c = R.curve_values(x, 1.0, 1.0, prm, ref_tables["hable_white"])[0, :, 0]
    assert (c >= 0).all() and (c <= 1).all()
    if curve == R.HABLE:
        # f(0) = D E / (D F) - E / F is three float32 roundings away from 0: 1.03e-8 in the definition's arithmetic,
        # far below one byte step of either transfer (linear 1 / 255, sRGB T[1] = 1.5e-4), so the byte of 0 is 0
        assert 0.0 <= c[0] < 2.0 ** -24
    else:
        assert c[0] == 0.0
    # float32 rounding may make neighbours swap by an ulp of the curve's value; the bytes must not decrease
    for transfer in (R.LINEAR, R.SRGB):
        b = R.to_bytes(c, transfer, ref_tables["srgb"]).astype(np.int32)
        assert b[0] == 0 and (np.diff(b) >= 0).all()


def test_window_is_never_empty():
    for lo, hi in [(102, 922), (0, 1024), (0, 1), (1023, 1024), (511, 512), (300, 301)]:
        for n in range(1, 2001):
            a, b, m = R.window(n, lo, hi)
            assert m >= 1 and 0 <= a < b <= n, (lo, hi, n)


def test_one_bin_gives_its_centre():
    for k in (0, 1, 107, 128, 255):
        for n in (1, 7, 350000):
            h = np.zeros(257, np.int64)
            h[k] = n
            h[256] = 5
            for lo, hi in [(102, 922), (0, 1024), (511, 512)]:
                assert R.level(h, lo, hi) == 32 * k + 16 - 4096


def test_histogram_bins():
    px = np.array([[0.18] * 3, [1.0] * 3, [2.0 ** 16] * 3, [1e30] * 3, [2.0 ** -16] * 3], np.float32).reshape(1, -1, 3)
    h = R.histogram(px, 1.0)
    assert h[107] == 1 and h[128] == 1 and h[255] == 2 and h.sum() == 5
    assert h[0] + h[256] == 1   # (2^-16 in all channels: the luminance's rounding decides its side of the edge)
    e = R.histogram(K.edge_row().reshape(1, -1, 3), 1.0)
    assert e.sum() == 56 and e[256] >= 12   # zeros, the denormal, NaN, infinities and the negative luminances
    assert R.histogram(K.black(5, 2), 1.0)[256] == 10


@pytest.mark.parametrize("rate", [1, 2, 32, 100, 255, 256])
def test_adaptation_reaches_the_target_and_stops(rate):
    for start, t in [(0, 2048), (2048, -2048), (5, 6), (-1000, -1000), (0, 1)]:
        state = (start, 1)
        seen = []
        for _ in range(5000):
            nxt = R.step(state, t, rate)
            assert abs(t - nxt[0]) <= abs(t - state[0])   # never away, never beyond
            assert (nxt[0] == state[0]) == (state[0] == t)
            state = nxt
            seen.append(state[0])
            if state[0] == t:
                break
        assert state == (t, 1), (rate, start, t)
        assert R.step(state, t, rate) == state
    assert R.step((123, 0), 77, rate) == (77, 1)      # the first metering jumps
    assert R.step((123, 1), None, rate) == (123, 1)   # nothing counted: nothing changes
    assert R.step((0, 0), None, rate) == (0, 0)


def test_scale_invariance(ref_tables):
    base = K.stepped(65, 3)
    prm = R.Params(exposure_mode=R.AUTO, curve=R.ACES, transfer=R.SRGB, min_ev=-20.0, max_ev=20.0)
    want, e0 = None, None
    for j in range(-6, 7):
        acc = base * F(2.0 ** j)
        h, (e, has) = R.meter(acc, 2.0, prm)
        assert has == 1 and h[256] == 0 and h[255] == 0
        got = R.apply(acc, 2.0, prm, ref_tables, R.multiplier(e, ref_tables["pow2"]))
        if want is None:
            want, e0 = got, e + 256 * j
        assert e + 256 * j == e0
        assert np.array_equal(got, want), j


def test_multiplier():
    pow2 = R.tables()["pow2"]
    assert R.multiplier(0, pow2) == 1.0 and R.multiplier(256, pow2) == 2.0 and R.multiplier(-512, pow2) == 0.25
    assert R.multiplier(-1, pow2) == F(pow2[255] * F(0.5))
    assert math.isclose(float(R.multiplier(128, pow2)), math.sqrt(2.0), rel_tol=1e-7)


# ---- pt_display_create's argument checks need no device ------------------------------------------------
def _create(w, h, **kw):
    from cuda_pathtracer_amd import DisplayParams, DisplayTransform
    p = DisplayParams.default()
    for k, v in kw.items():
        setattr(p, k, v)
    return DisplayTransform(w, h, p)


@pytest.mark.parametrize("kw", [
    {"exposure": 0.0}, {"exposure": -1.0}, {"exposure": float("nan")}, {"exposure": float("inf")},
    {"pct_lo": 500, "pct_hi": 500}, {"pct_lo": 600, "pct_hi": 500}, {"pct_lo": -1}, {"pct_hi": 1025},
    {"rate": 0}, {"rate": 257}, {"rate": -3},
    {"exposure_mode": 2}, {"exposure_mode": -1}, {"curve": 4}, {"curve": -1}, {"transfer": 2}, {"transfer": -1},
    {"key_value": 0.0}, {"key_value": float("nan")}, {"white": 0.0}, {"min_ev": 3.0, "max_ev": 2.0}, {"max_ev": float("inf")},
    {"compensation_ev": float("nan")},
])
def test_create_refuses_bad_parameters(kw):
    from cuda_pathtracer_amd import PtError
    with pytest.raises(PtError) as ei:
        _create(16, 16, **kw)
    assert ei.value.code == 1   # PT_ERR_ARG


@pytest.mark.parametrize("w,h", [(0, 4), (4, 0), (-1, 4), (4, -7), (65536, 65536)])
def test_create_refuses_bad_sizes(w, h):
    from cuda_pathtracer_amd import PtError
    with pytest.raises(PtError) as ei:
        _create(w, h)
    assert ei.value.code == 1


def test_create_refuses_reserved_words_and_accepts_the_rest():
    from cuda_pathtracer_amd import DisplayParams, DisplayTransform, PtError
    p = DisplayParams.default()
    p.reserved[1] = 1
    with pytest.raises(PtError):
        DisplayTransform(8, 8, p)
    d = _create(8, 8, exposure_mode=1, curve=3, transfer=1, rate=1, pct_lo=0, pct_hi=1024, mirror_x=1)
    d.free()


def test_info_before_any_use_needs_no_device():
    d = _create(8, 8, exposure_mode=1)
    i = d.info()
    assert i["e"] == 0 and i["mult"] == 1.0 and i["metered"] == 0 and not i["hist"].any()
    d.reset()
    d.free()
    m = _create(8, 8, exposure=0.37)
    assert F(m.info()["mult"]) == F(0.37)
    m.free()


# ---- the preview's settings ----------------------------------------------------------------------------
class FakeCtx:
    def __init__(self, log):
        self.log = log

    def set_flags(self, gui):
        pass

    def render_pass(self, it):
        self.log.append(("pass", it))

    def image(self):
        return np.full((32, 48, 3), 0.5, np.float32)

    def free(self):
        self.log.append(("free",))


def _session(tmp_path):
    import cuda_pathtracer_amd as P
    from cuda_pathtracer_amd import preview as V
    from tests.conftest import SCENES
    s = P.Scene(str(SCENES / "cornell.json"))
    s.set_camera((48, 32), 45.0, (0, 5, 10.5), (0, 5, 0), (0, 1, 0))
    st = s.state()
    s.set_render(5, st.traceDepth, st.imageName)
    s.finalize()
    log = []

    def read(ctx, it):
        log.append(("read", it))
        return np.zeros((32, 48, 4), np.uint8)

    return V.PreviewSession(s, out_dir=str(tmp_path), tracer_factory=lambda sc, g: FakeCtx(log), read_preview=read), log


def test_preview_settings(tmp_path):
    ses, log = _session(tmp_path)
    assert {k: ses.state()["settings"][k] for k in ("tonemap", "exposure_ev", "auto_exposure", "srgb")} == \
        {"tonemap": "none", "exposure_ev": 0.0, "auto_exposure": False, "srgb": False}
    ses.run_cuda()
    assert ses.iteration == 1 and not ses.visual_changed and not ses.camchanged
    for name, good, bad in [("tonemap", "aces", "filmic"), ("exposure_ev", -2.5, "bright"), ("auto_exposure", True, None),
                            ("srgb", True, None), ("tonemap", "hable", 3), ("tonemap", "reinhard", None),
                            ("exposure_ev", 16, 16.5), ("exposure_ev", -16.0, float("nan")), ("exposure_ev", 1.0, True)]:
        ses.handle_event({"kind": "setting", "name": name, "value": good})
        assert ses.visual_changed is False and ses.camchanged is False, name
        assert ses.state()["settings"][name] == good
        for b in ([bad] if bad is not None else []) + ([None] if name in ("tonemap", "exposure_ev") else []):
            with pytest.raises(ValueError):
                ses.set_setting(name, b)
            assert ses.state()["settings"][name] == good
    ses.run_cuda()
    assert ses.iteration == 2   # (display only: the accumulation goes on)
    p = ses._display_params()
    assert (p.curve, p.transfer, p.exposure_mode, p.rate, p.compensation_ev, p.mirror_x) == (R.REINHARD, R.SRGB, R.AUTO, 32, 1.0, 0)
    ses.set_setting("auto_exposure", False)
    assert ses._display_params().exposure == 2.0 and ses._display_params().exposure_mode == R.MANUAL
    ses.close()


def test_preview_defaults_take_the_old_paths(tmp_path):
    ses, log = _session(tmp_path)
    assert not ses._display_on()
    ses.run_cuda()
    assert ("read", 1) in log and ses._display is None
    for name, value in [("tonemap", "none"), ("exposure_ev", 0.0), ("auto_exposure", False), ("srgb", False)]:
        ses.set_setting(name, value)
    assert not ses._display_on()
    ses.set_setting("srgb", True)
    assert ses._display_on()
    ses.close()
