"""The display transform on the device (csrc/pt_display.hip) against its numpy restatement
(tests/display_ref.py, with the library's tables): every comparison is == on bytes or integers.  Shapes are the
smallest at which each part can go wrong (display_cases.SIZES): widths on both sides of a lane's four pixels and of
a wave, several workgroups, and 700 x 500, which is beyond one sweep of the kernels' grid of 256 workgroups."""
import io
import subprocess
import urllib.request

import numpy as np
import pytest

from tests import display_cases as K
from tests import display_ref as R

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = 256
CURVES = (R.NONE, R.REINHARD, R.ACES, R.HABLE)


@pytest.fixture(scope="module")
def tab():
    from cuda_pathtracer_amd import display_tables
    return display_tables()


def _params(**kw):
    """The library's parameters and the restatement's, from one set of fields."""
    from cuda_pathtracer_amd import DisplayParams
    p = DisplayParams.default()
    for k, v in kw.items():
        setattr(p, k, v)
    return p, R.Params(**kw)


def _display(w, h, **kw):
    from cuda_pathtracer_amd import DisplayTransform
    p, rp = _params(**kw)
    return DisplayTransform(w, h, p), rp


def _check_apply(acc, tab, exposures=(1.0, 0.37), sampless=(1.0, 3.0)):
    """Every curve x both transfers x strides 3 and 4 x mirror on and off, with a guard band around the bytes."""
    import torch
    h, w = acc.shape[:2]
    t_acc = torch.from_numpy(acc).cuda()
    for stride in (3, 4):
        n = w * h * stride
        buf = torch.empty(n + 2 * GUARD, dtype=torch.uint8, device="cuda")
        for samples in sampless:
            for exposure in exposures:
                for curve in CURVES:
                    c = R.curve_values(acc, samples, F(exposure), R.Params(curve=curve), tab["hable_white"])
                    for transfer in (R.LINEAR, R.SRGB):
                        b = R.to_bytes(c, transfer, tab["srgb"])
                        for mirror in (0, 1):
                            d, _ = _display(w, h, exposure=exposure, curve=curve, transfer=transfer, mirror_x=mirror)
                            buf.fill_(0xA5)
                            d.apply(t_acc.data_ptr(), samples, buf.data_ptr() + GUARD, stride)
                            got = buf.cpu().numpy()
                            d.free()
                            what = (w, h, stride, samples, exposure, curve, transfer, mirror)
                            assert (got[:GUARD] == 0xA5).all() and (got[GUARD + n:] == 0xA5).all(), what
                            assert np.array_equal(got[GUARD:GUARD + n].reshape(h, w, stride), R.layout(b, mirror, stride)), what


# ---- applying ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", K.SIZES)
def test_apply(gpu_device, tab, w, h):
    _check_apply(K.noisy(w, h, lo=-14.0, hi=8.0), tab)


def test_apply_edge_rows(gpu_device, tab):
    _check_apply(K.edge_image(), tab)


def test_apply_wide_range(gpu_device, tab):
    _check_apply(K.noisy(257, 5), tab, exposures=(1.0,), sampless=(3.0,))


def test_apply_unaligned_pointers(gpu_device, tab):
    """An accumulator that is not 16-byte aligned and bytes that are not word aligned take the scalar paths."""
    import torch
    w, h = 65, 3
    acc = K.noisy(w, h, lo=-14.0, hi=8.0)
    src = torch.zeros(w * h * 3 + 4, dtype=torch.float32, device="cuda")
    src[1:1 + w * h * 3] = torch.from_numpy(acc).cuda().reshape(-1)
    for stride in (3, 4):
        n = w * h * stride
        buf = torch.empty(n + 2 * GUARD, dtype=torch.uint8, device="cuda")
        for mirror in (0, 1):
            for off in (0, 1):
                d, rp = _display(w, h, curve=R.ACES, transfer=R.SRGB, mirror_x=mirror)
                buf.fill_(0xA5)
                d.apply(src.data_ptr() + 4, 2.0, buf.data_ptr() + GUARD + off, stride)
                got = buf.cpu().numpy()
                d.free()
                assert (got[:GUARD + off] == 0xA5).all() and (got[GUARD + off + n:] == 0xA5).all()
                assert np.array_equal(got[GUARD + off:GUARD + off + n].reshape(h, w, stride), R.apply(acc, 2.0, rp, tab, stride=stride))


@pytest.mark.parametrize("case", ["noisy", "edge"])
def test_defaults_are_tonemap(gpu_device, case):
    from cuda_pathtracer_amd import DisplayParams, DisplayTransform, display_transform, tonemap
    acc = K.noisy(257, 5, lo=-10.0, hi=2.0) if case == "noisy" else K.edge_image()
    p = DisplayParams.default()
    p.mirror_x = 1
    d = DisplayTransform(acc.shape[1], acc.shape[0], p)
    try:
        for samples in (1.0, 3.0):
            assert np.array_equal(d.apply(acc, samples), tonemap(acc, samples))
            assert np.array_equal(display_transform(acc, samples, p), tonemap(acc, samples))
    finally:
        d.free()


def test_arguments(gpu_device):
    import torch
    from cuda_pathtracer_amd import PtError
    d, _ = _display(8, 8)
    acc = torch.zeros((8, 8, 3), dtype=torch.float32, device="cuda")
    out = torch.zeros(8 * 8 * 4, dtype=torch.uint8, device="cuda")
    try:
        for args in [(acc.data_ptr(), 1.0, out.data_ptr(), 5), (acc.data_ptr(), 0.0, out.data_ptr(), 3),
                     (acc.data_ptr(), float("nan"), out.data_ptr(), 3), (acc.data_ptr(), 1.0, acc.data_ptr() + 16, 3)]:
            with pytest.raises(PtError) as ei:
                d.apply(*args)
            assert ei.value.code == 1
        with pytest.raises(PtError):
            d.meter(acc.data_ptr(), -1.0)
    finally:
        d.free()


# ---- metering ------------------------------------------------------------------------------------------
def _meter_check(acc, samples, tab, **kw):
    d, rp = _display(acc.shape[1], acc.shape[0], exposure_mode=R.AUTO, **kw)
    try:
        d.meter(acc, samples)
        i = d.info()
    finally:
        d.free()
    hist, (e, has) = R.meter(acc, samples, rp)
    assert np.array_equal(i["hist"].astype(np.int64), hist)
    assert (i["e"], i["metered"]) == (e, has)
    assert F(i["mult"]).tobytes() == R.multiplier(e, tab["pow2"]).tobytes()
    return i


@pytest.mark.parametrize("w,h", K.SIZES)
def test_meter_histogram(gpu_device, tab, w, h):
    _meter_check(K.noisy(w, h), 3.0, tab)
    _meter_check(K.noisy(w, h, seed=1, lo=-3.0, hi=3.0), 1.0, tab)


def test_meter_edge_rows(gpu_device, tab):
    i = _meter_check(K.edge_image(), 1.0, tab)
    assert i["hist"][256] >= 3 * 12 and i["hist"][255] >= 3


def test_meter_one_colour(gpu_device, tab):
    i = _meter_check(K.one_colour(700, 500), 1.0, tab)
    assert i["hist"].max() == 350000 and i["hist"].sum() == 350000 and i["hist"][256] == 0


def test_meter_black_and_one_pixel(gpu_device, tab):
    i = _meter_check(K.black(65, 3), 1.0, tab)
    assert (i["e"], i["metered"], i["mult"]) == (0, 0, 1.0) and i["hist"][256] == 195
    i = _meter_check(np.array([[[0.3, 0.5, 0.2]]], np.float32), 1.0, tab)
    assert i["metered"] == 1 and i["hist"].sum() == 1


@pytest.mark.parametrize("lo,hi", [(102, 922), (0, 1024), (511, 512)])
@pytest.mark.parametrize("key", [0.18, 0.5])
def test_meter_exposure(gpu_device, tab, lo, hi, key):
    _meter_check(K.noisy(257, 5, lo=-6.0, hi=6.0), 2.0, tab, pct_lo=lo, pct_hi=hi, key_value=key)
    _meter_check(K.noisy(257, 5, lo=-16.0, hi=-12.0), 2.0, tab, pct_lo=lo, pct_hi=hi, key_value=key, compensation_ev=0.5)   # max_ev


def test_adaptation(gpu_device, tab):
    """Six frames at rate 32, the brightness stepping by 2^3 after the third; then a reset."""
    base = K.stepped(65, 3)
    d, rp = _display(65, 3, exposure_mode=R.AUTO, rate=32, curve=R.REINHARD, transfer=R.SRGB)
    state, seen = (0, 0), []
    try:
        for k in range(8):
            acc = base * F(8.0) if 3 <= k < 6 else base
            if k == 6:
                d.reset()
                state = (0, 0)
            _, state = R.meter(acc, 2.0, rp, state)
            got = d.frame(acc, 2.0)
            assert d.info()["e"] == state[0], k
            assert np.array_equal(got, R.apply(acc, 2.0, rp, tab, R.multiplier(state[0], tab["pow2"]))), k
            seen.append(state[0])
    finally:
        d.free()
    assert seen[0] == seen[1] == seen[2]                       # the first metering jumps, the image stays
    assert seen[2] > seen[3] > seen[4] > seen[5] > seen[2] - 768   # on the way down by 3 stops, not there yet
    assert seen[6] == seen[7] == seen[0]                       # the reset makes the next frame jump


def test_scale_invariance(gpu_device, tab):
    base = K.stepped(65, 3)
    want = None
    for j in range(-6, 7):
        d, _ = _display(65, 3, exposure_mode=R.AUTO, curve=R.ACES, transfer=R.SRGB, min_ev=-20.0, max_ev=20.0)
        try:
            got = d.frame(base * F(2.0 ** j), 2.0)
            e = d.info()["e"]
        finally:
            d.free()
        if want is None:
            want, e0 = got, e + 256 * j
        assert e + 256 * j == e0 and np.array_equal(got, want), j


def test_stream_order(gpu_device, tab):
    """meter on one stream, apply on another behind the caller's event: the bytes of one stream."""
    import torch
    acc = K.stepped(257, 5)
    t_acc = torch.from_numpy(acc).cuda()
    outs = []
    for two in (False, True):
        d, rp = _display(257, 5, exposure_mode=R.AUTO, curve=R.HABLE, transfer=R.SRGB)
        out = torch.zeros((5, 257, 3), dtype=torch.uint8, device="cuda")
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        try:
            d.meter(t_acc.data_ptr(), 2.0, stream=s1)
            if two:
                ev = torch.cuda.Event()
                ev.record(s1)
                s2.wait_event(ev)
            d.apply(t_acc.data_ptr(), 2.0, out.data_ptr(), 3, stream=s2 if two else s1)
            (s2 if two else s1).synchronize()
            outs.append(out.cpu().numpy())
        finally:
            d.free()
    _, (e, _) = R.meter(acc, 2.0, rp)
    assert np.array_equal(outs[0], outs[1])
    assert np.array_equal(outs[0], R.apply(acc, 2.0, rp, tab, R.multiplier(e, tab["pow2"])))


# ---- the context path ----------------------------------------------------------------------------------
AUTO_ACES_SRGB = dict(exposure_mode=R.AUTO, curve=R.ACES, transfer=R.SRGB)


def _scene(cornell_path, iterations=4, res=(64, 64)):
    from cuda_pathtracer_amd import Scene
    s = Scene(cornell_path)
    s.set_camera(res, 45.0, (0, 5, 10.5), (0, 5, 0), (0, 1, 0))
    st = s.state()
    s.set_render(iterations, st.traceDepth, st.imageName)
    s.finalize()
    return s


def _auto_bytes(acc, samples, rp, tab, stride=3):
    _, (e, _) = R.meter(acc, samples, rp)
    return R.apply(acc, samples, rp, tab, R.multiplier(e, tab["pow2"]), stride)


def test_context_path(cornell_path, gpu_device, tab):
    import torch
    from PIL import Image
    from cuda_pathtracer_amd import JpegEncoder, PathTracer, PngEncoder, PtError, encode_jpeg, encode_png
    pt = PathTracer(_scene(cornell_path))
    d, rp = _display(64, 64, **AUTO_ACES_SRGB)
    small, _ = _display(32, 32, **AUTO_ACES_SRGB)
    jenc, penc = JpegEncoder(64, 64), PngEncoder(64, 64)
    try:
        for it in range(1, 5):
            pt.render_pass(it)
        acc = pt.image()
        rgba = torch.zeros((64, 64, 4), dtype=torch.uint8, device="cuda")
        pt.preview_rgba(4, rgba.data_ptr())
        plain = rgba.cpu().numpy()
        before = (pt.preview_jpeg(4, jenc), pt.preview_png(4, penc))
        want = _auto_bytes(acc, 4.0, rp, tab, 4)
        assert want[..., :3].max() > want[..., :3].min()
        buf = torch.full((64, 64, 4), 0xA5, dtype=torch.uint8, device="cuda")
        pt.preview_display(4, d, buf.data_ptr(), 4)
        assert np.array_equal(buf.cpu().numpy(), want)
        assert pt.preview_jpeg(4, jenc, display=d) == encode_jpeg(want, 90, "420")
        png = pt.preview_png(4, penc, display=d)
        assert png == encode_png(want)
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(png)).convert("RGB")), want[..., :3])
        # without display= the files are the ones the methods have always written
        assert (pt.preview_jpeg(4, jenc), pt.preview_png(4, penc)) == before
        assert before == (encode_jpeg(plain, 90, "420"), encode_png(plain))
        with pytest.raises(PtError) as ei:
            pt.preview_display(4, small, buf.data_ptr(), 4)
        assert ei.value.code == 1
    finally:
        for o in (jenc, penc, d, small, pt):
            o.free()
    s2 = _scene(cornell_path)
    half = PathTracer(s2, None, rank=0, world=2)
    d2, _ = _display(64, half.rows, **AUTO_ACES_SRGB)
    try:
        with pytest.raises(PtError) as ei:
            half.preview_display(1, d2, buf.data_ptr(), 4)
        assert ei.value.code == 1
    finally:
        d2.free()
        half.free()


# ---- the preview server --------------------------------------------------------------------------------
def test_preview_server(cornell_path, gpu_device, tab, tmp_path):
    """/frame.jpg with tonemap = aces and srgb = on is the device encoder's file of the restatement's bytes, which is
    stronger than a decoding error bound: test_jpeg_enc_gpu.py's own criterion for a preview frame is that file
    equality.  /frame.png (png_device) and the PBO path show the same pixels; a denoised frame goes through
    display_transform; with the defaults the frame is the one from before."""
    from PIL import Image
    from cuda_pathtracer_amd import encode_jpeg, encode_png
    from cuda_pathtracer_amd import preview as V
    from cuda_pathtracer_amd.pathtrace import decode_jpeg
    rp = R.Params(curve=R.ACES, transfer=R.SRGB)
    ses = V.PreviewSession(_scene(cornell_path, 8), out_dir=str(tmp_path), jpeg=90, png_device=True)
    srv = V.PreviewServer(ses).start(render=False)   # (the test drives the render loop: no waiting)

    def get(path):
        with urllib.request.urlopen(srv.url + path, timeout=10) as r:
            return r.read()
    try:
        ses.run_cuda()
        shown = ses.display_rgb()
        assert get("frame.jpg") == encode_jpeg(shown, 90) and ses._display is None   # the defaults: as before
        ses.set_setting("tonemap", "aces")
        ses.set_setting("srgb", True)
        ses.run_cuda()
        assert ses.iteration == 2   # (no restart)
        want = R.apply(ses.ctx.image(), 2.0, rp, tab)[:, ::-1]   # the window mirrors x
        jpg = get("frame.jpg")
        assert jpg == encode_jpeg(np.ascontiguousarray(want), 90)
        assert decode_jpeg(jpg).shape == (64, 64, 3)
        png = get("frame.png")
        assert png == encode_png(np.ascontiguousarray(want))
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(png)).convert("RGB")), want)
        assert np.array_equal(ses.display_rgb(), want)
        assert ses.state()["settings"]["tonemap"] == "aces"
        # a denoised frame is a host array
        ses.set_setting("denoise", True)
        ses.run_cuda()
        den = R.apply(ses.ctx.denoised(3.0), 1.0, rp, tab)[:, ::-1]
        assert np.array_equal(ses.display_rgb(), den)
        # auto exposure adapts over frames: the session's one object at rate 32
        ses.set_setting("denoise", False)
        ses.set_setting("auto_exposure", True)
        ses.run_cuda()
        ap = R.Params(exposure_mode=R.AUTO, rate=32, curve=R.ACES, transfer=R.SRGB)
        assert np.array_equal(ses.display_rgb(), _auto_bytes(ses.ctx.image(), 4.0, ap, tab)[:, ::-1])
        assert ses._display.info()["metered"] == 1
        assert ses.save_image() is not None
    finally:
        srv.stop()
        ses.close()


# ---- the CLI -------------------------------------------------------------------------------------------
def test_cli(cornell_path, gpu_device, tab, tmp_path):
    from PIL import Image
    from cuda_pathtracer_amd import PathTracer, Scene, build
    outs = {}
    for name, flags in (("plain", []), ("display", ["--tonemap", "aces", "--srgb", "--exposure", "auto"])):
        d = tmp_path / name
        d.mkdir()
        subprocess.run([str(build.CLI), cornell_path, "--iterations", "2", "--out", str(d), *flags], check=True,
                       capture_output=True, timeout=120)
        outs[name] = {f.name.split("samp", 1)[1]: f.read_bytes() for f in d.glob("*.png")}
    assert sorted(outs["plain"]) == [".png"] and sorted(outs["display"]) == [".display.png", ".png"]
    assert outs["display"][".png"] == outs["plain"][".png"]
    s = Scene(cornell_path)
    s.finalize()
    pt = PathTracer(s)
    try:
        pt.render_pass(1)
        pt.render_pass(2)
        acc = pt.image()
    finally:
        pt.free()
    from cuda_pathtracer_amd import tonemap
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(outs["plain"][".png"])).convert("RGB")), tonemap(acc, 2.0))
    rp = R.Params(mirror_x=1, **AUTO_ACES_SRGB)
    got = np.asarray(Image.open(io.BytesIO(outs["display"][".display.png"])).convert("RGB"))
    assert np.array_equal(got, _auto_bytes(acc, 2.0, rp, tab))
