"""The bloom on the device (csrc/pt_bloom.hip) against its numpy restatement (tests/bloom_ref.py):
every comparison is == on the bits of the floats (a NaN, which only passes through from the input, has to be a NaN
at the same place).  Shapes are the smallest at which each part can go wrong (bloom_cases.SIZES)."""
import io
import subprocess

import numpy as np
import pytest

from tests import bloom_cases as K
from tests import bloom_ref as R
from tests import display_ref as D

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = 64                 # floats on either side of the output
SENTINEL = 0x5A5A5A5A


def _params(rp: R.Params):
    from cuda_pathtracer_amd import BloomParams
    p = BloomParams.default()
    p.threshold, p.strength, p.spread, p.clamp, p.levels = rp.threshold, rp.strength, rp.spread, rp.clamp, rp.levels
    return p


def _same(got: np.ndarray, want: np.ndarray, what=None) -> None:
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]), what


def _apply(acc, samples, rp, offset=0, in_place=False, obj=None, stream=None):
    """pt_bloom_apply between device buffers, `offset` floats off their 16-byte alignment, with a guard band."""
    import torch
    from cuda_pathtracer_amd import Bloom
    h, w = acc.shape[:2]
    n = w * h * 3
    src = torch.zeros(n + 8, dtype=torch.float32, device="cuda")
    src[offset:offset + n] = torch.from_numpy(acc).cuda().reshape(-1)
    buf = torch.full((n + 2 * GUARD + 8,), SENTINEL, dtype=torch.int32, device="cuda")
    b = obj or Bloom(w, h, _params(rp))
    try:
        if in_place:
            b.apply(src.data_ptr() + 4 * offset, samples, src.data_ptr() + 4 * offset, stream=stream)
            torch.cuda.synchronize()
            return src.cpu().numpy()[offset:offset + n].reshape(h, w, 3)
        b.apply(src.data_ptr() + 4 * offset, samples, buf.data_ptr() + 4 * (GUARD + offset), stream=stream)
        torch.cuda.synchronize()
    finally:
        if obj is None:
            b.free()
    got = buf.cpu().numpy()
    lo = GUARD + offset
    assert (got[:lo] == SENTINEL).all() and (got[lo + n:] == SENTINEL).all(), "the guard band"
    assert np.array_equal(src.cpu().numpy()[offset:offset + n].view(np.uint32), acc.reshape(-1).view(np.uint32)), "the input"
    return got[lo:lo + n].view(np.float32).reshape(h, w, 3)


# ---- the kernels ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", K.SIZES)
def test_sizes(gpu_device, w, h):
    acc = K.noisy(w, h)
    for samples in (1.0, 3.0):
        _same(_apply(acc, samples, R.Params()), R.apply(acc, samples, R.Params()), (w, h, samples))


@pytest.mark.parametrize("w,h", [(5, 7), (33, 31)])
@pytest.mark.parametrize("levels", [1, 2, 0, 12])
def test_levels(gpu_device, w, h, levels):
    acc = K.noisy(w, h, seed=1)
    rp = R.Params(threshold=0.5, levels=levels)
    _same(_apply(acc, 3.0, rp), R.apply(acc, 3.0, rp))


@pytest.mark.parametrize("w,h", [(17, 15), (65, 33)])
def test_parameters(gpu_device, w, h):
    acc = K.noisy(w, h, seed=2)
    for samples in (1.0, 3.0):
        for t, s, sp in K.TRIPLES:
            rp = R.Params(threshold=t, strength=s, spread=sp)
            _same(_apply(acc, samples, rp), R.apply(acc, samples, rp), (t, s, sp, samples))
        # a pixel whose luminance is the threshold exactly: it does not glare, its brighter neighbours do
        lum = R.luminance(R.clamped(acc, samples, R.Params()))
        y, x = np.unravel_index(np.argsort(lum, axis=None)[lum.size // 2], lum.shape)
        rp = R.Params(threshold=float(lum[y, x]), strength=1.0)
        b0 = R.bright(acc, samples, rp)
        assert F(rp.threshold) == lum[y, x] and (b0[y, x] == 0).all() and (b0 > 0).any()
        _same(_apply(acc, samples, rp), R.apply(acc, samples, rp), ("L == threshold", samples))


@pytest.mark.parametrize("samples", [1.0, 3.0])
def test_edge_rows(gpu_device, samples):
    """0, -0, a denormal, NaN, both infinities, a negative, clamp, the float below it and 1e30 in every channel of the
    first, the middle and the last row."""
    acc = K.edge_image()
    for rp in (R.Params(), R.Params(threshold=0.0, strength=1.0, spread=1.0), R.Params(clamp=2.0, levels=12)):
        got = _apply(acc, samples, rp)
        _same(got, R.apply(acc, samples, rp), rp)
        fin = np.isfinite(acc)
        assert np.isfinite(got[fin]).all() and not np.signbit(got[fin & (acc >= 0)]).any()


@pytest.mark.parametrize("w,h", [(16, 16), (65, 33)])
def test_unaligned_pointers(gpu_device, w, h):
    acc = K.noisy(w, h, seed=3)
    want = R.apply(acc, 2.0, R.Params(threshold=0.25))
    for offset in (1, 2, 3):
        _same(_apply(acc, 2.0, R.Params(threshold=0.25), offset=offset), want, offset)


@pytest.mark.parametrize("w,h", [(5, 7), (129, 67)])
def test_in_place_and_twice(gpu_device, w, h):
    from cuda_pathtracer_amd import Bloom
    acc = K.noisy(w, h, seed=4)
    rp = R.Params(threshold=0.5, spread=1.0)
    want = R.apply(acc, 3.0, rp)
    _same(_apply(acc, 3.0, rp, in_place=True), want)
    _same(_apply(acc, 3.0, rp, offset=1, in_place=True), want)
    b = Bloom(w, h, _params(rp))
    try:
        first = _apply(acc, 3.0, rp, obj=b)
        _same(_apply(K.noisy(w, h, seed=5), 1.0, rp, obj=b), R.apply(K.noisy(w, h, seed=5), 1.0, rp))   # (the pyramid is reused)
        second = _apply(acc, 3.0, rp, obj=b)
    finally:
        b.free()
    _same(first, want)
    assert np.array_equal(first.view(np.uint32), second.view(np.uint32))


def test_second_stream(gpu_device):
    """The input written on one stream, the apply on another behind the caller's event."""
    import torch
    from cuda_pathtracer_amd import Bloom
    acc = K.noisy(257, 5, seed=6)
    rp = R.Params(threshold=0.5)
    host = torch.from_numpy(acc).pin_memory()
    src = torch.zeros((5, 257, 3), dtype=torch.float32, device="cuda")
    out = torch.zeros_like(src)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    b = Bloom(257, 5, _params(rp))
    try:
        with torch.cuda.stream(s1):
            src.copy_(host, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(s1)
        s2.wait_event(ev)
        assert b.apply(src.data_ptr(), 2.0, out.data_ptr(), stream=s2) is None
        s2.synchronize()
        got = out.cpu().numpy()
    finally:
        b.free()
    _same(got, R.apply(acc, 2.0, rp))


def test_host_arrays(gpu_device):
    from cuda_pathtracer_amd import Bloom, bloom
    for (w, h), samples in (((5, 7), 1.0), ((65, 33), 3.0)):
        acc = K.noisy(w, h, seed=7)
        rp = R.Params(threshold=0.3, strength=0.5)
        want = R.apply(acc, samples, rp)
        _same(bloom(acc, samples, _params(rp)), want)
        b = Bloom(w, h, _params(rp))
        try:
            _same(b.apply(acc, samples), want)
        finally:
            b.free()
    _same(bloom(K.edge_image(), 1.0), R.apply(K.edge_image(), 1.0, R.Params()))


def test_arguments(gpu_device):
    import torch
    from cuda_pathtracer_amd import Bloom, PtError, bloom
    b = Bloom(8, 8)
    acc = torch.zeros(8 * 8 * 3 * 3, dtype=torch.float32, device="cuda")
    a = acc.data_ptr()
    n = 8 * 8 * 12
    try:
        for args in [(a, 0.0, a + n), (a, float("nan"), a + n), (a, float("inf"), a + n), (a, -1.0, a + n), (a, 1.0, a + 4),
                     (a + n, 1.0, a + 4), (a, 1.0, a + n - 4), (a + 2, 1.0, a + n), (a, 1.0, a + n + 1), (0, 1.0, a), (a, 1.0, 0)]:
            with pytest.raises(PtError) as ei:
                b.apply(*args)
            assert ei.value.code == 1, args
        b.apply(a, 1.0, a + n)   # (adjacent: no overlap)
        b.apply(a, 1.0, a)
        torch.cuda.synchronize()
    finally:
        b.free()
    with pytest.raises(PtError):
        bloom(np.zeros((4, 4, 3), np.float32), 0.0)
    with pytest.raises(ValueError):
        bloom(np.zeros((4, 4), np.float32), 1.0)


# ---- the context path ----------------------------------------------------------------------------------
BLOOM = R.Params(threshold=0.2, strength=0.5)
ACES_SRGB = dict(curve=D.ACES, transfer=D.SRGB)


def _scene(cornell_path, iterations=4, res=(64, 64)):
    from cuda_pathtracer_amd import Scene
    s = Scene(cornell_path)
    s.set_camera(res, 45.0, (0, 5, 10.5), (0, 5, 0), (0, 1, 0))
    st = s.state()
    s.set_render(iterations, st.traceDepth, st.imageName)
    s.finalize()
    return s


def _display(w, h, **kw):
    from cuda_pathtracer_amd import DisplayParams, DisplayTransform
    p = DisplayParams.default()
    for k, v in kw.items():
        setattr(p, k, v)
    return DisplayTransform(w, h, p), D.Params(**kw)


def test_context_path(cornell_path, gpu_device):
    import torch
    from cuda_pathtracer_amd import (EXR_ALBEDO, EXR_BEAUTY, Bloom, ExrEncoder, HdrEncoder, JpegEncoder, PathTracer, PngEncoder,
                                     PtError, bloom, display_tables, encode_jpeg, encode_png, exr_ctx_channels)
    tab = display_tables()
    pt = PathTracer(_scene(cornell_path))
    b, small = Bloom(64, 64, _params(BLOOM)), Bloom(32, 32, _params(BLOOM))
    d, dp = _display(64, 64, **ACES_SRGB)
    auto, ap = _display(64, 64, exposure_mode=D.AUTO, **ACES_SRGB)
    jenc, penc, henc = JpegEncoder(64, 64), PngEncoder(64, 64), HdrEncoder(64, 64)
    xenc = ExrEncoder(64, 64, exr_ctx_channels(EXR_BEAUTY))
    try:
        for it in range(1, 5):
            pt.render_pass(it)
        acc = pt.image()
        want = R.apply(acc, 4.0, BLOOM)
        assert (want > acc).any() and R.glare(acc, 4.0, BLOOM).max() > 0
        before = (pt.preview_jpeg(4, jenc), pt.preview_png(4, penc), pt.preview_hdr(4, henc), pt.preview_exr(4, xenc))
        got = pt.preview_bloom(4, b)
        _same(got, want)
        _same(got, bloom(acc, 4.0, _params(BLOOM)))
        out = torch.zeros((64, 64, 3), dtype=torch.float32, device="cuda")
        assert pt.preview_bloom(4, b, out.data_ptr()) is None
        torch.cuda.synchronize()
        _same(out.cpu().numpy(), want)
        _same(pt.image(), acc)   # (the accumulator is not touched)
        # bloom, then the display transform: the composition of the two restatements
        shown = D.apply(want, 4.0, dp, tab, stride=4)
        buf = torch.full((64, 64, 4), 0xA5, dtype=torch.uint8, device="cuda")
        pt.preview_display(4, d, buf.data_ptr(), 4, bloom=b)
        torch.cuda.synchronize()
        assert np.array_equal(buf.cpu().numpy(), shown)
        assert not np.array_equal(shown, D.apply(acc, 4.0, dp, tab, stride=4))
        _, (e, _) = D.meter(want, 4.0, ap)
        pt.preview_display(4, auto, buf.data_ptr(), 4, bloom=b)
        torch.cuda.synchronize()
        assert np.array_equal(buf.cpu().numpy(), D.apply(want, 4.0, ap, tab, D.multiplier(e, tab["pow2"]), 4))
        assert pt.preview_png(4, penc, display=d, bloom=b) == encode_png(shown)
        assert pt.preview_jpeg(4, jenc, display=d, bloom=b) == encode_jpeg(shown, 90, "420")
        # without a display transform the encoders' accumulator entries take the bloom's buffer
        assert pt.preview_png(4, penc, bloom=b) == penc.encode(want, samples=4.0)
        assert pt.preview_jpeg(4, jenc, bloom=b) == jenc.encode(want, samples=4.0)
        assert pt.preview_hdr(4, henc, bloom=b) == henc.encode(want, 4.0)
        planes = [np.ascontiguousarray(want[..., c]) for c in range(3)]
        assert pt.preview_exr(4, xenc, bloom=b) == xenc.encode(planes, divisors=[4.0] * 3)
        # without bloom= the files are the ones the methods have always written
        assert (pt.preview_jpeg(4, jenc), pt.preview_png(4, penc), pt.preview_hdr(4, henc), pt.preview_exr(4, xenc)) == before
        assert pt.preview_hdr(4, henc, bloom=b) != before[2]
        # the refusals
        with pytest.raises(PtError) as ei:
            pt.preview_bloom(4, small, out.data_ptr())
        assert ei.value.code == 1
        with pytest.raises(PtError) as ei:
            pt.preview_bloom(0, b, out.data_ptr())
        assert ei.value.code == 1
        with pytest.raises(ValueError):
            pt.preview_exr(4, xenc, EXR_BEAUTY | EXR_ALBEDO, bloom=b)
        # what reads the bloom's buffer has to be of its size
        big, _ = _display(128, 64)
        benc = PngEncoder(64, 128)
        try:
            with pytest.raises(ValueError):
                pt.preview_display(4, big, buf.data_ptr(), 4, bloom=b)
            with pytest.raises(ValueError):
                pt.preview_png(4, benc, bloom=b)
        finally:
            big.free()
            benc.free()
    finally:
        for o in (jenc, penc, henc, xenc, d, auto, b, small, pt):
            o.free()
    half = PathTracer(_scene(cornell_path), None, rank=0, world=2)
    b2 = Bloom(64, half.rows, _params(BLOOM))
    try:
        with pytest.raises(PtError) as ei:
            half.preview_bloom(1, b2, out.data_ptr())
        assert ei.value.code == 1
    finally:
        b2.free()
        half.free()


def test_preview_session(cornell_path, gpu_device, tmp_path):
    """The panel's bloom and bloom_threshold: display only; the frame is the bloom's, then the display transform's."""
    from cuda_pathtracer_amd import display_tables, encode_png
    from cuda_pathtracer_amd import preview as V
    tab = display_tables()
    ses = V.PreviewSession(_scene(cornell_path, 8), out_dir=str(tmp_path), png_device=True)
    try:
        ses.run_cuda()
        plain = ses.display_rgb()
        assert ses._bloom is None and ses._display is None
        ses.set_setting("bloom", BLOOM.strength)
        ses.set_setting("bloom_threshold", BLOOM.threshold)
        ses.run_cuda()
        assert ses.iteration == 2   # (no restart)
        want = D.apply(R.apply(ses.ctx.image(), 2.0, BLOOM), 2.0, D.Params(), tab)[:, ::-1]
        assert np.array_equal(ses.display_rgb(), want)
        assert ses.png_frame() == encode_png(np.ascontiguousarray(want))
        ses.set_setting("tonemap", "aces")
        ses.run_cuda()
        want = D.apply(R.apply(ses.ctx.image(), 3.0, BLOOM), 3.0, D.Params(curve=D.ACES), tab)[:, ::-1]
        assert np.array_equal(ses.display_rgb(), want)
        ses.set_setting("denoise", True)   # a denoised frame is a host array: bloom() on it
        ses.run_cuda()
        den = D.apply(R.apply(ses.ctx.denoised(4.0), 1.0, BLOOM), 1.0, D.Params(curve=D.ACES), tab)[:, ::-1]
        assert np.array_equal(ses.display_rgb(), den)
        ses.set_setting("denoise", False)
        ses.set_setting("tonemap", "none")
        ses.set_setting("bloom", 0.0)
        ses.run_cuda()
        assert ses._bloom is None and ses.display_rgb().shape == plain.shape
    finally:
        ses.close()


# ---- the CLI -------------------------------------------------------------------------------------------
def test_cli(cornell_path, gpu_device, tmp_path):
    from PIL import Image
    from cuda_pathtracer_amd import PathTracer, Scene, build, display_tables
    tab = display_tables()
    runs = {"plain": [], "bloom": ["--bloom", "0.5", "--bloom-threshold", "0.2"],
            "both": ["--bloom", "0.5", "--bloom-threshold", "0.2", "--bloom-levels", "3", "--tonemap", "aces", "--srgb"]}
    outs = {}
    for name, flags in runs.items():
        d = tmp_path / name
        d.mkdir()
        subprocess.run([str(build.CLI), cornell_path, "--iterations", "2", "--out", str(d), *flags], check=True,
                       capture_output=True, timeout=120)
        outs[name] = {f.name.split("samp", 1)[1]: f.read_bytes() for f in d.glob("*.png")}
    assert sorted(outs["plain"]) == [".png"] and sorted(outs["bloom"]) == [".bloom.png", ".png"]
    assert sorted(outs["both"]) == [".bloom.png", ".display.png", ".png"]
    assert outs["bloom"][".png"] == outs["plain"][".png"] == outs["both"][".png"]
    for bad in (["--bloom", "-1"], ["--bloom-levels", "13"], ["--bloom-threshold", "x"], ["--bloom", "0.5", "--adaptive", "0.01"]):
        assert subprocess.run([str(build.CLI), cornell_path, *bad], capture_output=True, timeout=120).returncode == 1
    s = Scene(cornell_path)
    s.finalize()
    pt = PathTracer(s)
    try:
        pt.render_pass(1)
        pt.render_pass(2)
        acc = pt.image()
    finally:
        pt.free()

    def pixels(data):
        return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
    assert np.array_equal(pixels(outs["bloom"][".bloom.png"]), D.apply(R.apply(acc, 2.0, BLOOM), 2.0, D.Params(mirror_x=1), tab))
    rp = D.Params(mirror_x=1, **ACES_SRGB)
    assert np.array_equal(pixels(outs["both"][".display.png"]), D.apply(acc, 2.0, rp, tab))
    three = R.Params(threshold=0.2, strength=0.5, levels=3)
    assert np.array_equal(pixels(outs["both"][".bloom.png"]), D.apply(R.apply(acc, 2.0, three), 2.0, rp, tab))
