"""The device PNG encoder (csrc/pt_png_enc.hip) against its numpy restatement
(tests/png_enc_ref.py): the files are compared with == on bytes.  Shapes are the smallest at which each part
can go wrong: the CPU tests' sizes and crafted cases, more chunks than one scan tile (1024) with partial last
tile, chunk and deflate block, a payload of several CRC pieces (256 bytes) with a partial first one."""
import ctypes as C
import io
import urllib.request

import numpy as np
import pytest

from tests import png_enc_cases as K
from tests import png_enc_ref as R

pytestmark = pytest.mark.gpu


def _params(filt=R.ADAPTIVE, block=R.BLOCK_DEFAULT, mirror=False, conv=R.CONV_PREVIEW):
    from cuda_pathtracer_amd import PngParams
    p = PngParams.default()
    p.filter, p.block_bytes, p.mirror_x, p.conv = filt, block, int(mirror), conv
    return p


def _gpu(img, filt=R.ADAPTIVE, block=R.BLOCK_DEFAULT, mirror=False):
    from cuda_pathtracer_amd import PngEncoder
    enc = PngEncoder(img.shape[1], img.shape[0], _params(filt, block, mirror))
    try:
        return enc.encode(img)
    finally:
        enc.free()


def _decode(data: bytes) -> np.ndarray:
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)))


@pytest.mark.parametrize("block", K.BLOCKS)
@pytest.mark.parametrize("w,h", K.SIZES)
def test_sizes(gpu_device, w, h, block):
    """Every filter of one size through one upload of the image."""
    img = K.noisy(w, h)
    for filt in K.FILTERS:
        assert _gpu(img, filt, block) == R.encode(img, filt, block).data, filt


@pytest.mark.parametrize("name", sorted(K.crafted()))
def test_crafted(gpu_device, name):
    """Constant image, random bytes, one pixel, both block types, the two length limits (what each reaches is
    asserted in tests/test_png_enc_cpu.py)."""
    img, filt, block = K.crafted()[name]
    assert _gpu(img, filt, block) == K.reference(name).data


def test_many_chunks_partial_last_tile(gpu_device):
    """700 x 500: F has 500 * 2101 = 1050500 bytes = 2051 chunks and 388 bytes (2 scan tiles of 1024 chunks and 4
    chunks), 32 deflate blocks of 32768 bytes and 1924 bytes; the payload spans many CRC pieces, the first partial."""
    img = K.noisy(700, 500)
    ref = R.encode(img)
    n = len(ref.f)
    assert n == 1050500 and n % R.CHUNK == 388 and -(-n // R.CHUNK) == 2 * 1024 + 4 and n % R.BLOCK_DEFAULT == 1924
    assert len(ref.block_types) == 33 and len(ref.payload) + 4 > 8 * 256 and (len(ref.payload) + 4) % 256 != 0
    got = _gpu(img)
    assert got == ref.data
    assert np.array_equal(_decode(got), img)
    # deflate blocks of 256 chunks: a wave takes four rounds of 64 chunks, the last block 4 chunks of its first round
    assert _gpu(img, block=131072) == R.encode(img, block_bytes=131072).data


def test_golden_200(gpu_device):
    img = K.golden_200()
    assert _gpu(img) == R.encode(img).data


@pytest.fixture(scope="module")
def cornell_200(cornell_path, gpu_device):
    """A 1-spp Cornell 200 x 200 context (mostly black and noisy) and its accumulator."""
    from cuda_pathtracer_amd import PathTracer, Scene
    s = Scene(cornell_path)
    s.set_camera((200, 200), 45.0, (0, 5, 10.5), (0, 5, 0), (0, 1, 0))
    s.finalize()
    pt = PathTracer(s)
    pt.render_pass(1)
    yield pt, pt.image()
    pt.free()


def test_cornell_three_routes(cornell_200):
    import torch
    from cuda_pathtracer_amd import PngEncoder
    pt, accum = cornell_200
    ref = R.encode(R.preview_bytes(accum, 1.0)).data
    enc = PngEncoder(200, 200, _params())
    try:
        a = enc.encode(accum, samples=1.0)                    # pt_png_enc_accum
        b = pt.preview_png(1, enc)                            # pt_preview_png
        rgba = torch.empty((200, 200, 4), dtype=torch.uint8, device="cuda")
        pt.preview_rgba(1, rgba.data_ptr())
        c = enc.encode(rgba)                                  # pt_preview_rgba, then pt_png_enc_pixels (stride 4)
        d = enc.encode(rgba.data_ptr(), pixel_stride=4)       # the same through a device pointer
    finally:
        enc.free()
    assert np.array_equal(rgba.cpu().numpy()[..., :3], R.preview_bytes(accum, 1.0))
    assert a == ref and b == ref and c == ref and d == ref


def test_accumulator_conversions(cornell_200):
    """samples > 1 under both conversions, mirrored; CONV_SAVE decodes to pt_tonemap's bytes."""
    from cuda_pathtracer_amd import PngEncoder, tonemap
    _, accum = cornell_200
    acc = accum * np.float32(3.0)
    for conv, conv_bytes in ((R.CONV_PREVIEW, R.preview_bytes), (R.CONV_SAVE, R.save_bytes)):
        enc = PngEncoder(200, 200, _params(mirror=True, conv=conv))
        try:
            got = enc.encode(acc, samples=7.0)
        finally:
            enc.free()
        assert got == R.encode(conv_bytes(acc, 7.0), mirror_x=True).data, conv
    assert np.array_equal(_decode(got), tonemap(acc, 7.0))


@pytest.mark.parametrize("mirror", [False, True])
@pytest.mark.parametrize("conv", [R.CONV_PREVIEW, R.CONV_SAVE])
def test_crafted_accumulator(gpu_device, conv, mirror):
    """pt_png_enc_accum on negatives, values above 1 and both neighbours of every k / 255, under both conversions
    (which agree on every finite value: tests/test_png_enc_cpu.py::test_conversions)."""
    from cuda_pathtracer_amd import PngEncoder, tonemap
    acc = K.accumulator()
    want = (R.save_bytes if conv == R.CONV_SAVE else R.preview_bytes)(acc, 3.0)
    enc = PngEncoder(acc.shape[1], acc.shape[0], _params(mirror=mirror, conv=conv))
    try:
        got = enc.encode(acc, samples=3.0)
    finally:
        enc.free()
    assert got == R.encode(want, mirror_x=mirror).data
    assert np.array_equal(_decode(got), want[:, ::-1] if mirror else want)
    if conv == R.CONV_SAVE and mirror:
        assert np.array_equal(_decode(got), tonemap(acc, 3.0))


def test_save_png(cornell_200, tmp_path):
    from cuda_pathtracer_amd import tonemap
    pt, accum = cornell_200
    path = pt.save_png(str(tmp_path / "out.png"), 1)
    data = open(path, "rb").read()
    assert np.array_equal(_decode(data), tonemap(pt.image(), 1.0))
    assert data == R.encode(R.save_bytes(accum, 1.0), mirror_x=True).data


def test_preview_png_refuses_another_size(cornell_200):
    from cuda_pathtracer_amd import PngEncoder, PtError
    pt, _ = cornell_200
    enc = PngEncoder(200, 199)
    with pytest.raises(PtError):
        pt.preview_png(1, enc)
    enc.free()


def test_mirror_x(gpu_device):
    img = K.noisy(37, 21)
    got = _gpu(img, mirror=True)
    assert got == R.encode(img, mirror_x=True).data == R.encode(np.ascontiguousarray(img[:, ::-1])).data
    assert got != R.encode(img).data


def test_stride_3_against_4(gpu_device):
    rgba = K.noisy(37, 21, chans=4)
    rgb = np.ascontiguousarray(rgba[..., :3])
    ref = R.encode(rgb).data
    assert _gpu(rgb) == ref and _gpu(rgba) == ref


def test_host_entry(gpu_device):
    from cuda_pathtracer_amd import encode_png
    img = K.noisy(50, 34, chans=4)
    assert encode_png(img, filter=4, block_bytes=2048, mirror_x=True) == R.encode(img, 4, 2048, True).data
    assert encode_png(img[..., :3]) == R.encode(img).data


def test_reuse_one_object(gpu_device):
    """A long file, then a short one, then long ones again: no stale bit of the OR-ed stream survives."""
    from cuda_pathtracer_amd import PngEncoder
    rnd = np.random.default_rng(2).integers(0, 256, (48, 64, 3), dtype=np.uint8)
    flat = np.full((48, 64, 3), 77, np.uint8)
    other = K.noisy(64, 48)
    enc = PngEncoder(64, 48, _params(block=2048))
    try:
        got = [enc.encode(im) for im in (rnd, flat, other, rnd)]
    finally:
        enc.free()
    ref = [R.encode(im, block_bytes=2048).data for im in (rnd, flat, other, rnd)]
    assert got == ref and len(ref[1]) < len(ref[0]) // 8


def test_non_default_stream_behind_a_pass(cornell_path, gpu_device):
    import torch
    from cuda_pathtracer_amd import PathTracer, PngEncoder, Scene
    s = Scene(cornell_path)
    s.set_camera((72, 40), 45.0, (0, 5, 10.5), (0, 5, 0), (0, 1, 0))
    s.finalize()
    pt = PathTracer(s)
    enc = PngEncoder(72, 40)
    st = torch.cuda.Stream()
    try:
        pt.render_pass(1, stream=st)
        got = pt.preview_png(1, enc, stream=st)   # queued behind the pass; the read waits for the stream
        accum = pt.image()
    finally:
        enc.free()
        pt.free()
    assert got == R.encode(R.preview_bytes(accum, 1.0)).data


def test_overflow(gpu_device):
    """cap ten bytes short: the negated size, the file's first cap bytes, and nothing behind them."""
    import torch
    from cuda_pathtracer_amd import _native as N
    img = K.noisy(64, 48)
    ref = R.encode(img).data
    cap = len(ref) - 10
    L = N.lib()
    e = C.c_void_p()
    assert L.pt_png_enc_create(64, 48, C.byref(_params()), C.byref(e)) == 0
    pix = torch.from_numpy(img).cuda()
    out = torch.full((cap + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    size = torch.zeros(1, dtype=torch.int64, device="cuda")
    try:
        for short in (cap, 40, 0):   # inside IEND and the CRC; inside the payload; nothing at all
            out.fill_(0xA5)
            assert L.pt_png_enc_pixels(e, pix.data_ptr(), 3, out.data_ptr(), short, size.data_ptr(), None) == 0
            torch.cuda.synchronize()
            assert int(size.cpu()[0]) == -len(ref)
            got = out.cpu().numpy()
            assert got[:short].tobytes() == ref[:short]
            assert (got[short:] == 0xA5).all()
        # the same call with room: the size, and the guard bytes behind the file untouched
        assert L.pt_png_enc_pixels(e, pix.data_ptr(), 3, out.data_ptr(), cap + 10, size.data_ptr(), None) == 0
        torch.cuda.synchronize()
        assert int(size.cpu()[0]) == len(ref)
        got = out.cpu().numpy()
        assert got[:len(ref)].tobytes() == ref and (got[len(ref):] == 0xA5).all()
    finally:
        L.pt_png_enc_destroy(e)
    hout, n = np.zeros(cap, np.uint8), C.c_int64(0)
    rc = L.pt_png_encode_host(64, 48, img.ctypes.data, 3, C.byref(_params()), hout.ctypes.data, cap, C.byref(n))
    assert rc == 1 and n.value == len(ref)   # PT_ERR_ARG and the size needed
    from cuda_pathtracer_amd import PngEncoder, PtError
    enc = PngEncoder(64, 48, cap=cap)
    with pytest.raises(PtError):
        enc.encode(img)
    enc.free()


def test_profile(gpu_device):
    from cuda_pathtracer_amd import PngEncoder
    from cuda_pathtracer_amd import _native as N
    img = K.noisy(64, 48)
    enc = PngEncoder(64, 48)
    try:
        assert N.lib().pt_png_enc_profile(enc._h, 1) == 0
        data = enc.encode(img)
        ms = (C.c_float * 6)()
        assert N.lib().pt_png_enc_profile_read(enc._h, ms) == 0
    finally:
        enc.free()
    assert data == R.encode(img).data and all(0.0 <= v < 1e3 for v in ms)


# ---- the preview window -----------------------------------------------------------------------------------
def _scene(cornell_path, iterations, res=(64, 64)):
    from cuda_pathtracer_amd import Scene
    s = Scene(cornell_path)
    s.set_camera(res, 45.0, (0, 5, 10.5), (0, 5, 0), (0, 1, 0))
    st = s.state()
    s.set_render(iterations, st.traceDepth, st.imageName)
    s.finalize()
    return s


def _frame_png(srv) -> bytes:
    with urllib.request.urlopen(srv.url + "frame.png", timeout=10) as r:
        assert r.headers["Content-Type"] == "image/png"
        return r.read()


def test_preview_server_png_device(cornell_path, gpu_device, tmp_path):
    from cuda_pathtracer_amd import preview as V
    ses = V.PreviewSession(_scene(cornell_path, 8), out_dir=str(tmp_path), png_device=True)
    srv = V.PreviewServer(ses).start(render=False)   # (the test drives the render loop: no waiting)
    try:
        ses.run_cuda()
        ses.run_cuda()
        png = _frame_png(srv)
        shown = ses.display_rgb()
        assert np.array_equal(_decode(png), shown)
        assert png == R.encode(shown).data != V.png_bytes(shown)
        # a denoised frame is a host array: it goes through encode_png with mirror_x
        ses.set_setting("denoise", True)
        ses.run_cuda()
        png = _frame_png(srv)
        assert png == R.encode(ses.display_rgb()).data
        assert ses.save_image() is not None
    finally:
        srv.stop()
        ses.close()


def test_preview_server_without_png_device(cornell_path, gpu_device, tmp_path):
    from cuda_pathtracer_amd import preview as V
    ses = V.PreviewSession(_scene(cornell_path, 4), out_dir=str(tmp_path))
    srv = V.PreviewServer(ses).start(render=False)
    try:
        ses.run_cuda()
        shown = ses.display_rgb()
        assert _frame_png(srv) == V.png_bytes(shown)
        assert ses._png_enc is None
    finally:
        srv.stop()
        ses.close()


def test_cli_device_png(cornell_path, gpu_device, tmp_path):
    """--device-png: the same file name and the same pixels as without it."""
    import subprocess
    from cuda_pathtracer_amd import build
    outs = []
    for flags in ([], ["--device-png"]):
        d = tmp_path / ("dev" if flags else "host")
        d.mkdir()
        subprocess.run([str(build.CLI), cornell_path, "--iterations", "2", "--out", str(d), *flags], check=True,
                       capture_output=True, timeout=120)
        files = sorted(d.glob("*.png"))
        assert len(files) == 1 and files[0].name.endswith(".2samp.png")
        outs.append(files[0].read_bytes())
    assert outs[0] != outs[1] and np.array_equal(_decode(outs[0]), _decode(outs[1]))
