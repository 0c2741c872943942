"""The device JPEG encoder (csrc/pt_jpeg_enc.hip) against its numpy restatement
(tests/jpeg_enc_ref.py): the files are compared with == on bytes.  Shapes are the smallest at which each
part can go wrong: partial blocks and MCUs, more blocks than one scan tile (1024) with a partial last
tile of the blocks kernel (32 blocks), an unstuffed stream longer than one stuffing chunk (4096 bytes)."""
import ctypes as C
import io
import urllib.error
import urllib.request

import numpy as np
import pytest

from tests import jpeg_enc_ref as R

pytestmark = pytest.mark.gpu


def _params(q=90, sub=R.S420, mirror=False):
    from cuda_pathtracer_amd import JpegParams
    p = JpegParams.default()
    p.quality, p.subsampling, p.mirror_x = q, sub, int(mirror)
    return p


def _gpu(img, q=90, sub=R.S420, mirror=False):
    from cuda_pathtracer_amd import JpegEncoder
    enc = JpegEncoder(img.shape[1], img.shape[0], _params(q, sub, mirror))
    try:
        return enc.encode(img)
    finally:
        enc.free()


def _noisy(w, h, seed=0, chans=3):
    rng = np.random.default_rng(7 * w + h + seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([x * 255 // max(w - 1, 1), y * 255 // max(h - 1, 1), (x + y) * 255 // max(w + h - 2, 1)], -1)
    img = np.clip(base + rng.integers(-40, 41, (h, w, 3)), 0, 255).astype(np.uint8)
    if chans == 4:
        img = np.concatenate([img, rng.integers(0, 256, (h, w, 1), dtype=np.uint8)], -1)   # alpha: ignored
    return img


@pytest.mark.parametrize("sub", [R.S444, R.S420])
@pytest.mark.parametrize("w,h", [(1, 1), (8, 8), (7, 5), (17, 9), (64, 48)])
def test_sizes(gpu_device, w, h, sub):
    img = _noisy(w, h)
    assert _gpu(img, 90, sub) == R.encode(img, 90, sub).data


def test_many_blocks_partial_last_tile(gpu_device):
    """264 x 264 in 4:4:4: 3267 blocks = 3 scan tiles and a part, 102 tiles of the blocks kernel and 3 blocks."""
    img = _noisy(264, 264)
    ref = R.encode(img, 90, R.S444)
    assert len(ref.coefs) == 3267 and 3267 % 1024 != 0 and 3267 % 32 != 0
    assert _gpu(img, 90, R.S444) == ref.data


@pytest.mark.parametrize("sub", [R.S444, R.S420])
def test_constant_image(gpu_device, sub):
    """Grey 128: every block is a zero DC difference and EOB, 6 bits for luma and 4 for chroma."""
    img = np.full((48, 64, 3), 128, np.uint8)
    ref = R.encode(img, 90, sub)
    assert not ref.coefs.any()
    assert set(ref.bit_lengths) == {6, 4}
    assert _gpu(img, 90, sub) == ref.data


@pytest.mark.parametrize("sub", [R.S444, R.S420])
def test_random_bytes_quality_100(gpu_device, sub):
    """The longest codes, 0xFF bytes to stuff and an unstuffed stream of several stuffing chunks."""
    img = np.random.default_rng(11).integers(0, 256, (80, 96, 3), dtype=np.uint8)
    ref = R.encode(img, 100, sub)
    assert ref.stuffed > 0 and b"\xff\x00" in ref.data[R.HEADER_BYTES:]
    assert ref.unstuffed_bytes > 2 * R.STUFF_CHUNK and ref.unstuffed_bytes % R.STUFF_CHUNK != 0
    assert _gpu(img, 100, sub) == ref.data


def test_stuffing_scan_two_sums_per_lane(gpu_device):
    """512 x 512 random bytes, quality 100, 4:4:4: more than 256 stuffing chunks, so the one-workgroup scan of
    their sums takes two per lane, and the last chunk is partial."""
    img = np.random.default_rng(11).integers(0, 256, (512, 512, 3), dtype=np.uint8)
    ref = R.encode(img, 100, R.S444)
    assert len(ref.coefs) == 12288 and ref.unstuffed_bytes == 1069358
    assert ref.unstuffed_bytes > 256 * R.STUFF_CHUNK and ref.unstuffed_bytes % R.STUFF_CHUNK != 0
    assert _gpu(img, 100, R.S444) == ref.data


def test_zero_runs_of_16(gpu_device):
    """One block of the highest-frequency cosine on a flat field: a run of 62 zeros before the last coefficient."""
    x = np.arange(8)
    c7 = np.cos((2 * x + 1) * 7 * np.pi / 16)
    img = np.full((16, 24, 3), 128, np.uint8)
    img[8:16, 8:16] = np.clip(128 + 100 * np.outer(c7, c7), 0, 255).astype(np.uint8)[..., None]
    ref = R.encode(img, 50, R.S444)
    assert ref.zrl >= 3
    assert _gpu(img, 50, R.S444) == ref.data


@pytest.fixture(scope="module")
def cornell_200(cornell_path, gpu_device):
    """A 1-spp Cornell 200 x 200 context (noisy: the hard case for the entropy coder) and its accumulator."""
    from cuda_pathtracer_amd import PathTracer, Scene
    s = Scene(cornell_path)
    s.set_camera((200, 200), 45.0, (0, 5, 10.5), (0, 5, 0), (0, 1, 0))
    s.finalize()
    pt = PathTracer(s)
    pt.render_pass(1)
    yield pt, pt.image()
    pt.free()


@pytest.mark.parametrize("sub", [R.S444, R.S420])
def test_cornell_three_routes(cornell_200, sub):
    import torch
    from cuda_pathtracer_amd import JpegEncoder
    pt, accum = cornell_200
    ref = R.encode(R.preview_bytes(accum, 1.0), 90, sub).data
    enc = JpegEncoder(200, 200, _params(90, sub))
    try:
        a = enc.encode(accum, samples=1.0)                    # pt_jpeg_enc_accum
        b = pt.preview_jpeg(1, enc)                           # pt_preview_jpeg
        rgba = torch.empty((200, 200, 4), dtype=torch.uint8, device="cuda")
        pt.preview_rgba(1, rgba.data_ptr())
        c = enc.encode(rgba)                                  # pt_preview_rgba, then pt_jpeg_enc_pixels (stride 4)
        d = enc.encode(rgba.data_ptr(), pixel_stride=4)       # the same through a device pointer
    finally:
        enc.free()
    assert np.array_equal(rgba.cpu().numpy()[..., :3], R.preview_bytes(accum, 1.0))
    assert a == ref and b == ref and c == ref and d == ref


def test_accumulator_division(cornell_200):
    """samples > 1: the bytes are k_preview's (int)((double)(v / n) * 255.0)."""
    from cuda_pathtracer_amd import JpegEncoder
    _, accum = cornell_200
    enc = JpegEncoder(200, 200, _params(90, R.S420, True))
    try:
        got = enc.encode(accum * np.float32(3.0), samples=7.0)
    finally:
        enc.free()
    assert got == R.encode(R.preview_bytes(accum * np.float32(3.0), 7.0), 90, R.S420, True).data


def test_preview_jpeg_refuses_another_size(cornell_200):
    from cuda_pathtracer_amd import JpegEncoder, PtError
    pt, _ = cornell_200
    enc = JpegEncoder(200, 199)
    with pytest.raises(PtError):
        pt.preview_jpeg(1, enc)
    enc.free()


@pytest.mark.parametrize("sub", [R.S444, R.S420])
def test_mirror_x(gpu_device, sub):
    img = _noisy(37, 21)
    got = _gpu(img, 90, sub, mirror=True)
    assert got == R.encode(img, 90, sub, True).data == R.encode(np.ascontiguousarray(img[:, ::-1]), 90, sub).data
    assert got != R.encode(img, 90, sub).data


def test_stride_3_against_4(gpu_device):
    rgba = _noisy(37, 21, chans=4)
    rgb = np.ascontiguousarray(rgba[..., :3])
    ref = R.encode(rgb, 90, R.S420).data
    assert _gpu(rgb) == ref and _gpu(rgba) == ref


@pytest.mark.parametrize("sub", [R.S444, R.S420])
def test_quality_1(gpu_device, sub):
    img = _noisy(64, 48)
    assert _gpu(img, 1, sub) == R.encode(img, 1, sub).data


def test_host_entry(gpu_device):
    from cuda_pathtracer_amd import encode_jpeg
    from cuda_pathtracer_amd.pathtrace import decode_jpeg
    img = _noisy(50, 34, chans=4)
    data = encode_jpeg(img, 75, "444", mirror_x=True)
    assert data == R.encode(img, 75, R.S444, True).data
    assert decode_jpeg(data).shape == (34, 50, 3)
    assert encode_jpeg(img[..., :3]) == R.encode(img, 90, R.S420).data


def test_reuse_one_object(gpu_device):
    """A long file, then a short one, then the long one again: no stale bit of the OR-ed stream survives."""
    from cuda_pathtracer_amd import JpegEncoder
    rnd = np.random.default_rng(2).integers(0, 256, (48, 64, 3), dtype=np.uint8)
    flat = np.full((48, 64, 3), 77, np.uint8)
    other = _noisy(64, 48)
    enc = JpegEncoder(64, 48, _params(100, R.S444))
    try:
        got = [enc.encode(im) for im in (rnd, flat, other, rnd)]
    finally:
        enc.free()
    assert got == [R.encode(im, 100, R.S444).data for im in (rnd, flat, other, rnd)]


def test_two_encoders_alive(gpu_device):
    """A JPEG and a PNG encoder used alternately on one stream: nothing of one object's encode reaches the other's
    (the unit the two share keeps no state of its own)."""
    import torch
    from cuda_pathtracer_amd import JpegEncoder, PngEncoder
    from tests import png_enc_ref as RP
    a, b = _noisy(64, 48), _noisy(64, 48, seed=1)
    assert not np.array_equal(a, b)
    jpg, png, st = JpegEncoder(64, 48), PngEncoder(64, 48), torch.cuda.Stream()
    try:
        got = [enc.encode(im, stream=st) for enc, im in ((jpg, a), (png, a), (jpg, b), (png, b), (jpg, a))]
    finally:
        jpg.free()
        png.free()
    ja, jb = R.encode(a, 90, R.S420).data, R.encode(b, 90, R.S420).data
    assert got == [ja, RP.encode(a).data, jb, RP.encode(b).data, ja]
    assert got[0] == got[4] != got[2]


def test_non_default_stream_behind_a_pass(cornell_path, gpu_device):
    import torch
    from cuda_pathtracer_amd import JpegEncoder, PathTracer, Scene
    s = Scene(cornell_path)
    s.set_camera((72, 40), 45.0, (0, 5, 10.5), (0, 5, 0), (0, 1, 0))
    s.finalize()
    pt = PathTracer(s)
    enc = JpegEncoder(72, 40)
    st = torch.cuda.Stream()
    try:
        pt.render_pass(1, stream=st)
        got = pt.preview_jpeg(1, enc, stream=st)   # queued behind the pass; the read waits for the stream
        accum = pt.image()
    finally:
        enc.free()
        pt.free()
    assert got == R.encode(R.preview_bytes(accum, 1.0), 90, R.S420).data


def test_overflow(gpu_device):
    """cap ten bytes short: the negated size, the file's first cap bytes, and nothing behind them."""
    import torch
    from cuda_pathtracer_amd import _native as N
    img = _noisy(64, 48)
    ref = R.encode(img, 90, R.S420).data
    cap = len(ref) - 10
    L = N.lib()
    e = C.c_void_p()
    assert L.pt_jpeg_enc_create(64, 48, C.byref(_params()), C.byref(e)) == 0
    pix = torch.from_numpy(img).cuda()
    out = torch.full((cap + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    size = torch.zeros(1, dtype=torch.int64, device="cuda")
    try:
        assert L.pt_jpeg_enc_pixels(e, pix.data_ptr(), 3, out.data_ptr(), cap, size.data_ptr(), None) == 0
        torch.cuda.synchronize()
        assert int(size.cpu()[0]) == -len(ref)
        got = out.cpu().numpy()
        assert got[:cap].tobytes() == ref[:cap]
        assert (got[cap:] == 0xA5).all()
        # the same call with room: the size, and the guard bytes behind the file untouched
        assert L.pt_jpeg_enc_pixels(e, pix.data_ptr(), 3, out.data_ptr(), cap + 10, size.data_ptr(), None) == 0
        torch.cuda.synchronize()
        assert int(size.cpu()[0]) == len(ref)
        got = out.cpu().numpy()
        assert got[:len(ref)].tobytes() == ref and (got[len(ref):] == 0xA5).all()
    finally:
        L.pt_jpeg_enc_destroy(e)
    hout, n = np.zeros(cap, np.uint8), C.c_int64(0)
    rc = L.pt_jpeg_encode_host(64, 48, img.ctypes.data, 3, C.byref(_params()), hout.ctypes.data, cap, C.byref(n))
    assert rc == 1 and n.value == len(ref)   # PT_ERR_ARG and the size needed
    from cuda_pathtracer_amd import JpegEncoder, PtError
    enc = JpegEncoder(64, 48, cap=cap)
    with pytest.raises(PtError):
        enc.encode(img)
    enc.free()


# ---- the preview window -----------------------------------------------------------------------------------
def _scene(cornell_path, iterations, res=(64, 64)):
    from cuda_pathtracer_amd import Scene
    s = Scene(cornell_path)
    s.set_camera(res, 45.0, (0, 5, 10.5), (0, 5, 0), (0, 1, 0))
    st = s.state()
    s.set_render(iterations, st.traceDepth, st.imageName)
    s.finalize()
    return s


def _read_part(resp):
    """One part of a multipart/x-mixed-replace body: (iteration, file)."""
    assert resp.readline().strip() == b"--frame"
    head = {}
    while True:
        line = resp.readline().strip()
        if not line:
            break
        k, v = line.split(b":", 1)
        head[k.strip().lower()] = v.strip()
    assert head[b"content-type"] == b"image/jpeg"
    data = resp.read(int(head[b"content-length"]))
    assert resp.readline() == b"\r\n"
    return int(head[b"x-iteration"]), data


def test_preview_server_jpeg(cornell_path, gpu_device, tmp_path):
    from PIL import Image
    from cuda_pathtracer_amd import encode_jpeg
    from cuda_pathtracer_amd import preview as V
    from cuda_pathtracer_amd.pathtrace import decode_jpeg
    ses = V.PreviewSession(_scene(cornell_path, 8), out_dir=str(tmp_path), jpeg=90)
    srv = V.PreviewServer(ses).start(render=False)   # (the test drives the render loop: no waiting)
    try:
        stream = urllib.request.urlopen(srv.url + "stream.mjpg", timeout=30)
        assert stream.headers["Content-Type"].startswith("multipart/x-mixed-replace")
        parts = []
        for _ in range(3):
            ses.run_cuda()
            parts.append(_read_part(stream))
        stream.close()
        assert [it for it, _ in parts] == [1, 2, 3] and ses.iteration == 3
        assert len({data for _, data in parts}) == 3
        with urllib.request.urlopen(srv.url + "frame.jpg", timeout=10) as r:
            assert r.headers["Content-Type"] == "image/jpeg"
            jpg = r.read()
        assert jpg == parts[-1][1]
        assert decode_jpeg(jpg).shape == (64, 64, 3)
        shown = ses.display_rgb()   # (read from the PBO on demand)
        assert jpg == encode_jpeg(shown, 90) == R.encode(shown, 90, R.S420).data
        with urllib.request.urlopen(srv.url + "frame.png", timeout=10) as r:
            assert np.array_equal(np.asarray(Image.open(io.BytesIO(r.read()))), shown)
        with urllib.request.urlopen(srv.url, timeout=10) as r:
            assert b"/frame.jpg" in r.read()
        # a denoised frame is a host array: it goes through encode_jpeg with mirror_x
        ses.set_setting("denoise", True)
        ses.run_cuda()
        assert ses.jpeg_bytes == R.encode(ses.display_rgb(), 90, R.S420).data
        assert ses.save_image() is not None
    finally:
        srv.stop()
        ses.close()


def test_preview_server_without_jpeg(cornell_path, gpu_device, tmp_path):
    from cuda_pathtracer_amd import preview as V
    ses = V.PreviewSession(_scene(cornell_path, 4), out_dir=str(tmp_path))
    srv = V.PreviewServer(ses).start(render=False)
    try:
        ses.run_cuda()
        for path in ("frame.jpg", "stream.mjpg"):
            with pytest.raises(urllib.error.HTTPError) as err:
                urllib.request.urlopen(srv.url + path, timeout=10)
            assert err.value.code == 404
        with urllib.request.urlopen(srv.url, timeout=10) as r:
            assert b"/frame.jpg" not in r.read()
    finally:
        srv.stop()
        ses.close()
