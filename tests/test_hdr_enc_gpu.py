"""The device Radiance HDR encoder (csrc/pt_hdr_enc.hip) against the host library's encode_hdr: the
files are compared with == on bytes, and at the small sizes also against the line-by-line restatement of the
reference's writer (oracle.hdr_oracle).  Shapes are the smallest at which each part can go wrong: flat rows on both
sides of the coded range, rows shorter than, equal to and just longer than a wave's step of 64 bytes, widths that
are no multiple of the four pixels a lane converts, several rows per workgroup stride, more (row, plane) lengths
than one scan tile of 1024, and the longest coded row."""
import ctypes as C
import urllib.error
import urllib.request

import numpy as np
import pytest

from oracle import hdr_oracle
from tests import hdr_enc_cases as K
from tests import hdr_enc_ref as R

pytestmark = pytest.mark.gpu


def _params(mirror=True):
    from cuda_pathtracer_amd import HdrParams
    p = HdrParams.default()
    p.mirror_x = int(mirror)
    return p


def _gpu(acc, samples, mirror=True):
    from cuda_pathtracer_amd import HdrEncoder
    enc = HdrEncoder(acc.shape[1], acc.shape[0], _params(mirror))
    try:
        return enc.encode(acc, samples)
    finally:
        enc.free()


@pytest.mark.parametrize("w,h", [(7, 3), (1, 1), (8, 1), (9, 2), (64, 1), (65, 3), (130, 2), (257, 5)])
def test_small_sizes(gpu_device, w, h):
    from cuda_pathtracer_amd import encode_hdr
    acc = K.noisy(w, h)
    got = _gpu(acc, 3.0)
    assert got == encode_hdr(acc, 3.0)
    assert got == hdr_oracle.encode_hdr(acc, 3.0)


def test_many_rows(gpu_device):
    """700 x 500: 2000 (row, plane) lengths, a scan tile of 1024 and a partial one; rows of 10 steps and 60 bytes."""
    from cuda_pathtracer_amd import encode_hdr
    acc = K.noisy(700, 500)
    got = _gpu(acc, 3.0)
    assert got == encode_hdr(acc, 3.0)
    dec = hdr_oracle.decode_hdr(got)
    ref = (acc / np.float32(3.0))[:, ::-1]
    assert (np.abs(dec - ref) <= ref.max(axis=2, keepdims=True) * 2 ** -7 + 1e-30).all()


@pytest.mark.parametrize("w", [32767, 32768])
def test_longest_coded_row_and_the_flat_one_behind_it(gpu_device, w):
    """32767 x 1: 512 steps in one wave, W >> 8 = 127 in the row marker; 32768 x 1 is flat."""
    from cuda_pathtracer_amd import encode_hdr
    acc = K.noisy(w, 1)
    got = _gpu(acc, 3.0)
    assert got == encode_hdr(acc, 3.0)
    assert (len(got) == len(R.header(w, 1)) + 4 * w) == (w == 32768)


@pytest.mark.parametrize("others", ["random", "constant"])
@pytest.mark.parametrize("w", sorted(K.by_width()))
def test_crafted_rows(gpu_device, w, others):
    """Every crafted row (tests/test_hdr_enc_cpu.py asserts what each reaches) as the R plane of an image."""
    from cuda_pathtracer_amd import encode_hdr
    names, stacked = K.by_width()[w]
    acc = K.accumulator_of_rows(stacked, others, seed=w)
    got = _gpu(acc, 1.0, mirror=False)
    assert got == encode_hdr(np.ascontiguousarray(acc[:, ::-1]), 1.0), names
    assert got == R.encode(acc, 1.0, mirror_x=False)


@pytest.mark.parametrize("mirror", [True, False])
@pytest.mark.parametrize("samples", K.ACC_SAMPLES)
def test_crafted_accumulator(gpu_device, samples, mirror):
    """Zeros, the 1e-32 threshold, every frexp boundary, ties, negative components, divisions that round."""
    from cuda_pathtracer_amd import encode_hdr
    acc = K.accumulator()
    got = _gpu(acc, samples, mirror)
    assert got == encode_hdr(acc if mirror else np.ascontiguousarray(acc[:, ::-1]), samples)


def test_host_entry(gpu_device):
    from cuda_pathtracer_amd import encode_hdr, encode_hdr_device
    acc = K.noisy(50, 34)
    assert encode_hdr_device(acc, 7.0) == encode_hdr(acc, 7.0)
    assert encode_hdr_device(acc, 7.0, mirror_x=False) == encode_hdr(np.ascontiguousarray(acc[:, ::-1]), 7.0)


@pytest.fixture(scope="module")
def cornell_200(cornell_path, gpu_device):
    """A Cornell 200 x 200 context."""
    from cuda_pathtracer_amd import PathTracer, Scene
    s = Scene(cornell_path)
    s.set_camera((200, 200), 45.0, (0, 5, 10.5), (0, 5, 0), (0, 1, 0))
    s.finalize()
    pt = PathTracer(s)
    yield pt
    pt.free()


def test_cornell_three_routes(cornell_200, tmp_path):
    """1 spp (mostly black and noisy) and 16 spp through pt_hdr_enc_accum, pt_preview_hdr and PathTracer.save_hdr."""
    from cuda_pathtracer_amd import HdrEncoder, save_image_hdr
    pt = cornell_200
    enc = HdrEncoder(200, 200, _params())
    try:
        it = 0
        for spp in (1, 16):
            while it < spp:
                it += 1
                pt.render_pass(it)
            accum = pt.image()
            ref = open(save_image_hdr(str(tmp_path / f"host{spp}.hdr"), accum, float(spp)), "rb").read()
            assert enc.encode(accum, float(spp)) == ref                   # pt_hdr_enc_accum
            assert pt.preview_hdr(spp, enc) == ref                        # pt_preview_hdr
            got = open(pt.save_hdr(str(tmp_path / f"dev{spp}.hdr"), spp), "rb").read()
            assert got == ref
            dec = hdr_oracle.decode_hdr(got)
            want = (accum / np.float32(spp))[:, ::-1]
            assert (np.abs(dec - want) <= want.max(axis=2, keepdims=True) * 2 ** -7 + 1e-30).all()
    finally:
        enc.free()


def test_preview_hdr_refuses_another_size(cornell_200):
    from cuda_pathtracer_amd import HdrEncoder, PtError
    enc = HdrEncoder(200, 199)
    with pytest.raises(PtError):
        cornell_200.preview_hdr(1, enc)
    enc.free()


def test_reuse_one_object(gpu_device):
    """A long file, a short one, the long one again."""
    from cuda_pathtracer_amd import HdrEncoder, encode_hdr
    a, b = K.noisy(130, 40), np.full((40, 130, 3), 0.5, np.float32)
    enc = HdrEncoder(130, 40, _params())
    try:
        got = [enc.encode(im, 2.0) for im in (a, b, a)]
    finally:
        enc.free()
    ref = [encode_hdr(im, 2.0) for im in (a, b, a)]
    assert got == ref and len(ref[1]) < len(ref[0]) // 4


def test_non_default_stream_behind_a_pass(cornell_path, gpu_device):
    import torch
    from cuda_pathtracer_amd import HdrEncoder, PathTracer, Scene, encode_hdr
    s = Scene(cornell_path)
    s.set_camera((72, 40), 45.0, (0, 5, 10.5), (0, 5, 0), (0, 1, 0))
    s.finalize()
    pt = PathTracer(s)
    enc = HdrEncoder(72, 40, _params())
    st = torch.cuda.Stream()
    try:
        pt.render_pass(1, stream=st)
        got = pt.preview_hdr(1, enc, stream=st)   # queued behind the pass; the read waits for the stream
        accum = pt.image()
    finally:
        enc.free()
        pt.free()
    assert got == encode_hdr(accum, 1.0)


def test_overflow(gpu_device):
    """Three capacities: the negated size, the file's first cap bytes, and nothing at or behind out + cap."""
    import torch
    from cuda_pathtracer_amd import _native as N
    from cuda_pathtracer_amd import encode_hdr
    acc = K.noisy(65, 12)
    ref = encode_hdr(acc, 2.0)
    head = len(R.header(65, 12))
    L = N.lib()
    e = C.c_void_p()
    assert L.pt_hdr_enc_create(65, 12, C.byref(_params()), C.byref(e)) == 0
    src = torch.from_numpy(acc).cuda()
    out = torch.full((len(ref) + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    size = torch.zeros(1, dtype=torch.int64, device="cuda")
    two = C.c_float(2.0)
    try:
        for short in (0, head + 5, len(ref) - 1):
            out.fill_(0xA5)
            assert L.pt_hdr_enc_accum(e, src.data_ptr(), two, out.data_ptr(), short, size.data_ptr(), None) == 0
            torch.cuda.synchronize()
            assert int(size.cpu()[0]) == -len(ref)
            got = out.cpu().numpy()
            assert got[:short].tobytes() == ref[:short]
            assert (got[short:] == 0xA5).all()
        assert L.pt_hdr_enc_accum(e, src.data_ptr(), two, out.data_ptr(), len(ref), size.data_ptr(), None) == 0
        torch.cuda.synchronize()
        assert int(size.cpu()[0]) == len(ref)
        got = out.cpu().numpy()
        assert got[:len(ref)].tobytes() == ref and (got[len(ref):] == 0xA5).all()
    finally:
        L.pt_hdr_enc_destroy(e)
    # flat rows take the other path to the file
    flat = K.noisy(5, 4)
    fref = encode_hdr(flat, 2.0)
    assert L.pt_hdr_enc_create(5, 4, C.byref(_params()), C.byref(e)) == 0
    src = torch.from_numpy(flat).cuda()
    try:
        short = len(fref) - 3
        out.fill_(0xA5)
        assert L.pt_hdr_enc_accum(e, src.data_ptr(), two, out.data_ptr(), short, size.data_ptr(), None) == 0
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert int(size.cpu()[0]) == -len(fref) and got[:short].tobytes() == fref[:short] and (got[short:] == 0xA5).all()
    finally:
        L.pt_hdr_enc_destroy(e)
    hout, n = np.zeros(len(ref), np.uint8), C.c_int64(0)
    rc = L.pt_hdr_encode_host(65, 12, acc.ctypes.data, two, C.byref(_params()), hout.ctypes.data, len(ref) - 1, C.byref(n))
    assert rc == 1 and n.value == len(ref)   # PT_ERR_ARG and the size needed


def test_profile(gpu_device):
    from cuda_pathtracer_amd import HdrEncoder, encode_hdr
    from cuda_pathtracer_amd import _native as N
    acc = K.noisy(64, 48)
    enc = HdrEncoder(64, 48, _params())
    try:
        assert N.lib().pt_hdr_enc_profile(enc._h, 1) == 0
        data = enc.encode(acc, 1.0)
        ms = (C.c_float * 4)()
        assert N.lib().pt_hdr_enc_profile_read(enc._h, ms) == 0
    finally:
        enc.free()
    assert data == encode_hdr(acc, 1.0) and all(np.isfinite(v) and 0.0 <= v < 1e3 for v in ms)


def test_cli_device_hdr(cornell_path, gpu_device, tmp_path):
    """--hdr --device-hdr: the same file name and the same bytes as --hdr."""
    import subprocess
    from cuda_pathtracer_amd import build
    outs = []
    for flags in ([], ["--device-hdr"]):
        d = tmp_path / ("dev" if flags else "host")
        d.mkdir()
        subprocess.run([str(build.CLI), cornell_path, "--iterations", "2", "--out", str(d), "--no-png", "--hdr", *flags],
                       check=True, capture_output=True, timeout=120)
        files = sorted(d.glob("*.hdr"))
        assert len(files) == 1 and files[0].name.endswith(".2samp.hdr")
        outs.append(files[0].read_bytes())
    assert outs[0] == outs[1] and outs[0].startswith(b"#?RADIANCE\n")


def test_preview_server_frame_hdr(cornell_path, gpu_device, tmp_path):
    """/frame.hdr decodes to the session's accumulator within RGBE's quantisation, 2^-7 of each pixel's largest
    component, and is the host writer's file of it."""
    from cuda_pathtracer_amd import Scene, encode_hdr
    from cuda_pathtracer_amd import preview as V
    s = Scene(cornell_path)
    s.set_camera((64, 64), 45.0, (0, 5, 10.5), (0, 5, 0), (0, 1, 0))
    st = s.state()
    s.set_render(8, st.traceDepth, st.imageName)
    s.finalize()
    ses = V.PreviewSession(s, out_dir=str(tmp_path))
    srv = V.PreviewServer(ses).start(render=False)   # (the test drives the render loop: no waiting)
    try:
        with pytest.raises(urllib.error.HTTPError) as err:   # nothing accumulated yet
            urllib.request.urlopen(srv.url + "frame.hdr", timeout=10)
        assert err.value.code == 404
        ses.run_cuda()
        ses.run_cuda()
        with urllib.request.urlopen(srv.url + "frame.hdr", timeout=10) as r:
            assert r.headers["Content-Type"] == "image/vnd.radiance"
            data = r.read()
        accum, it = ses.ctx.image(), ses.iteration
        assert it == 2 and data == encode_hdr(accum, float(it))
        dec = hdr_oracle.decode_hdr(data)
        want = (accum / np.float32(it))[:, ::-1]
        assert (np.abs(dec - want) <= want.max(axis=2, keepdims=True) * 2 ** -7 + 1e-30).all()
        assert ses._hdr_enc is not None and ses._png_enc is None
    finally:
        srv.stop()
        ses.close()
