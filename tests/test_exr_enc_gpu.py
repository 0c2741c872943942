"""The device OpenEXR encoder (csrc/pt_exr_enc.hip) against its restatement (tests/exr_ref.py): the
kernels' file must equal the restatement's byte for byte, and the independent reader must get the source values back."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import exr_cases as K
from tests import exr_ref as R

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (3, 1), (7, 5), (64, 1), (65, 17), (257, 33), (700, 500)]
COMPRESSIONS = [R.NONE, R.ZIPS, R.ZIP]


def _params(comp=R.ZIP, mirror=False, block_bytes=None):
    from cuda_pathtracer_amd import ExrParams
    p = ExrParams.default()
    p.compression, p.mirror_x = comp, int(mirror)
    if block_bytes is not None:
        p.block_bytes = block_bytes
    return p


def _gpu(chans, comp=R.ZIP, mirror=False, block_bytes=None):
    from cuda_pathtracer_amd import ExrEncoder
    h, w = np.asarray(chans[0][2]).shape
    enc = ExrEncoder(w, h, [(n, t) for n, t, _, _ in chans], _params(comp, mirror, block_bytes))
    try:
        return enc.encode([p for _, _, p, _ in chans], divisors=[d for _, _, _, d in chans])
    finally:
        enc.free()


@functools.lru_cache(maxsize=None)
def _case(w, h, count):
    return K.channel_set(count, w, h, seed=w + h)


@pytest.mark.parametrize("comp", COMPRESSIONS)
@pytest.mark.parametrize("count", [1, 3, 16])
@pytest.mark.parametrize("w,h", SIZES)
def test_sizes_compressions_and_channel_sets(gpu_device, w, h, count, comp):
    """(65, 17): two ZIP chunks, the last of one line, rows that are no multiple of a lane's 4 pixels.  (700, 500) with
    the three FLOAT channels: ZIP chunks of 134400 bytes, 5 deflate blocks (the last partial) and 263 lane chunks; with
    ZIPS 500 streams; with the 16 channels ZIP streams of 537600 bytes, 1050 lane chunks: two tiles of the stream's scan."""
    chans = _case(w, h, count)
    ref = R.encode(chans, comp)
    if (w, h, count, comp) == (700, 500, 3, R.ZIP):
        assert ref.n[0] == 134400 and len(ref.block_types[0]) == 5 and -(-ref.n[0] // R.CHUNK) == 263
    if (w, h, count, comp) == (700, 500, 16, R.ZIP):
        assert -(-ref.n[0] // R.CHUNK) > 1024
    got = _gpu(chans, comp)
    assert len(got) == len(ref.data) and got == ref.data


@pytest.mark.parametrize("divisor", [1.0, 3.0])
def test_half_conversion_plane(gpu_device, divisor):
    """Every finite half's neighbourhood, ties, the overflow's edge, denormals, infinities and NaNs as one HALF channel; with
    the divisor 3 the division comes first, as in the restatement."""
    chans = [("Y", R.HALF, K.half_plane(), divisor)]
    ref = R.encode(chans, R.ZIP)
    got = _gpu(chans, R.ZIP)
    assert got == ref.data
    want = R.half_bits(R.value_bytes(K.half_plane(), R.FLOAT, divisor).view(np.uint32))   # the division first
    assert (R.read_exr(got)["Y"].view(np.uint16) == want).all()


@pytest.mark.parametrize("comp", [R.ZIPS, R.ZIP])
def test_noise_and_constant_image(gpu_device, comp):
    chans = K.noise_and_constant()
    ref = R.encode(chans, comp)
    got = _gpu(chans, comp)
    assert got == ref.data
    info = {}
    dec = R.read_exr(got, info)
    assert any(info["raw"]) and not all(info["raw"])   # the file holds raw chunks and compressed ones
    for name, _, plane, _ in chans:
        assert (dec[name].view(np.uint32) == plane.view(np.uint32)).all()


@pytest.mark.parametrize("comp", COMPRESSIONS)
def test_mirror_x_and_small_blocks(gpu_device, comp):
    chans = _case(65, 17, 16)
    assert _gpu(chans, comp, mirror=True, block_bytes=1024) == R.encode(chans, comp, block_bytes=1024, mirror_x=True).data


@pytest.mark.parametrize("comp", [R.NONE, R.ZIP])
def test_strides_offsets_aliases_and_uint(gpu_device, comp):
    """Planes interleaved 3 and 4 floats apart and a plain one, given as device pointers: channel pointers one float past an
    aligned address, two channels reading the same plane, and a UINT channel with 0xffffffff in it."""
    import torch
    from cuda_pathtracer_amd import ExrEncoder
    w, h = 67, 19
    rng = np.random.default_rng(5)
    rgb = K.mixed(3 * w, h, 1).reshape(h, w, 3)
    four = K.mixed(4 * w, h, 2).reshape(h, w, 4).copy()
    four.view(np.uint32)[..., 3] = rng.integers(0, 3, (h, w), dtype=np.uint32) * np.uint32(0xffffffff)
    plain = np.concatenate([np.zeros(1, np.float32), K.mixed(w, h, 3).reshape(-1)])   # the plane starts one float in
    d_rgb, d_four, d_plain = (torch.from_numpy(a).cuda() for a in (rgb, four, plain))
    names = [("R", R.FLOAT), ("G", R.HALF), ("B", R.FLOAT), ("N.X", R.HALF), ("id", R.UINT), ("Y", R.FLOAT), ("Y2", R.HALF),
             ("Y3", R.FLOAT)]
    ptrs = [d_rgb.data_ptr(), d_rgb.data_ptr() + 4, d_rgb.data_ptr() + 8, d_four.data_ptr() + 4, d_four.data_ptr() + 12,
            d_plain.data_ptr() + 4, d_plain.data_ptr() + 4, d_four.data_ptr()]
    strides = [3, 3, 3, 4, 4, 1, 1, 4]
    divisors = [1.0, 2.0, 1.0, 1.0, 7.0, 1.0, 3.0, 1.0]
    planes = [rgb[..., 0], rgb[..., 1], rgb[..., 2], four[..., 1], four[..., 3], plain[1:].reshape(h, w), plain[1:].reshape(h, w),
              four[..., 0]]
    enc = ExrEncoder(w, h, names, _params(comp))
    try:
        got = enc.encode(ptrs, strides=strides, divisors=divisors)
    finally:
        enc.free()
    ref = R.encode([(n, t, np.ascontiguousarray(p), d) for (n, t), p, d in zip(names, planes, divisors)], comp)
    assert got == ref.data
    dec = R.read_exr(got)
    assert (dec["id"] == four.view(np.uint32)[..., 3]).all() and (dec["id"] == 0xffffffff).any()   # the divisor 7 is ignored
    assert (dec["Y"] == plain[1:].reshape(h, w)).all()


def test_reuse_one_object(gpu_device):
    """Data that compresses, data that does not, the first again: the same bytes as at first (no stale scratch)."""
    from cuda_pathtracer_amd import ExrEncoder
    w, h = 130, 40
    a = [("R", R.FLOAT, K.smooth(w, h), 1.0), ("G", R.HALF, K.mixed(w, h, 1), 1.0)]
    b = [("R", R.FLOAT, K.noise(w, h, 2), 1.0), ("G", R.HALF, K.noise(w, h, 3), 1.0)]
    enc = ExrEncoder(w, h, [("R", R.FLOAT), ("G", R.HALF)], _params(R.ZIP))
    try:
        got = [enc.encode([c[0][2], c[1][2]]) for c in (a, b, a)]
    finally:
        enc.free()
    ref = [R.encode(c, R.ZIP).data for c in (a, b, a)]
    assert got == ref and len(ref[0]) < len(ref[1]) // 2


def test_non_default_stream_behind_a_pass(cornell_path, gpu_device):
    import torch
    from cuda_pathtracer_amd import EXR_BEAUTY, ExrEncoder, PathTracer, Scene, exr_ctx_channels
    s = Scene(cornell_path)
    s.set_camera((72, 40), 45.0, (0, 5, 10.5), (0, 5, 0), (0, 1, 0))
    s.finalize()
    pt = PathTracer(s)
    enc = ExrEncoder(72, 40, exr_ctx_channels(EXR_BEAUTY), _params(R.ZIP))
    st = torch.cuda.Stream()
    try:
        pt.render_pass(1, stream=st)
        got = pt.preview_exr(1, enc, EXR_BEAUTY, stream=st)   # queued behind the pass; the read waits for the stream
        accum = pt.image()
    finally:
        enc.free()
        pt.free()
    ref = R.encode([(n, R.FLOAT, np.ascontiguousarray(accum[..., k]), 1.0) for k, n in enumerate("RGB")], R.ZIP)
    assert got == ref.data


@pytest.mark.parametrize("comp", COMPRESSIONS)
def test_overflow(gpu_device, comp):
    """Three capacities, 0, inside the offset table and inside the last chunk: the negated size, the file's first cap bytes,
    and nothing at or behind out + cap."""
    import torch
    from cuda_pathtracer_amd import _native as N
    chans = K.noise_and_constant(65, 64)
    ref = R.encode(chans, comp).data
    head = len(R.header(65, 64, [(n, t) for n, t, _, _ in chans], comp))
    L = N.lib()
    e = C.c_void_p()
    arr = (N.ExrChannel * 3)(*[N.ExrChannel(n, t) for n, t, _, _ in chans])
    assert L.pt_exr_enc_create(65, 64, arr, 3, C.byref(_params(comp)), C.byref(e)) == 0
    src = [torch.from_numpy(p).cuda() for _, _, p, _ in chans]
    planes = (N.ExrPlane * 3)(*[N.ExrPlane(t.data_ptr(), 1, 1.0) for t in src])
    out = torch.full((len(ref) + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    size = torch.zeros(1, dtype=torch.int64, device="cuda")
    try:
        for short in (0, head + 13, len(ref) - 5):
            out.fill_(0xA5)
            assert L.pt_exr_enc_planes(e, planes, out.data_ptr(), short, size.data_ptr(), None) == 0
            torch.cuda.synchronize()
            assert int(size.cpu()[0]) == -len(ref)
            got = out.cpu().numpy()
            assert got[:short].tobytes() == ref[:short]
            assert (got[short:] == 0xA5).all()
        assert L.pt_exr_enc_planes(e, planes, out.data_ptr(), len(ref), size.data_ptr(), None) == 0
        torch.cuda.synchronize()
        assert int(size.cpu()[0]) == len(ref)
        got = out.cpu().numpy()
        assert got[:len(ref)].tobytes() == ref and (got[len(ref):] == 0xA5).all()
    finally:
        L.pt_exr_enc_destroy(e)
    hout, n = np.zeros(len(ref), np.uint8), C.c_int64(0)
    ptrs = (C.c_void_p * 3)(*[p.ctypes.data for _, _, p, _ in chans])
    rc = L.pt_exr_encode_host(65, 64, arr, 3, ptrs, None, None, C.byref(_params(comp)), hout.ctypes.data, len(ref) - 1, C.byref(n))
    assert rc == 1 and n.value == len(ref)   # PT_ERR_ARG and the size needed


def test_host_entry_and_profile(gpu_device):
    from cuda_pathtracer_amd import ExrEncoder, encode_exr
    from cuda_pathtracer_amd import _native as N
    w, h = 64, 48
    y, ident = K.mixed(w, h, 4), np.arange(w * h, dtype=np.uint32).reshape(h, w)
    got = encode_exr({"Y": y, "A": y, "id": ident}, half=("A",), compression="zips", mirror_x=True)
    ref = R.encode([("Y", R.FLOAT, y, 1.0), ("A", R.HALF, y, 1.0), ("id", R.UINT, ident.view(np.float32), 1.0)], R.ZIPS, mirror_x=True)
    assert got == ref.data
    enc = ExrEncoder(w, h, [("Y", R.FLOAT)], _params(R.ZIP))
    try:
        assert N.lib().pt_exr_enc_profile(enc._h, 1) == 0
        data = enc.encode([y])
        ms = (C.c_float * 6)()
        assert N.lib().pt_exr_enc_profile_read(enc._h, ms) == 0
        assert enc.header() == R.header(w, h, [("Y", R.FLOAT)], R.ZIP) and enc.bound == R.bound(w, h, [("Y", R.FLOAT)], R.ZIP)
    finally:
        enc.free()
    assert data == R.encode([("Y", R.FLOAT, y, 1.0)], R.ZIP).data and all(np.isfinite(v) and 0.0 <= v < 1e3 for v in ms)


@pytest.fixture(scope="module")
def cornell_64(cornell_path, gpu_device):
    """A Cornell 64 x 64 context with 4 samples per pixel."""
    from cuda_pathtracer_amd import PathTracer, Scene
    s = Scene(cornell_path)
    s.set_camera((64, 64), 45.0, (0, 5, 10.5), (0, 5, 0), (0, 1, 0))
    s.finalize()
    pt = PathTracer(s)
    for it in range(1, 5):
        pt.render_pass(it)
    yield pt
    pt.free()


def _layers_expected(pt, mirror=False):
    img, g = pt.image() / np.float32(4), pt.gbuffer()
    want = {"R": img[..., 0], "G": img[..., 1], "B": img[..., 2], "Z": g["t"], "id": g["mat"].view(np.uint32),
            "UV.U": g["uv"][..., 0], "UV.V": g["uv"][..., 1]}
    for k, c in enumerate("RGB"):
        want["albedo." + c] = g["albedo"][..., k]
    for k, c in enumerate("XYZ"):
        want["N." + c] = g["normal"][..., k]
        want["P." + c] = g["position"][..., k]
    return {n: np.ascontiguousarray(a[:, ::-1] if mirror else a) for n, a in want.items()}


def _check_layers(dec, want, chans):
    assert sorted(dec) == sorted(n for n, _ in chans)
    for n, t in chans:
        if t == R.HALF:
            assert dec[n].dtype == np.float16 and (dec[n].view(np.uint16) == R.half_bits(want[n].view(np.uint32))).all(), n
        else:
            assert dec[n].dtype.itemsize == 4 and (dec[n].view(np.uint32) == want[n].view(np.uint32)).all(), n


@pytest.mark.parametrize("half", [0, 127])
def test_through_the_context(cornell_64, half, tmp_path):
    """Every layer through pt_preview_exr, read back by the independent reader and compared with == against image() / 4 and
    gbuffer(); HALF layers against half_bits of them; save_exr is mirrored."""
    from cuda_pathtracer_amd import EXR_ALL_LAYERS, EXR_BEAUTY, ExrEncoder, exr_ctx_channels
    pt = cornell_64
    chans = exr_ctx_channels(EXR_ALL_LAYERS, half)
    want = _layers_expected(pt)
    enc = ExrEncoder(64, 64, chans, _params(R.ZIP))
    try:
        got = pt.preview_exr(4, enc, EXR_ALL_LAYERS)
        again = pt.preview_exr(4, enc, EXR_ALL_LAYERS)
    finally:
        enc.free()
    assert got == again
    _check_layers(R.read_exr(got), want, chans)
    assert got == R.encode([(n, t, want[n].view(np.float32), 1.0) for n, t in chans], R.ZIP).data
    # a beauty-only file, and the saved one
    enc = ExrEncoder(64, 64, exr_ctx_channels(EXR_BEAUTY, half), _params(R.ZIPS))
    try:
        _check_layers(R.read_exr(pt.preview_exr(4, enc)), want, exr_ctx_channels(EXR_BEAUTY, half))
    finally:
        enc.free()
    path = pt.save_exr(str(tmp_path / "all.exr"), 4, EXR_ALL_LAYERS, half)
    _check_layers(R.read_exr(open(path, "rb").read()), _layers_expected(pt, mirror=True), chans)


def test_refusals(cornell_64, cornell_path):
    from cuda_pathtracer_amd import (EXR_ALBEDO, EXR_BEAUTY, EXR_FLOAT, EXR_NORMAL, ExrEncoder, PathTracer, PtError, Scene,
                                     exr_ctx_channels)
    pt = cornell_64
    cases = [(ExrEncoder(64, 63, exr_ctx_channels(EXR_BEAUTY)), EXR_BEAUTY),                    # another size
             (ExrEncoder(64, 64, exr_ctx_channels(EXR_BEAUTY)), EXR_BEAUTY | EXR_ALBEDO),        # fewer channels than the layers
             (ExrEncoder(64, 64, exr_ctx_channels(EXR_NORMAL)), EXR_ALBEDO),                     # another layer's
             (ExrEncoder(64, 64, [("G", EXR_FLOAT), ("R", EXR_FLOAT), ("B", EXR_FLOAT)]), EXR_BEAUTY),   # another order
             (ExrEncoder(64, 64, [("R", 1), ("G", 2), ("B", 1)]), EXR_BEAUTY),                   # a layer half HALF
             (ExrEncoder(64, 64, exr_ctx_channels(EXR_BEAUTY)), 0)]
    for enc, layers in cases:
        with pytest.raises(PtError):
            pt.preview_exr(4, enc, layers)
        enc.free()
    s = Scene(cornell_path)
    s.set_camera((64, 64), 45.0, (0, 5, 10.5), (0, 5, 0), (0, 1, 0))
    s.finalize()
    tile = PathTracer(s, rank=0, world=2)
    enc = ExrEncoder(64, tile.rows, exr_ctx_channels(EXR_BEAUTY))
    try:
        with pytest.raises(PtError):
            tile.preview_exr(1, enc)
    finally:
        enc.free()
        tile.free()


def test_cli(cornell_path, gpu_device, tmp_path):
    """--exr and --exr --exr-half --aov DIR; the PNG and the .f32 files of the same run equal those of a run without --exr."""
    import subprocess
    from cuda_pathtracer_amd import build
    runs = {"plain": [], "exr": ["--exr"], "all": ["--exr", "--exr-half"]}
    files = {}
    for name, flags in runs.items():
        d = tmp_path / name
        d.mkdir()
        subprocess.run([str(build.CLI), cornell_path, "--iterations", "2", "--out", str(d), "--aov", str(d), *flags],
                       check=True, capture_output=True, timeout=120)
        files[name] = {("png" if p.suffix == ".png" else p.name): p.read_bytes() for p in d.iterdir() if p.suffix != ".exr"}
        exr = sorted(d.glob("*.exr"))
        assert len(exr) == (1 if flags else 0)
        if flags:
            assert exr[0].name.endswith(".2samp.exr")
            files[name + ".exr"] = exr[0].read_bytes()
    assert files["plain"] == files["exr"] == files["all"] and len(files["plain"]) == 6   # png, 4 planes, the JSON
    shape = None
    for name, nhalf in (("exr", 0), ("all", 11)):
        dec = R.read_exr(files[name + ".exr"])
        assert len(dec) == 16 and sum(a.dtype == np.float16 for a in dec.values()) == nhalf
        shape = dec["R"].shape
    # the planes of the .f32 files, mirrored, are the layers
    ga = np.frombuffer(next(v for k, v in files["plain"].items() if k.endswith(".gA.f32")), np.float32).reshape(shape + (4,))
    dec = R.read_exr(files["exr.exr"])
    assert (dec["N.X"] == ga[:, ::-1, 0]).all() and (dec["id"] == ga.view(np.uint32)[:, ::-1, 3]).all()
    d = tmp_path / "beauty"
    d.mkdir()
    subprocess.run([str(build.CLI), cornell_path, "--iterations", "2", "--out", str(d), "--exr"], check=True, capture_output=True,
                   timeout=120)
    dec = R.read_exr(next(d.glob("*.exr")).read_bytes())
    assert sorted(dec) == ["B", "G", "R"] and dec["R"].dtype == np.float32
    assert (dec["R"] == R.read_exr(files["exr.exr"])["R"]).all()
