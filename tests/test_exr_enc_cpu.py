"""The OpenEXR encoder's definition without a device: the restatement (tests/exr_ref.py) against its own
independent reader and against zlib, the crafted cases (tests/exr_cases.py) reach what they are for, and the host side of
pt_exr_enc (header, bound, context channels, argument errors).

Total chunk payload against zlib's run-length coder, zlib.compressobj(6, DEFLATED, 15, 8, Z_RLE), over the same p with the
same raw-fallback rule, golden Cornell 800 x 800 / 255 as R, G, B, ZIP (50 chunks, none raw): FLOAT 4016203 / 3957553 =
1.0148, HALF 1416119 / 1387562 = 1.0206; asserted at the next 0.01, 1.02 and 1.03."""
import ctypes as C
import zlib

import numpy as np
import pytest

from tests import exr_cases as K
from tests import exr_ref as R

SIZES = [(1, 1), (3, 1), (7, 5), (65, 17), (64, 48)]
COMPRESSIONS = [R.NONE, R.ZIPS, R.ZIP]


def expected(chans, mirror_x=False):
    """What a reader must return: the value bytes of the definition, as arrays."""
    out = {}
    for name, typ, plane, div in chans:
        plane = np.asarray(plane)[:, ::-1] if mirror_x else np.asarray(plane)
        b = R.value_bytes(plane, typ, div)
        out[name] = b.view({R.UINT: np.uint32, R.HALF: np.uint16, R.FLOAT: np.uint32}[typ])
    return out


def same_values(got: dict, want: dict):
    assert sorted(got) == sorted(want)
    for name in want:
        g = got[name].view(np.uint16 if got[name].dtype.itemsize == 2 else np.uint32)
        assert g.shape == want[name].shape and (g == want[name]).all(), name


def test_half_bits_is_the_ieee_conversion():
    v = K.half_values()
    assert 380000 < v.size < 420000
    bits = v.view(np.uint32)
    got = R.half_bits(bits)
    nan = np.isnan(v)
    assert nan.sum() == 8
    with np.errstate(over="ignore"):
        want = v.astype(np.float16).view(np.uint16)
    assert (got[~nan] == want[~nan]).all()
    assert (got[nan] == (((bits[nan] >> 16) & 0x8000) | 0x7e00)).all()
    # what the cases are for: subnormal halves, ties both ways, the overflow's edge, float denormals
    assert ((got & 0x7c00) == 0).sum() > 4000 and (got == 0x7c00).any() and (got == 0xfc00).any()
    assert R.half_bits(np.array([0x477fefff, 0x477ff000, 0x33000000, 0x33000001, 1], np.uint32)).tolist() == [0x7bff, 0x7c00, 0, 1, 0]
    plane = K.half_plane()
    assert plane.shape[1] == K.HALF_PLANE_W and plane.size >= v.size and (plane.reshape(-1)[:v.size].view(np.uint32) == bits).all()


@pytest.mark.parametrize("comp", COMPRESSIONS)
@pytest.mark.parametrize("count", [1, 3, 16])
@pytest.mark.parametrize("w,h", SIZES)
def test_round_trip_and_the_two_restatements(w, h, count, comp):
    chans = K.channel_set(count, w, h, seed=w + h)
    enc = R.encode(chans, comp, block_bytes=1024)
    assert enc.data == R.encode(chans, comp, block_bytes=1024, slow=True).data
    info = {}
    same_values(R.read_exr(enc.data, info), expected(chans))
    assert info["raw"] == enc.raw and info["attrs"]["compression"][1][0] == comp
    assert len(enc.data) <= R.bound(w, h, [(n, t) for n, t, _, _ in chans], comp)
    for k, raw in enumerate(enc.raw):
        if comp == R.NONE or raw:
            continue
        assert zlib.decompress(enc.payload[k]) == enc.p[k]                       # zlib inflates the stream to p
        assert enc.payload[k][-4:] == zlib.adler32(enc.p[k]).to_bytes(4, "big")  # and its checksum is zlib's
        assert enc.payload[k][:2] == b"\x78\x01" and len(enc.payload[k]) == enc.z[k] < enc.n[k]


def test_mirror_and_divisor_round_trip():
    chans = [(n, t, p, 3.0) for n, t, p, _ in K.channel_set(3, 13, 4)]
    enc = R.encode(chans, R.ZIP, mirror_x=True)
    same_values(R.read_exr(enc.data), expected(chans, mirror_x=True))
    a = np.array([[1.0, 2.0, 5.0]], np.float32)
    got = R.read_exr(R.encode([("Y", R.FLOAT, a, 3.0)], R.NONE, mirror_x=True).data)["Y"]
    assert (got == (a / np.float32(3))[:, ::-1]).all()


def test_noise_and_constant_image_holds_both_kinds_of_chunk():
    chans = K.noise_and_constant()
    for comp in (R.ZIP, R.ZIPS):
        enc = R.encode(chans, comp)
        assert any(enc.raw) and not all(enc.raw)
        assert enc.raw[0] and not enc.raw[-1]
        same_values(R.read_exr(enc.data), expected(chans))
        # the issue's measurement: noise as FLOAT does not compress; the streams are longer than the raw bytes
        assert all(z >= n for z, n, raw in zip(enc.z, enc.n, enc.raw) if raw)


def test_fallback_rule_at_the_boundary():
    n = 4096
    assert [R.raw_fallback(z, n) for z in (n - 1, n, n + 1)] == [False, True, True]


def test_smallest_and_odd_streams():
    # 1 x 1, one HALF channel: n = 2, one even and one odd byte; p[0] = t[0]
    enc = R.encode([("Y", R.HALF, np.array([[1.5]], np.float32), 1.0)], R.ZIP)
    assert enc.n == [2] and enc.p[0] == bytes([0x00, (0x3e - 0x00 + 128) & 255]) and enc.raw == [True]
    assert R.read_exr(enc.data)["Y"].view(np.uint16).tolist() == [[0x3e00]]
    # every value has 2 or 4 bytes, so no chunk has an odd number of bytes (n = 1 among them), and the split's
    # (n + 1) / 2 is n / 2: the even and the odd half are equally long
    sizes = K.stream_sizes()
    assert 2 in sizes and 6 in sizes and 1 not in sizes and all(n % 2 == 0 and (n + 1) // 2 == n // 2 for n in sizes)
    # W = 1, ZIPS, one HALF and one FLOAT channel: n = 6
    chans = [("a", R.HALF, np.array([[2.0], [-2.0]], np.float32), 1.0), ("b", R.FLOAT, np.array([[1.0], [3.0]], np.float32), 1.0)]
    enc = R.encode(chans, R.ZIPS)
    assert enc.n == [6, 6]
    r = bytes([0x00, 0x40, 0x00, 0x00, 0x80, 0x3f])
    t = bytes([r[0], r[2], r[4], r[1], r[3], r[5]])
    assert enc.p[0] == bytes([t[0]] + [(t[i] - t[i - 1] + 128) & 255 for i in range(1, 6)])
    assert R.unpreprocess(R.preprocess(r)) == r
    same_values(R.read_exr(enc.data), expected(chans))
    # what the split would do with an odd n, though no file has one: the even half gets the byte more
    assert R.unpreprocess(R.preprocess(b"\x01\x02\x03")) == b"\x01\x02\x03" and R.preprocess(b"\x01\x02\x03")[1] == (3 - 1 + 128)


# ---- the library's host side ----------------------------------------------------------------------------
def _lib():
    from cuda_pathtracer_amd import _native as N
    return N, N.lib()


def _create(w, h, chans, comp=R.ZIP, block_bytes=None, mirror=0, reserved=None):
    N, L = _lib()
    prm = N.ExrParams.default()
    prm.compression, prm.mirror_x = comp, mirror
    if block_bytes is not None:
        prm.block_bytes = block_bytes
    if reserved is not None:
        prm.reserved[reserved] = 1
    arr = (N.ExrChannel * max(len(chans), 1))(*[N.ExrChannel(n, t) for n, t in chans])
    e = C.c_void_p()
    rc = L.pt_exr_enc_create(w, h, arr, len(chans), C.byref(prm), C.byref(e))
    return rc, e


@pytest.mark.parametrize("comp", COMPRESSIONS)
@pytest.mark.parametrize("count", [1, 3, 16])
def test_header_and_bound(count, comp):
    N, L = _lib()
    for w, h in SIZES + [(700, 500)]:
        chans = [(n, t) for n, t, _, _ in K.channel_set(count, 1, 1)]
        rc, e = _create(w, h, chans, comp)
        assert rc == 0
        want = R.header(w, h, chans, comp)
        n = L.pt_exr_enc_header(e, None, 0)
        buf = (C.c_uint8 * n)()
        assert L.pt_exr_enc_header(e, buf, n) == n and bytes(buf) == want
        chunks = -(-h // R.LINES[comp])
        line = w * sum(2 if t == R.HALF else 4 for _, t in chans)
        assert L.pt_exr_enc_bound(e) == len(want) + 8 * chunks + chunks * 8 + h * line == R.bound(w, h, chans, comp)
        assert L.pt_exr_enc_destroy(e) == 0
    defaults = N.ExrParams.default()
    assert (defaults.compression, defaults.block_bytes, defaults.mirror_x) == (R.ZIP, 32768, 0)


def test_ctx_channels():
    import cuda_pathtracer_amd as P
    table = [(P.EXR_BEAUTY, ["R", "G", "B"], True), (P.EXR_ALBEDO, ["albedo.R", "albedo.G", "albedo.B"], True),
             (P.EXR_NORMAL, ["N.X", "N.Y", "N.Z"], True), (P.EXR_POSITION, ["P.X", "P.Y", "P.Z"], False),
             (P.EXR_DEPTH, ["Z"], False), (P.EXR_UV, ["UV.U", "UV.V"], True), (P.EXR_ID, ["id"], False)]
    for bit, names, halfable in table:
        base = P.EXR_UINT if bit == P.EXR_ID else P.EXR_FLOAT
        assert P.exr_ctx_channels(bit, 0) == [(n, base) for n in names]
        assert P.exr_ctx_channels(bit, P.EXR_ALL_LAYERS) == [(n, P.EXR_HALF if halfable else base) for n in names]
    every = P.exr_ctx_channels(P.EXR_ALL_LAYERS, P.EXR_NORMAL)
    assert [n for n, _ in every] == sum((names for _, names, _ in table), []) and len(every) == 16
    assert [t for n, t in every if n.startswith("N.")] == [P.EXR_HALF] * 3 and sum(t == P.EXR_HALF for _, t in every) == 3
    N, L = _lib()
    out, n = (N.ExrChannel * 16)(), C.c_int32(0)
    assert L.pt_exr_ctx_channels(0, 0, out, C.byref(n)) == 1 and L.pt_exr_ctx_channels(128, 0, out, C.byref(n)) == 1
    assert L.pt_exr_ctx_channels(1, 0, None, C.byref(n)) == 1 and L.pt_exr_ctx_channels(1, 0, out, None) == 1


def test_argument_errors_need_no_device():
    N, L = _lib()
    ok = [("R", R.FLOAT)]
    bad = [
        dict(chans=[]),                                                   # 0 channels
        dict(chans=[(f"c{k}", R.FLOAT) for k in range(17)]),              # 17
        dict(chans=[("", R.FLOAT)]),                                      # an empty name
        dict(chans=[("x" * 32, R.FLOAT)]),                                # 32 bytes: no room for the end
        dict(chans=[("R", R.FLOAT), ("G", R.HALF), ("R", R.HALF)]),       # a duplicate
        dict(chans=[("a b", R.FLOAT)]), dict(chans=[("a-b", R.FLOAT)]), dict(chans=[("é", R.FLOAT)]),
        dict(chans=[("R", 3)]), dict(chans=[("R", -1)]),                  # a bad type
        dict(chans=ok, comp=1), dict(chans=ok, comp=4), dict(chans=ok, comp=-1),
        dict(chans=ok, block_bytes=512), dict(chans=ok, block_bytes=1025), dict(chans=ok, block_bytes=1536 + 256),
        dict(chans=ok, block_bytes=(1 << 20) + 512),
        dict(chans=ok, reserved=0), dict(chans=ok, reserved=4),
    ]
    for kw in bad:
        rc, _ = _create(8, 8, **kw)
        assert rc == 1, kw
    assert _create(0, 8, ok)[0] == 1 and _create(8, -1, ok)[0] == 1
    # the bound must stay below 2^31: 3 FLOAT channels of 13400^2 pixels are 2.15e9 bytes, of 13300^2 2.12e9
    rgb = [("R", R.FLOAT), ("G", R.FLOAT), ("B", R.FLOAT)]
    assert _create(13400, 13400, rgb)[0] == 1 and _create(65535, 65535, rgb)[0] == 1
    rc, e = _create(13300, 13300, rgb)
    assert rc == 0 and L.pt_exr_enc_bound(e) == R.bound(13300, 13300, rgb, R.ZIP) < 2 ** 31 and L.pt_exr_enc_destroy(e) == 0
    # and so must a stream's bit offsets: 16 lines of 14.9 million HALF pixels are 4.8e8 bytes, 9 bits each
    assert _create(14_900_000, 16, [("Y", R.HALF)], R.ZIP)[0] == 1
    rc, e = _create(14_900_000, 16, [("Y", R.HALF)], R.ZIPS)
    assert rc == 0 and L.pt_exr_enc_destroy(e) == 0
    rc, e = _create(14_900_000, 16, [("Y", R.HALF)], R.NONE)
    assert rc == 0 and L.pt_exr_enc_destroy(e) == 0
    # null pointers
    prm = N.ExrParams.default()
    ch = (N.ExrChannel * 1)(N.ExrChannel("R", R.FLOAT))
    e = C.c_void_p()
    assert L.pt_exr_enc_create(8, 8, None, 1, C.byref(prm), C.byref(e)) == 1
    assert L.pt_exr_enc_create(8, 8, ch, 1, None, C.byref(e)) == 1
    assert L.pt_exr_enc_create(8, 8, ch, 1, C.byref(prm), None) == 1
    assert L.pt_exr_enc_bound(None) == 0 and L.pt_exr_enc_destroy(None) == 0 and L.pt_exr_enc_header(None, None, 0) == 0
    # a created object checks an encode's arguments before it touches a device
    rc, e = _create(8, 8, ok)
    assert rc == 0
    pl = (N.ExrPlane * 1)(N.ExrPlane(16, 1, 1.0))
    assert L.pt_exr_enc_planes(e, None, 16, 64, 16, None) == 1 and L.pt_exr_enc_planes(e, pl, None, 64, 16, None) == 1
    assert L.pt_exr_enc_planes(e, pl, 16, -1, 16, None) == 1 and L.pt_exr_enc_planes(e, pl, 16, 64, None, None) == 1
    for plane in (N.ExrPlane(None, 1, 1.0), N.ExrPlane(16, 0, 1.0), N.ExrPlane(16, 1, 0.0), N.ExrPlane(16, 1, float("nan")),
                  N.ExrPlane(16, 1, float("inf"))):
        assert L.pt_exr_enc_planes(e, (N.ExrPlane * 1)(plane), 16, 64, 16, None) == 1
    assert L.pt_exr_enc_profile_read(e, (C.c_float * 6)()) == 1 and L.pt_exr_enc_profile(None, 1) == 1
    assert L.pt_exr_enc_destroy(e) == 0
    n = C.c_int64(0)
    assert L.pt_exr_encode_host(8, 8, ch, 1, None, None, None, C.byref(prm), None, 0, C.byref(n)) == 1
    assert L.pt_preview_exr(None, 1, 1, None, None, 0, None, None) == 1


@pytest.mark.parametrize("typ,limit", [(R.FLOAT, 1.02), (R.HALF, 1.03)])
def test_size_against_zlib_rle(typ, limit):
    from tests.png_enc_cases import golden_800
    img = golden_800().astype(np.float32) / np.float32(255)
    chans = [(n, typ, np.ascontiguousarray(img[..., k]), 1.0) for k, n in enumerate("RGB")]
    enc = R.encode(chans, R.ZIP)
    ours = ref = 0
    for k, p in enumerate(enc.p):
        co = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
        z = len(co.compress(p) + co.flush())
        ref += enc.n[k] if R.raw_fallback(z, enc.n[k]) else z
        ours += len(enc.payload[k])
    print(f"type {typ}: payload {ours}, zlib RLE {ref}, ratio {ours / ref:.4f}, raw chunks {sum(enc.raw)} of {len(enc.raw)}")
    assert ours <= limit * ref
