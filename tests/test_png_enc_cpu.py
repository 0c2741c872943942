"""The PNG encoder's definition without a GPU: the numpy restatement's files (tests/png_enc_ref.py)
are valid PNG files of the right pixels, the crafted cases reach what they are for, the files are no larger than
today's, and the argument checks of the native library need no device.

Payload against zlib's own run-length coder, zlib.compressobj(6, DEFLATED, 15, 8, Z_RLE), over the same F:
golden Cornell [::4, ::4] (200 x 200) 48251 / 48064 = 1.0039, golden Cornell 800 x 800 731390 / 729789 = 1.0022;
asserted at the next whole percent, 1.01."""
import ctypes as C
import io
import struct
import warnings
import zlib

import numpy as np
import pytest

from tests import png_enc_cases as K
from tests import png_enc_ref as R


def parse(data: bytes) -> dict:
    """Signature and the chunks, each CRC checked."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    out, i = [], 8
    while i < len(data):
        n, tag = struct.unpack(">I", data[i:i + 4])[0], data[i + 4:i + 8]
        body = data[i + 8:i + 8 + n]
        assert struct.unpack(">I", data[i + 8 + n:i + 12 + n])[0] == zlib.crc32(tag + body)
        out.append((tag, body))
        i += 12 + n
    assert i == len(data) and [t for t, _ in out] == [b"IHDR", b"IDAT", b"IEND"]
    return dict(out)


def check_file(enc: R.Encoded, img: np.ndarray, mirror: bool = False) -> None:
    from PIL import Image
    h, w = img.shape[:2]
    chunks = parse(enc.data)
    assert struct.unpack(">IIBBBBB", enc.data[16:29]) == (w, h, 8, 2, 0, 0, 0) and len(chunks[b"IHDR"]) == 13
    assert chunks[b"IDAT"] == enc.payload and zlib.decompress(enc.payload) == enc.f
    assert struct.unpack(">I", enc.payload[-4:])[0] == zlib.adler32(enc.f)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        got = np.asarray(Image.open(io.BytesIO(enc.data)))
    want = img[..., :3]
    assert np.array_equal(got, want[:, ::-1] if mirror else want)
    assert len(enc.f) == R.stream_bytes(w, h)


@pytest.mark.parametrize("block", K.BLOCKS)
@pytest.mark.parametrize("filt", K.FILTERS)
@pytest.mark.parametrize("w,h", K.SIZES)
def test_sizes(w, h, filt, block):
    img = K.noisy(w, h)
    enc = R.encode(img, filt, block)
    check_file(enc, img)
    assert set(enc.filters) == {filt} if filt != R.ADAPTIVE else set(enc.filters) <= {0, 1, 2, 3, 4}
    assert len(enc.data) <= R.bound(w, h, block)
    assert len(enc.block_types) == R.blocks_of(w, h, block)


def test_adaptive_picks_several_types():
    assert len(set(R.encode(K.noisy(64, 48)).filters)) >= 3


def test_mirror_and_alpha():
    img = K.noisy(17, 9, chans=4)
    enc = R.encode(img, mirror_x=True)
    check_file(enc, img, mirror=True)
    assert enc.data == R.encode(np.ascontiguousarray(img[:, ::-1, :3])).data != R.encode(img).data


def test_constant_image():
    enc = K.reference("constant")
    check_file(enc, K.crafted()["constant"][0])
    assert set(enc.f) == {0} and len(enc.f) == 3630
    # chunk 0: a literal, then 511 bytes; 6 more whole chunks; the last has 3630 - 7 * 512 = 46 bytes
    assert enc.matches == [258, 253] + [258, 254] * 6 + [46]
    for start in (R.CHUNK, R.BLOCK_MIN):                                         # a lane chunk's, a deflate block's start
        assert R.tokens_of(enc.f, start, start + R.CHUNK) == [256 + 258, 256 + 254]
    assert len(enc.block_types) == 4


def test_random_bytes():
    enc = K.reference("random")
    check_file(enc, K.crafted()["random"][0])
    assert enc.block_types == [2] and enc.matches == []


def test_one_pixel_is_a_fixed_block():
    enc = K.reference("one_pixel")
    check_file(enc, K.crafted()["one_pixel"][0])
    assert enc.block_types == [1]


def test_both_block_types():
    enc = K.reference("both_types")
    check_file(enc, K.crafted()["both_types"][0])
    assert enc.block_types == [2] * 9 + [1]


def test_length_limit_15():
    enc = K.reference("fibonacci")
    check_file(enc, K.crafted()["fibonacci"][0])
    assert enc.block_types == [2] and enc.matches == []
    assert enc.lit_info[0]["unlimited_max"] > 15 and enc.lit_info[0]["max"] == 15


def test_length_limit_7():
    enc = K.reference("code_length_7")
    check_file(enc, K.crafted()["code_length_7"][0])
    assert enc.block_types == [2] and enc.matches == []
    assert enc.lit_info[0]["unlimited_max"] == 15
    assert enc.cl_info[0]["unlimited_max"] > 7 and enc.cl_info[0]["max"] == 7


def test_conversions():
    from cuda_pathtracer_amd import tonemap
    acc = K.accumulator()
    save = R.save_bytes(acc, 3.0)
    assert np.array_equal(save[:, ::-1], tonemap(acc, 3.0))         # pt_tonemap (host code) mirrors x
    assert save.min() == 0 and save.max() == 255
    check_file(R.encode(save, mirror_x=True), save, mirror=True)
    # The double product and the float product truncate alike on every finite quotient (a float x times
    # 255 never lies within half a float step below an integer), so no input separates the two conversions; every
    # float of one binade is checked here, the boundaries and the clamps by the crafted case.
    assert np.array_equal(R.preview_bytes(acc, 3.0), save)
    binade = np.arange(0x3F000000, 0x3F800000, dtype=np.uint32).view(np.float32)      # [0.5, 1)
    assert np.array_equal(R.preview_bytes(binade, 1.0), R.save_bytes(binade, 1.0))


def test_bound_is_the_formula():
    for (w, h), block in [((1, 1), 1024), ((7, 5), 1024), ((800, 800), 32768), ((3840, 2160), 32768)]:
        n = h * (1 + 3 * w)
        assert R.bound(w, h, block) == (9 * n + 10 * ((n + block - 1) // block) + 7) // 8 + 63


def test_argument_errors_need_no_device():
    from cuda_pathtracer_amd import PngParams
    from cuda_pathtracer_amd import _native as N
    L = N.lib()
    e = C.c_void_p()

    def create(w, h, **kw):
        p = PngParams.default()
        for k, v in kw.items():
            setattr(p, k, v)
        return L.pt_png_enc_create(w, h, C.byref(p), C.byref(e))

    d = PngParams.default()
    assert (d.filter, d.block_bytes, d.conv, d.mirror_x) == (N.PNG_FILTER_ADAPTIVE, R.BLOCK_DEFAULT, N.PNG_CONV_PREVIEW, 0)
    for bad in (dict(filter=-1), dict(filter=6), dict(block_bytes=512), dict(block_bytes=1000), dict(block_bytes=2 << 20),
                dict(conv=2), dict(conv=-1)):
        assert create(8, 8, **bad) == 1, bad
    p = PngParams.default()
    p.reserved[2] = 1
    assert L.pt_png_enc_create(8, 8, C.byref(p), C.byref(e)) == 1
    assert create(0, 8) == 1 and create(8, 0) == 1 and create(-3, 8) == 1
    assert L.pt_png_enc_create(8, 8, None, C.byref(e)) == 1 and L.pt_png_enc_create(8, 8, C.byref(d), None) == 1
    # 9 N + 10 blocks bits must stay below 2^31: N = 8930 * 26791 = 239.2 million bytes is too many, 8900 * 26701 fits
    assert create(8930, 8930) == 1 and create(65535, 65535) == 1
    assert create(8900, 8900) == 0 and L.pt_png_enc_bound(e) == R.bound(8900, 8900) and L.pt_png_enc_destroy(e) == 0
    assert L.pt_png_enc_bound(None) == 0 and L.pt_png_enc_destroy(None) == 0
    # a created object answers bound without a device, and the encode entries check before they touch one
    for (w, h), block in [((1, 1), 1024), ((17, 9), 1024), ((800, 800), 32768)]:
        assert create(w, h, block_bytes=block) == 0
        assert L.pt_png_enc_bound(e) == R.bound(w, h, block)
        assert L.pt_png_enc_pixels(e, None, 3, None, 0, None, None) == 1
        assert L.pt_png_enc_pixels(e, 16, 5, 16, 64, 16, None) == 1
        assert L.pt_png_enc_pixels(e, 16, 3, 16, -1, 16, None) == 1
        assert L.pt_png_enc_accum(e, 16, C.c_float(0.0), 16, 64, 16, None) == 1
        assert L.pt_png_enc_accum(e, 16, C.c_float(float("nan")), 16, 64, 16, None) == 1
        assert L.pt_png_enc_profile_read(e, (C.c_float * 6)()) == 1
        assert L.pt_png_enc_destroy(e) == 0
    n = C.c_int64(0)
    assert L.pt_png_encode_host(8, 8, None, 3, C.byref(d), None, 0, C.byref(n)) == 1
    assert L.pt_preview_png(None, 1, None, None, 0, None, None) == 1


@pytest.mark.parametrize("name", ["golden_200", "golden_800"])
def test_size_against_todays_encoder_and_zlib_rle(name):
    from cuda_pathtracer_amd.preview import png_bytes
    img = getattr(K, name)()
    enc = R.encode(img)
    check_file(enc, img)
    assert len(enc.data) <= len(png_bytes(img))
    co = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
    rle = co.compress(enc.f) + co.flush()
    print(f"{name}: file {len(enc.data)}, png_bytes {len(png_bytes(img))}, payload {len(enc.payload)}, zlib RLE {len(rle)}, "
          f"ratio {len(enc.payload) / len(rle):.4f}")
    assert len(enc.payload) <= 1.01 * len(rle)
