"""The JPEG encoder's definition without a device: the numpy restatement
(tests/jpeg_enc_ref.py) writes files that its own Huffman decoder, the native stb-pinned decoder and
libjpeg (Pillow) all read; its fidelity is libjpeg's; and the C ABI's argument checks, bound and header
need no device."""
import ctypes as C
import io
import math
import warnings

import numpy as np
import pytest

from cuda_pathtracer_amd import _native as N
from cuda_pathtracer_amd.pathtrace import decode_jpeg
from tests import jpeg_enc_ref as R
from tests.conftest import SCENES

SIZES = [(1, 1), (8, 8), (7, 5), (17, 9), (64, 48)]   # (width, height)
SUBS = [R.S444, R.S420]
QUALITIES = [1, 50, 90, 100]
CASES = [(w, h, sub, q) for (w, h) in SIZES for sub in SUBS for q in QUALITIES]
PT_ERR_ARG = 1


def _image(w, h, seed=0):
    """Smooth colour ramps plus noise: coefficients of every size, runs of zeros at the lower qualities."""
    rng = np.random.default_rng(1000 * w + h + seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([x * 255 // max(w - 1, 1), y * 255 // max(h - 1, 1), (x + y) * 255 // max(w + h - 2, 1)], -1)
    return np.clip(base + rng.integers(-40, 41, (h, w, 3)), 0, 255).astype(np.uint8)


_FILES = {}


def _encoded(w, h, sub, q):
    key = (w, h, sub, q)
    if key not in _FILES:
        _FILES[key] = R.encode(_image(w, h), q, sub)
    return _FILES[key]


def test_dct_table_is_the_rounded_cosine():
    for u in range(8):
        for x in range(8):
            s = math.sqrt(1 / 8) if u == 0 else 0.5
            assert R.T[u][x] == round(8192 * s * math.cos((2 * x + 1) * u * math.pi / 16))


def test_colour_conversion_needs_no_clamp():
    """Every Y, Cb, Cr of the fixed-point matrix lies in 0..255: the extremes are at corners of the RGB cube."""
    c = np.array([[r, g, b] for r in (0, 255) for g in (0, 255) for b in (0, 255)], np.uint8).reshape(1, 8, 3)
    R.quantised(c, 90, R.S444)   # (asserts the range)
    rng = np.random.default_rng(5)
    R.quantised(rng.integers(0, 256, (64, 64, 3), dtype=np.uint8), 90, R.S444)


@pytest.mark.parametrize("w,h,sub,q", CASES)
def test_closed_loop(w, h, sub, q):
    e = _encoded(w, h, sub, q)
    assert e.coefs.shape == (R.blocks_of(w, h, sub), 64)
    assert np.array_equal(R.decode_coefs(e.data), e.coefs)
    assert len(e.data) <= R.bound(w, h, sub)
    assert max(e.bit_lengths) <= R.BLOCK_BITS_MAX


@pytest.mark.parametrize("w,h,sub,q", CASES)
def test_native_decoder_reads_it(w, h, sub, q):
    got = decode_jpeg(_encoded(w, h, sub, q).data)
    assert got.shape == (h, w, 3)


@pytest.mark.parametrize("w,h,sub,q", CASES)
def test_pillow_reads_it(w, h, sub, q):
    Image = pytest.importorskip("PIL.Image")
    with warnings.catch_warnings():
        warnings.simplefilter("error")   # libjpeg's "extraneous bytes" / "premature end" arrive as warnings
        im = Image.open(io.BytesIO(_encoded(w, h, sub, q).data))
        im.load()
    assert im.mode == "RGB" and np.asarray(im).shape == (h, w, 3)


def test_quality_100_decodes_close_to_the_source():
    """End to end through an independent decoder: a wrong table, zigzag or chroma phase costs far more."""
    img = _image(64, 48)
    got = decode_jpeg(R.encode(img, 100, R.S444).data).astype(int)
    assert np.abs(got - img.astype(int)).max() <= 6


def _psnr(a, b):
    return 10 * math.log10(255.0 ** 2 / np.mean((a.astype(float) - b.astype(float)) ** 2))


@pytest.mark.parametrize("name", ["wallpaper.jpg", "chair.jpg"])
@pytest.mark.parametrize("q", [50, 90])
@pytest.mark.parametrize("sub", SUBS)
def test_fidelity_against_libjpeg(name, q, sub):
    """PSNR against the source, both files decoded by Pillow: ours no more than 0.5 dB below libjpeg's file
    of the same settings.  Measured: differences between -0.09 and +0.01 dB."""
    Image = pytest.importorskip("PIL.Image")
    src = decode_jpeg((SCENES / "Textures" / name).read_bytes())
    ours = np.asarray(Image.open(io.BytesIO(R.encode(src, q, sub).data)).convert("RGB"))
    bio = io.BytesIO()
    Image.fromarray(src).save(bio, "JPEG", quality=q, optimize=False, subsampling=0 if sub == R.S444 else 2)
    theirs = np.asarray(Image.open(io.BytesIO(bio.getvalue())).convert("RGB"))
    a, b = _psnr(ours, src), _psnr(theirs, src)
    print(f"{name} q{q} {'444' if sub == R.S444 else '420'}: ours {a:.3f} dB, libjpeg {b:.3f} dB, diff {a - b:+.3f}")
    assert a >= b - 0.5


# ---- C ABI without a device -------------------------------------------------------------------------------
def _params(quality=90, sub=R.S420, mirror=0):
    p = N.JpegParams.default()
    p.quality, p.subsampling, p.mirror_x = quality, sub, mirror
    return p


def _create(w, h, p):
    e = C.c_void_p()
    return N.lib().pt_jpeg_enc_create(w, h, C.byref(p) if p is not None else None, C.byref(e)), e


def test_params_default():
    p = N.JpegParams.default()
    assert (p.quality, p.subsampling, p.mirror_x, list(p.reserved)) == (90, N.JPEG_420, 0, [0] * 5)


def test_create_argument_errors():
    L = N.lib()
    bad = [(64, 64, _params(quality=0)), (64, 64, _params(quality=101)), (64, 64, _params(sub=2)), (64, 64, _params(sub=-1)),
           (0, 64, _params()), (64, 0, _params()), (-3, 64, _params()), (65536, 8, _params()), (8, 65536, _params()),
           (65535, 65535, _params()),                  # the block cap: blocks * 1664 >= 2^31
           (65535, 417, _params(sub=R.S444)),          # 3 * 8192 * 53 * 1664 >= 2^31 ...
           (64, 64, None)]
    res = _params()
    res.reserved[2] = 1
    bad.append((64, 64, res))
    for w, h, p in bad:
        rc, e = _create(w, h, p)
        assert rc == PT_ERR_ARG and not e.value, (w, h)
        assert L.pt_last_error()
    assert L.pt_jpeg_enc_create(64, 64, C.byref(_params()), None) == PT_ERR_ARG
    rc, e = _create(65535, 416, _params(sub=R.S444))   # ... and 3 * 8192 * 52 * 1664 < 2^31 is accepted
    assert rc == 0 and R.blocks_of(65535, 416, R.S444) * 1664 < 2 ** 31 <= R.blocks_of(65535, 417, R.S444) * 1664
    assert L.pt_jpeg_enc_destroy(e) == 0


def test_encode_argument_errors_before_any_device_call():
    L = N.lib()
    rc, e = _create(16, 16, _params())
    assert rc == 0
    one = C.c_void_p(256)   # (never dereferenced: every case fails its argument check first)
    assert L.pt_jpeg_enc_pixels(e, one, 2, one, 4096, one, None) == PT_ERR_ARG
    assert L.pt_jpeg_enc_pixels(e, one, 5, one, 4096, one, None) == PT_ERR_ARG
    assert L.pt_jpeg_enc_pixels(None, one, 3, one, 4096, one, None) == PT_ERR_ARG
    assert L.pt_jpeg_enc_pixels(e, None, 3, one, 4096, one, None) == PT_ERR_ARG
    assert L.pt_jpeg_enc_pixels(e, one, 3, None, 4096, one, None) == PT_ERR_ARG
    assert L.pt_jpeg_enc_pixels(e, one, 3, one, 4096, None, None) == PT_ERR_ARG
    assert L.pt_jpeg_enc_pixels(e, one, 3, one, -1, one, None) == PT_ERR_ARG
    for samples in (0.0, -1.0, float("inf"), float("nan")):
        assert L.pt_jpeg_enc_accum(e, one, samples, one, 4096, one, None) == PT_ERR_ARG
    assert L.pt_jpeg_enc_accum(e, None, 1.0, one, 4096, one, None) == PT_ERR_ARG
    assert L.pt_jpeg_enc_accum(None, one, 1.0, one, 4096, one, None) == PT_ERR_ARG
    assert L.pt_preview_jpeg(None, 1, e, one, 4096, one, None) == PT_ERR_ARG
    assert L.pt_jpeg_enc_destroy(e) == 0
    pix = np.zeros((16, 16, 3), np.uint8)
    out, n = np.zeros(8192, np.uint8), C.c_int64(0)
    host = lambda w, h, px, stride, p, o, cap, sz: L.pt_jpeg_encode_host(   # noqa: E731
        w, h, px, stride, C.byref(p) if p is not None else None, o, cap, sz)
    po, oo = pix.ctypes.data, out.ctypes.data
    assert host(16, 16, None, 3, _params(), oo, out.size, C.byref(n)) == PT_ERR_ARG
    assert host(16, 16, po, 3, _params(), None, out.size, C.byref(n)) == PT_ERR_ARG
    assert host(16, 16, po, 3, _params(), oo, out.size, None) == PT_ERR_ARG
    assert host(16, 16, po, 2, _params(), oo, out.size, C.byref(n)) == PT_ERR_ARG
    assert host(16, 16, po, 3, _params(quality=0), oo, out.size, C.byref(n)) == PT_ERR_ARG
    assert host(16, 16, po, 3, _params(sub=7), oo, out.size, C.byref(n)) == PT_ERR_ARG
    assert host(16, 16, po, 3, None, oo, out.size, C.byref(n)) == PT_ERR_ARG
    assert host(0, 16, po, 3, _params(), oo, out.size, C.byref(n)) == PT_ERR_ARG
    assert host(16, 70000, po, 3, _params(), oo, out.size, C.byref(n)) == PT_ERR_ARG
    assert N.lib().pt_jpeg_enc_bound(None) == 0


@pytest.mark.parametrize("w,h", [(1, 1), (17, 9), (800, 800), (3840, 2160)])
@pytest.mark.parametrize("sub", SUBS)
def test_bound_is_the_formula(w, h, sub):
    rc, e = _create(w, h, _params(sub=sub))
    assert rc == 0
    blocks = R.blocks_of(w, h, sub)
    assert N.lib().pt_jpeg_enc_bound(e) == 623 + 2 * (blocks * 1664 // 8) + 2 == R.bound(w, h, sub)
    N.lib().pt_jpeg_enc_destroy(e)


@pytest.mark.parametrize("w,h,sub,q,mirror", [(1, 1, R.S444, 90, 0), (17, 9, R.S420, 1, 1), (800, 600, R.S420, 50, 0),
                                              (65535, 3, R.S444, 100, 0), (333, 65535, R.S420, 75, 1)])
def test_header(w, h, sub, q, mirror):
    """The native header is the restatement's, and parses to the requested size, sampling factors and tables."""
    rc, e = _create(w, h, _params(q, sub, mirror))
    assert rc == 0
    buf = (C.c_uint8 * 1024)()
    n = N.lib().pt_jpeg_enc_header(e, buf, 1024)
    N.lib().pt_jpeg_enc_destroy(e)
    hdr = bytes(buf[:n])
    assert n == R.HEADER_BYTES and hdr == R.header(w, h, q, sub)
    info = R.parse_header(hdr)
    assert (info["width"], info["height"], info["precision"]) == (w, h, 8)
    assert info["components"] == [(1, 0x11 if sub == R.S444 else 0x22, 0), (2, 0x11, 1), (3, 0x11, 1)]
    assert info["segments"] == [0xE0, 0xDB, 0xDB, 0xC0, 0xC4, 0xC4, 0xC4, 0xC4, 0xDA]
    assert info["jfif"][:5] == b"JFIF\0"
    assert np.array_equal(info["qt"][0], R.quant_table(R.Q_LUMA, q))
    assert np.array_equal(info["qt"][1], R.quant_table(R.Q_CHROMA, q))
    assert info["ht"] == {0x00: R.DC_LUMA, 0x10: R.AC_LUMA, 0x01: R.DC_CHROMA, 0x11: R.AC_CHROMA}
    assert info["ecs"] == n


def test_quality_rule():
    assert np.array_equal(R.quant_table(R.Q_LUMA, 50), R.Q_LUMA)
    assert R.quant_table(R.Q_LUMA, 100).max() == 1 and R.quant_table(R.Q_CHROMA, 1).min() == 255
    assert R.quant_table(R.Q_LUMA, 25)[0] == (16 * 200 + 50) // 100
