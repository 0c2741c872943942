"""numpy restatement of the device JPEG encoder (csrc/pt_jpeg_enc.hip): baseline
sequential JFIF, YCbCr 4:4:4 or 4:2:0, the Annex K tables, one scan without restart markers.  Every
operation is an int32 / int64 operation in the order §14 states, so the bytes are a function of the
input bytes alone; the GPU tests compare the kernel's file with encode()'s byte for byte.  decode_coefs
is a Huffman decoder of its own (driven by the tables the file carries) for the closed-loop tests."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

# T[u][x] = round(2^13 s(u) cos((2x + 1) u pi / 16)), s(0) = sqrt(1/8), s(u) = 1/2: literals, as in the kernel
T = np.array([[2896, 2896, 2896, 2896, 2896, 2896, 2896, 2896],
              [4017, 3406, 2276, 799, -799, -2276, -3406, -4017],
              [3784, 1567, -1567, -3784, -3784, -1567, 1567, 3784],
              [3406, -799, -4017, -2276, 2276, 4017, 799, -3406],
              [2896, -2896, -2896, 2896, 2896, -2896, -2896, 2896],
              [2276, -4017, 799, 3406, -3406, -799, 4017, -2276],
              [1567, -3784, 3784, -1567, -1567, 3784, -3784, 1567],
              [799, -2276, 3406, -4017, 4017, -3406, 2276, -799]], np.int64)

# zigzag position -> natural index (ITU T.81 figure A.6)
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,
                   7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31,
                   39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

# ITU T.81 Annex K.1: quantisation tables, natural order
Q_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                   14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                   49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
Q_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                     47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32)

# ITU T.81 Annex K.3: BITS (codes per length 1..16) and HUFFVAL
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125],
           [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
            0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
            0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
            0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
            0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
            0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
            0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
            0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
            0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119],
             [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
              0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
              0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
              0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
              0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
              0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
              0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
              0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
              0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])

S444, S420 = 0, 1          # PT_JPEG_444 / PT_JPEG_420
BLOCK_BITS_MAX = 1664      # 20 (DC) + 63 * 26 (AC) bits bound one block's code
STUFF_CHUNK = 4096         # bytes of the unstuffed stream one workgroup of the stuffing kernels takes
HEADER_BYTES = 623


def quant_table(base: np.ndarray, quality: int) -> np.ndarray:
    """The IJG rule: scale = 5000 / quality below 50 else 200 - 2 quality; (base scale + 50) / 100 in 1..255."""
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((base.astype(np.int64) * scale + 50) // 100, 1, 255)


def huff_codes(bits, vals) -> dict:
    """Canonical codes (T.81 Annex C): symbol -> (code, length)."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def blocks_of(width: int, height: int, sub: int) -> int:
    if sub == S444:
        return 3 * ((width + 7) // 8) * ((height + 7) // 8)
    return 6 * ((width + 15) // 16) * ((height + 15) // 16)


def bound(width: int, height: int, sub: int) -> int:
    """pt_jpeg_enc_bound: header + 2 x the unstuffed worst case + 2."""
    return HEADER_BYTES + 2 * (blocks_of(width, height, sub) * BLOCK_BITS_MAX // 8) + 2


def header(width: int, height: int, quality: int, sub: int) -> bytes:
    def seg(marker: int, body: bytes) -> bytes:
        return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + body

    out = b"\xff\xd8" + seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for tid, base in ((0, Q_LUMA), (1, Q_CHROMA)):
        out += seg(0xDB, bytes([tid]) + bytes(int(v) for v in quant_table(base, quality)[ZIGZAG]))
    hv = 0x11 if sub == S444 else 0x22
    out += seg(0xC0, bytes([8]) + height.to_bytes(2, "big") + width.to_bytes(2, "big") +
               bytes([3, 1, hv, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tc_th, (bits, vals) in ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA)):
        out += seg(0xC4, bytes([tc_th]) + bytes(bits) + bytes(vals))
    out += seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    assert len(out) == HEADER_BYTES
    return out


def preview_bytes(accum: np.ndarray, samples: float) -> np.ndarray:
    """k_preview's bytes of a float32 accumulator: (int)((double)(v / n) * 255.0) clamped to 0..255."""
    v = (np.asarray(accum, np.float32) / np.float32(samples)).astype(np.float64) * 255.0
    return np.clip(np.trunc(v), 0, 255).astype(np.uint8)


def _component_blocks(plane: np.ndarray) -> np.ndarray:
    """(8 by, 8 bx) samples -> (by, bx, 8, 8)."""
    h, w = plane.shape
    return plane.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)


def quantised(rgb: np.ndarray, quality: int, sub: int, mirror_x: bool = False) -> np.ndarray:
    """The quantised coefficients, (blocks, 64) int64 in zigzag order, blocks in MCU-interleaved scan order."""
    px = np.asarray(rgb)[..., :3].astype(np.int64)
    if mirror_x:
        px = px[:, ::-1]
    h, w = px.shape[:2]
    m = 8 if sub == S444 else 16
    px = np.pad(px, ((0, -h % m), (0, -w % m), (0, 0)), mode="edge")   # the last column and row replicated
    r, g, b = px[..., 0], px[..., 1], px[..., 2]
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11058 * r - 21710 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    assert min(y.min(), cb.min(), cr.min()) >= 0 and max(y.max(), cb.max(), cr.max()) <= 255
    if sub == S420:
        cb = (cb[0::2, 0::2] + cb[0::2, 1::2] + cb[1::2, 0::2] + cb[1::2, 1::2] + 2) >> 2
        cr = (cr[0::2, 0::2] + cr[0::2, 1::2] + cr[1::2, 0::2] + cr[1::2, 1::2] + 2) >> 2
    qt = [quant_table(Q_LUMA, quality), quant_table(Q_CHROMA, quality)]
    comp = []
    for k, plane in enumerate((y, cb, cr)):
        s = _component_blocks(plane) - 128                                  # [by, bx, y, x]
        row = (np.einsum("ux,abyx->abyu", T, s) + 256) >> 9                 # sums below 2^23
        f = np.einsum("vy,abyu->abvu", T, row)                              # scaled by 2^17, below 2^29
        assert np.abs(f).max() < 1 << 29
        q = qt[min(k, 1)].reshape(8, 8)
        v = np.sign(f) * ((np.abs(f) + (q << 16)) // (q << 17))
        v[..., 1:, :] = np.clip(v[..., 1:, :], -1023, 1023)
        v[..., 0, 1:] = np.clip(v[..., 0, 1:], -1023, 1023)
        v[..., 0, 0] = np.clip(v[..., 0, 0], -1024, 1023)
        comp.append(v.reshape(v.shape[0], v.shape[1], 64)[..., ZIGZAG])
    my, mx = comp[1].shape[:2]
    if sub == S444:
        mcu = np.stack(comp, axis=2)                                        # [my, mx, 3, 64]
    else:
        yb = comp[0].reshape(my, 2, mx, 2, 64).transpose(0, 2, 1, 3, 4).reshape(my, mx, 4, 64)
        mcu = np.concatenate([yb, comp[1][:, :, None], comp[2][:, :, None]], axis=2)
    return mcu.reshape(-1, 64)


def component_of(block: int, sub: int) -> int:
    k = block % (3 if sub == S444 else 6)
    return k if sub == S444 else max(0, k - 3)


def prev_block(block: int, sub: int) -> int:
    """The previous block of the same component in scan order (-1: none): arithmetic on the block number."""
    if sub == S444:
        return block - 3
    k = block % 6
    if k >= 4:
        return block - 6
    if k > 0:
        return block - 1
    return block - 3 if block >= 6 else -1


@dataclass
class Encoded:
    data: bytes
    coefs: np.ndarray                 # (blocks, 64), zigzag order, scan order
    bit_lengths: list = field(default_factory=list)
    unstuffed_bytes: int = 0
    stuffed: int = 0                  # 0xFF bytes of the entropy-coded segment (each followed by a 0x00)
    zrl: int = 0                      # ZRL codes emitted


def _bitlen(a: int) -> int:
    return int(a).bit_length()


def encode(rgb: np.ndarray, quality: int = 90, sub: int = S420, mirror_x: bool = False) -> Encoded:
    rgb = np.asarray(rgb)
    h, w = rgb.shape[:2]
    coefs = quantised(rgb, quality, sub, mirror_x)
    dc = [huff_codes(*DC_LUMA), huff_codes(*DC_CHROMA)]
    ac = [huff_codes(*AC_LUMA), huff_codes(*AC_CHROMA)]
    acc, nbits, zrl, lengths = 0, 0, 0, []     # acc: the bits not yet moved to `raw` (fewer than 8 between blocks)
    raw, done = bytearray(), 0
    rows = coefs.tolist()
    for b, c in enumerate(rows):
        t = min(component_of(b, sub), 1)
        start = nbits
        p = prev_block(b, sub)
        d = c[0] - (rows[p][0] if p >= 0 else 0)
        s = _bitlen(abs(d))
        code, ln = dc[t][s]
        acc = (acc << (ln + s)) | (code << s) | ((d if d >= 0 else d + (1 << s) - 1) & ((1 << s) - 1))
        nbits += ln + s
        run = 0
        for k in range(1, 64):
            v = c[k]
            if v == 0:
                run += 1
                continue
            while run >= 16:
                code, ln = ac[t][0xF0]
                acc = (acc << ln) | code
                nbits += ln
                run -= 16
                zrl += 1
            s = _bitlen(abs(v))
            code, ln = ac[t][(run << 4) | s]
            acc = (acc << (ln + s)) | (code << s) | ((v if v >= 0 else v + (1 << s) - 1) & ((1 << s) - 1))
            nbits += ln + s
            run = 0
        if run > 0:
            code, ln = ac[t][0x00]
            acc = (acc << ln) | code
            nbits += ln
        lengths.append(nbits - start)
        assert nbits - start <= BLOCK_BITS_MAX
        whole, left = (nbits - done) // 8, (nbits - done) % 8
        raw += (acc >> left).to_bytes(whole, "big")
        acc &= (1 << left) - 1
        done += 8 * whole
    pad = -nbits % 8
    if pad:
        raw.append((acc << pad) | ((1 << pad) - 1))   # the final byte padded with 1-bits
    raw = bytes(raw)
    body = raw.replace(b"\xff", b"\xff\x00")
    data = header(w, h, quality, sub) + body + b"\xff\xd9"
    return Encoded(data, coefs, lengths, len(raw), raw.count(b"\xff"), zrl)


# ---- a decoder of its own: file -> quantised coefficients ---------------------------------------
def parse_header(data: bytes) -> dict:
    """Marker segments up to SOS: size, sampling factors, quantisation tables (natural order), Huffman
    (BITS, HUFFVAL) lists and the offset of the entropy-coded segment."""
    assert data[:2] == b"\xff\xd8"
    info = {"qt": {}, "ht": {}, "segments": []}
    i = 2
    while True:
        assert data[i] == 0xFF
        m, ln = data[i + 1], int.from_bytes(data[i + 2:i + 4], "big")
        seg = data[i + 4:i + 2 + ln]
        info["segments"].append(m)
        if m == 0xE0:
            info["jfif"] = seg
        elif m == 0xDB:
            assert len(seg) == 65 and seg[0] >> 4 == 0
            nat = np.zeros(64, np.int64)
            nat[ZIGZAG] = list(seg[1:])
            info["qt"][seg[0] & 15] = nat
        elif m == 0xC0:
            info["precision"] = seg[0]
            info["height"], info["width"] = int.from_bytes(seg[1:3], "big"), int.from_bytes(seg[3:5], "big")
            info["components"] = [(seg[6 + 3 * c], seg[7 + 3 * c], seg[8 + 3 * c]) for c in range(seg[5])]
        elif m == 0xC4:
            bits = list(seg[1:17])
            info["ht"][seg[0]] = (bits, list(seg[17:17 + sum(bits)]))
            assert len(seg) == 17 + sum(bits)
        elif m == 0xDA:
            info["scan"] = seg
            info["ecs"] = i + 2 + ln
            return info
        else:
            raise AssertionError(f"unexpected marker {m:#x}")
        i += 2 + ln


def decode_coefs(data: bytes) -> np.ndarray:
    """The quantised coefficients of a file, as `quantised` orders them; asserts that the scan ends exactly at EOI
    after at most 7 padding 1-bits."""
    info = parse_header(data)
    assert data[-2:] == b"\xff\xd9"
    ecs = data[info["ecs"]:-2]
    assert b"\xff" not in ecs.replace(b"\xff\x00", b"")   # every 0xFF is stuffed: no marker inside
    raw = ecs.replace(b"\xff\x00", b"\xff")
    total = len(raw) * 8
    stream = int.from_bytes(raw, "big")
    pos = 0

    def take(n: int) -> int:
        nonlocal pos
        pos += n
        assert pos <= total
        return (stream >> (total - pos)) & ((1 << n) - 1)

    def lookup(table: dict) -> int:
        code = 0
        for length in range(1, 17):
            code = (code << 1) | take(1)
            if (code, length) in table:
                return table[(code, length)]
        raise AssertionError("bad Huffman code")

    def extend(v: int, s: int) -> int:
        return v if s == 0 or v >= 1 << (s - 1) else v - (1 << s) + 1

    inv = {k: {cl: sym for sym, cl in huff_codes(*bv).items()} for k, bv in info["ht"].items()}
    sub = S444 if info["components"][0][1] == 0x11 else S420
    n = blocks_of(info["width"], info["height"], sub)
    out = np.zeros((n, 64), np.int64)
    for b in range(n):
        t = min(component_of(b, sub), 1)
        s = lookup(inv[t])
        p = prev_block(b, sub)
        out[b, 0] = (out[p, 0] if p >= 0 else 0) + extend(take(s), s)
        k = 1
        while k < 64:
            rs = lookup(inv[0x10 | t])
            r, s = rs >> 4, rs & 15
            if s == 0:
                if r != 15:
                    break          # EOB
                k += 16            # ZRL
                continue
            k += r
            out[b, k] = extend(take(s), s)
            k += 1
        assert k <= 64
    rest = total - pos
    assert 0 <= rest < 8 and take(rest) == (1 << rest) - 1
    return out
