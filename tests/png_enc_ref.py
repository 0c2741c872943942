"""numpy restatement of the device PNG encoder (csrc/pt_png_enc.hip): 8-bit RGB, one IDAT
holding one zlib stream whose deflate blocks use literals and distance-1 matches only, coded per block
with the fixed or a dynamic Huffman code.  Every step is an integer operation in the order §15 states,
so the file is a function of the input bytes; the GPU tests compare the kernels' file with encode()'s
byte for byte.  The two checksums are zlib's own functions: they have one right answer."""
from __future__ import annotations

import struct
import zlib
from dataclasses import dataclass, field

import numpy as np

CHUNK = 512                 # C: bytes of the filtered stream one lane tokenises
BLOCK_MIN, BLOCK_MAX, BLOCK_DEFAULT = 1024, 1 << 20, 32768
ADAPTIVE = 5                # PT_PNG_FILTER_ADAPTIVE
CONV_PREVIEW, CONV_SAVE = 0, 1
FRAMING = 63                # signature 8, IHDR 25, IDAT 12, zlib header 2, Adler-32 4, IEND 12
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]

# RFC 1951 §3.2.5: length symbol 257 + i codes the lengths from LEN_BASE[i] with LEN_EXTRA[i] extra bits
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227,
            258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
LEN_SYM = {}                # match length -> (symbol, extra bits, extra value)
for _i in range(29):
    for _k in range(LEN_BASE[_i], 259 if _i == 28 else min(LEN_BASE[_i] + (1 << LEN_EXTRA[_i]), 258)):
        LEN_SYM[_k] = (257 + _i, LEN_EXTRA[_i], _k - LEN_BASE[_i])
SYM_EXTRA = [0] * 257 + LEN_EXTRA


def stream_bytes(width: int, height: int) -> int:
    return height * (1 + 3 * width)


def blocks_of(width: int, height: int, block_bytes: int = BLOCK_DEFAULT) -> int:
    return -(-stream_bytes(width, height) // block_bytes)


def bound(width: int, height: int, block_bytes: int = BLOCK_DEFAULT) -> int:
    """pt_png_enc_bound: 9 bits per byte of F and 10 per deflate block, in bytes, plus the framing."""
    return (9 * stream_bytes(width, height) + 10 * blocks_of(width, height, block_bytes) + 7) // 8 + FRAMING


def preview_bytes(accum: np.ndarray, samples: float) -> np.ndarray:
    """PT_PNG_CONV_PREVIEW, k_preview's bytes: (int)((double)(v / n) * 255.0) clamped to 0..255."""
    v = (np.asarray(accum, np.float32) / np.float32(samples)).astype(np.float64) * 255.0
    return np.clip(np.trunc(v), 0, 255).astype(np.uint8)


def save_bytes(accum: np.ndarray, samples: float) -> np.ndarray:
    """PT_PNG_CONV_SAVE, pt_tonemap's bytes: float division, v > 0 ? v : 0, v < 1 ? v : 1, (uint8_t)(v * 255.f)."""
    v = np.asarray(accum, np.float32) / np.float32(samples)
    v = np.where(v > 0, v, np.float32(0))
    v = np.where(v < 1, v, np.float32(1))
    return (v * np.float32(255)).astype(np.uint8)


def filtered(rgb: np.ndarray, filt: int = ADAPTIVE, mirror_x: bool = False):
    """F (H rows of 1 + 3W bytes) and the filter type of every row."""
    px = np.asarray(rgb)[..., :3].astype(np.int64)
    if mirror_x:
        px = px[:, ::-1]
    h, w = px.shape[:2]
    raw = px.reshape(h, 3 * w)
    a = np.concatenate([np.zeros((h, 3), np.int64), raw[:, :-3]], 1)           # left
    b = np.concatenate([np.zeros((1, 3 * w), np.int64), raw[:-1]], 0)          # above (row -1: zeros)
    c = np.concatenate([np.zeros((h, 3), np.int64), b[:, :-3]], 1)             # above left
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    res = np.stack([raw, raw - a, raw - b, raw - ((a + b) >> 1), raw - paeth]) & 255   # [type, y, i]
    cost = np.where(res < 128, res, 256 - res).sum(2)                           # sum of |signed residual|
    types = np.argmin(cost, 0) if filt == ADAPTIVE else np.full(h, filt)        # ties: the lowest type
    rows = res[types, np.arange(h)]
    f = np.concatenate([types[:, None], rows], 1).astype(np.uint8)
    return f.reshape(-1), types


def tokens_of(f: bytes, start: int, end: int) -> list:
    """One lane chunk [start, end) of F, greedily: a literal (0..255) or, where the next k >= 3 bytes equal byte
    i - 1, a match (256 + k), k capped at 258 and at the chunk's end."""
    out, i = [], start
    while i < end:
        if i > 0:
            p, k, lim = f[i - 1], 0, min(258, end - i)
            while k < lim and f[i + k] == p:
                k += 1
            if k >= 3:
                out.append(256 + k)
                i += k
                continue
        out.append(f[i])
        i += 1
    return out


def code_lengths(freq, limit: int, info: dict | None = None) -> list:
    """Huffman code lengths of the symbols with freq > 0 (at least two), at most `limit`.
    1. the used symbols sorted by (freq, symbol);
    2. the two-queue Huffman construction over that order (a leaf is taken before an internal node of the same
       weight), which gives every leaf's depth;
    3. the number of codes of each length, depths beyond the limit counted at the limit;
    4. while the Kraft sum exceeds 1: one code leaves the limit, and the longest shorter code gets it as a sibling
       (count[limit]--, count[l]--, count[l + 1] += 2 for the largest l < limit with count[l] > 0);
    5. the lengths dealt out over the sorted order, the shortest to the most frequent."""
    order = sorted((s for s in range(len(freq)) if freq[s] > 0), key=lambda s: freq[s] * 512 + s)
    n = len(order)
    assert n >= 2
    wt = [freq[s] for s in order] + [0] * (n - 1)
    parent = [0] * (2 * n - 1)
    i, j = 0, n
    for nxt in range(n, 2 * n - 1):
        pick = []
        for _ in range(2):
            if i < n and (j >= nxt or wt[i] <= wt[j]):
                pick.append(i)
                i += 1
            else:
                pick.append(j)
                j += 1
        wt[nxt] = wt[pick[0]] + wt[pick[1]]
        parent[pick[0]] = parent[pick[1]] = nxt
    depth = [0] * (2 * n - 1)
    for v in range(2 * n - 3, -1, -1):
        depth[v] = depth[parent[v]] + 1
    count = [0] * (limit + 1)
    for v in range(n):
        count[min(depth[v], limit)] += 1
    total = sum(count[l] << (limit - l) for l in range(1, limit + 1))
    if info is not None:
        info["unlimited_max"] = max(depth[:n])
        info["moves"] = total - (1 << limit)
    while total > 1 << limit:
        count[limit] -= 1
        for l in range(limit - 1, 0, -1):
            if count[l]:
                count[l] -= 1
                count[l + 1] += 2
                break
        total -= 1
    lens, j = [0] * len(freq), n
    for l in range(1, limit + 1):
        for _ in range(count[l]):
            j -= 1
            lens[order[j]] = l
    if info is not None:
        info["max"] = max(lens)
    return lens


def canonical(lens) -> list:
    """RFC 1951 §3.2.2: (code, length) per symbol, the code bit-reversed for the LSB-first stream."""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = []
    for l in lens:
        if l == 0:
            out.append((0, 0))
            continue
        out.append((int(format(nxt[l], f"0{l}b")[::-1], 2), l))
        nxt[l] += 1
    return out


FIXED_LENS = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED = canonical(FIXED_LENS)[:286]


class BitSink:
    def __init__(self):
        self.out, self.acc, self.nb, self.bits = bytearray(), 0, 0, 0

    def put(self, value: int, length: int):
        self.acc |= value << self.nb
        self.nb += length
        self.bits += length
        while self.nb >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.nb -= 8

    def finish(self) -> bytes:
        if self.nb:
            self.out.append(self.acc & 255)     # padded with zero bits
        return bytes(self.out)


@dataclass
class Encoded:
    data: bytes
    f: bytes                                    # the filtered stream
    filters: list = field(default_factory=list)
    block_types: list = field(default_factory=list)    # BTYPE of every deflate block
    matches: list = field(default_factory=list)        # match lengths, in stream order
    payload: bytes = b""                        # the zlib stream
    chunk_bits: list = field(default_factory=list)
    lit_info: list = field(default_factory=list)       # per block: code_lengths' info for the literal/length code
    cl_info: list = field(default_factory=list)        # ... and for the code-length code


def dynamic_header(lens, has_match: bool, final: bool, info=None):
    """The header of a dynamic block as (value, bits) pairs.  No repeat symbols (16..18): every length is one
    symbol of the code-length code."""
    nlit = max(257, max(s for s in range(286) if lens[s]) + 1)
    seq = lens[:nlit] + [1 if has_match else 0]
    clfreq = [0] * 19
    for l in seq:
        clfreq[l] += 1
    cl = canonical(code_lengths(clfreq, 7, info))
    ncl = max(4, max(i for i in range(19) if cl[CL_ORDER[i]][1]) + 1)
    out = [(int(final), 1), (2, 2), (nlit - 257, 5), (0, 5), (ncl - 4, 4)]
    out += [(cl[CL_ORDER[i]][1], 3) for i in range(ncl)]
    out += [cl[l] for l in seq]
    return out


def encode(rgb: np.ndarray, filt: int = ADAPTIVE, block_bytes: int = BLOCK_DEFAULT, mirror_x: bool = False) -> Encoded:
    rgb = np.asarray(rgb)
    h, w = rgb.shape[:2]
    assert block_bytes % CHUNK == 0 and BLOCK_MIN <= block_bytes <= BLOCK_MAX
    fa, types = filtered(rgb, filt, mirror_x)
    f = fa.tobytes()
    n = len(f)
    enc = Encoded(b"", f, [int(t) for t in types])
    sink = BitSink()
    nblocks = -(-n // block_bytes)
    for b in range(nblocks):
        b0, b1 = b * block_bytes, min((b + 1) * block_bytes, n)
        chunks = [tokens_of(f, c0, min(c0 + CHUNK, b1)) for c0 in range(b0, b1, CHUNK)]
        freq = [0] * 286
        for toks in chunks:
            for t in toks:
                freq[t if t < 256 else LEN_SYM[t - 256][0]] += 1
        freq[256] = 1
        nmatch = sum(freq[257:])
        info, clinfo = {}, {}
        lens = code_lengths(freq, 15, info)
        enc.lit_info.append(info)
        enc.cl_info.append(clinfo)
        head = dynamic_header(lens, nmatch > 0, b == nblocks - 1, clinfo)
        dyn_bits = sum(l for _, l in head) + sum(freq[s] * (lens[s] + SYM_EXTRA[s]) for s in range(286)) + nmatch
        fix_bits = 3 + sum(freq[s] * (FIXED[s][1] + SYM_EXTRA[s]) for s in range(286)) + 5 * nmatch
        if dyn_bits < fix_bits:                 # ties go to fixed
            table, dist_bits = canonical(lens), 1
            enc.block_types.append(2)
        else:
            table, dist_bits, head = FIXED, 5, [(int(b == nblocks - 1), 1), (1, 2)]
            enc.block_types.append(1)
        for k, toks in enumerate(chunks):
            start = sink.bits
            if k == 0:
                for v, l in head:
                    sink.put(v, l)
            for t in toks:
                if t < 256:
                    sink.put(*table[t])
                else:
                    sym, eb, ev = LEN_SYM[t - 256]
                    sink.put(*table[sym])
                    sink.put(ev, eb)
                    sink.put(0, dist_bits)      # distance 1: symbol 0, whose code is all zeros in both codings
                    enc.matches.append(t - 256)
            if k == len(chunks) - 1:
                sink.put(*table[256])
            enc.chunk_bits.append(sink.bits - start)
        assert sink.bits <= 9 * b1 + 10 * (b + 1)
    payload = b"\x78\x01" + sink.finish() + struct.pack(">I", zlib.adler32(f))
    enc.payload = payload

    def chunk(tag: bytes, body: bytes) -> bytes:
        return struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body))

    enc.data = (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + chunk(b"IDAT", payload) +
                chunk(b"IEND", b""))
    assert len(enc.data) <= bound(w, h, block_bytes)
    return enc
