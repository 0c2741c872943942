"""The OpenEXR file of the device encoder (csrc/pt_exr_enc.hip), from DESIGN.md §18 alone, in two independent halves.

(a) read_exr(data): a reader.  It parses the header generically, checks the offset table against the chunks' positions,
    inflates compressed chunks with zlib.decompress, undoes the differences and the byte split, and returns the channels.
(b) encode(...): the byte-exact restatement of the writer.  A chunk's stream is §15's run-length deflate; its token rule,
    code-length construction, canonical codes and block header are tests/png_enc_ref.py's, by import.  encode(slow=True)
    tokenises with png_enc_ref.tokens_of and writes bit by bit; the default does the same steps on numpy arrays (runs of
    "equals the previous byte" cut at the lane chunks, one bit-packing call), because the GPU tests' sizes are millions of
    bytes.  tests/test_exr_enc_cpu.py asserts that the two give the same files.
"""
from __future__ import annotations

import struct
import zlib
from dataclasses import dataclass, field

import numpy as np

from tests.png_enc_ref import (CHUNK, FIXED, LEN_SYM, SYM_EXTRA, BitSink, canonical, code_lengths, dynamic_header, tokens_of)

UINT, HALF, FLOAT = 0, 1, 2
NONE, ZIPS, ZIP = 0, 2, 3
MAGIC = bytes([0x76, 0x2f, 0x31, 0x01, 2, 0, 0, 0])
BLOCK_DEFAULT = 32768
LINES = {NONE: 1, ZIPS: 1, ZIP: 16}


# ---- values -----------------------------------------------------------------------------------------------
def half_bits(f32_bits) -> np.ndarray:
    """§18's HALF from the bits of float32 values, in integers: round to nearest even, subnormal halves, overflow to
    infinity, NaN to sign | 0x7e00."""
    f = np.asarray(f32_bits, np.uint32).astype(np.int64)
    sign, a = (f >> 16) & 0x8000, f & 0x7fffffff
    out = np.zeros(f.shape, np.int64)
    nan, inf = a > 0x7f800000, (a >= 0x477ff000) & (a <= 0x7f800000)
    normal = (a >= 0x38800000) & (a < 0x477ff000)
    sub = (a > 0x33000000) & (a < 0x38800000)
    out[nan] = 0x7e00
    out[inf] = 0x7c00
    v = a - 0x38000000
    out[normal] = ((v + 0xfff + ((v >> 13) & 1)) >> 13)[normal]
    shift = np.clip(126 - (a >> 23), 14, 24)
    mant = (a & 0x7fffff) | 0x800000
    m, rem, halfway = mant >> shift, mant & ((1 << shift) - 1), 1 << (shift - 1)
    out[sub] = (m + ((rem > halfway) | ((rem == halfway) & ((m & 1) == 1))))[sub]
    return (sign | out).astype(np.uint16)


def value_bytes(plane: np.ndarray, typ: int, divisor: float = 1.0) -> np.ndarray:
    """(H, W) plane words -> (H, W * size) bytes of the channel's values, little-endian."""
    words = np.ascontiguousarray(plane).view(np.uint32)
    if typ != UINT and np.float32(divisor) != np.float32(1):
        with np.errstate(all="ignore"):
            words = (words.view(np.float32) / np.float32(divisor)).view(np.uint32)   # one float32 division
    if typ == HALF:
        return half_bits(words).astype("<u2").view(np.uint8).reshape(words.shape[0], -1)
    return words.astype("<u4").view(np.uint8).reshape(words.shape[0], -1)


# ---- header -----------------------------------------------------------------------------------------------
def header(width: int, height: int, channels, compression: int) -> bytes:
    """channels: (name, type) pairs in any order."""
    def attr(name, typ, value):
        return name.encode() + b"\0" + typ.encode() + b"\0" + struct.pack("<i", len(value)) + value
    chl = b"".join(n.encode() + b"\0" + struct.pack("<iB3xii", t, 0, 1, 1) for n, t in sorted(channels, key=lambda c: c[0].encode()))
    box = struct.pack("<4i", 0, 0, width - 1, height - 1)
    return (MAGIC + attr("channels", "chlist", chl + b"\0") + attr("compression", "compression", bytes([compression])) +
            attr("dataWindow", "box2i", box) + attr("displayWindow", "box2i", box) + attr("lineOrder", "lineOrder", b"\0") +
            attr("pixelAspectRatio", "float", struct.pack("<f", 1.0)) + attr("screenWindowCenter", "v2f", struct.pack("<2f", 0, 0)) +
            attr("screenWindowWidth", "float", struct.pack("<f", 1.0)) + b"\0")


def bound(width: int, height: int, channels, compression: int) -> int:
    """pt_exr_enc_bound: the NONE file, header + 8 chunks + sum (8 + n)."""
    chunks = -(-height // LINES[compression])
    line = width * sum(2 if t == HALF else 4 for _, t in channels)
    return len(header(width, height, channels, compression)) + 8 * chunks + 8 * chunks + height * line


# ---- a chunk's stream -------------------------------------------------------------------------------------
def preprocess(r: bytes) -> bytes:
    """§18 step 5.1 and 5.2: even bytes then odd bytes, then differences of neighbours + 128."""
    a = np.frombuffer(r, np.uint8)
    t = np.concatenate([a[0::2], a[1::2]]).astype(np.int64)
    p = t.copy()
    p[1:] = (t[1:] - t[:-1] + 128) & 255
    return p.astype(np.uint8).tobytes()


def unpreprocess(p: bytes) -> bytes:
    t = np.cumsum(np.frombuffer(p, np.uint8).astype(np.int64) - 128) + 128   # t[i] = p[0] + sum (p[k] - 128)
    t = (t & 255).astype(np.uint8)
    n, half = len(t), (len(t) + 1) // 2
    r = np.empty(n, np.uint8)
    r[0::2], r[1::2] = t[:half], t[half:]
    return r.tobytes()


def _block_code(freq, final: bool):
    """The code of one deflate block from its symbol counts (freq[256] = 1): table of (code, length), the bits of a
    distance, the header as (value, bits) pairs, the block type."""
    nmatch = sum(freq[257:])
    lens = code_lengths(freq, 15)
    head = dynamic_header(lens, nmatch > 0, final)
    dyn = sum(l for _, l in head) + sum(freq[s] * (lens[s] + SYM_EXTRA[s]) for s in range(286)) + nmatch
    fix = 3 + sum(freq[s] * (FIXED[s][1] + SYM_EXTRA[s]) for s in range(286)) + 5 * nmatch
    if dyn < fix:                               # ties go to fixed
        return canonical(lens), 1, head, 2
    return FIXED, 5, [(int(final), 1), (1, 2)], 1


def deflate_slow(p: bytes, block_bytes: int):
    """The zlib stream of p, token by token (png_enc_ref.encode's loop on one stream), and its block types."""
    n, sink, types = len(p), BitSink(), []
    nblocks = -(-n // block_bytes)
    for b in range(nblocks):
        b0, b1 = b * block_bytes, min((b + 1) * block_bytes, n)
        chunks = [tokens_of(p, c0, min(c0 + CHUNK, b1)) for c0 in range(b0, b1, CHUNK)]
        freq = [0] * 286
        for toks in chunks:
            for t in toks:
                freq[t if t < 256 else LEN_SYM[t - 256][0]] += 1
        freq[256] = 1
        table, dist_bits, head, typ = _block_code(freq, b == nblocks - 1)
        types.append(typ)
        for v, l in head:
            sink.put(v, l)
        for toks in chunks:
            for t in toks:
                if t < 256:
                    sink.put(*table[t])
                else:
                    sym, eb, ev = LEN_SYM[t - 256]
                    sink.put(*table[sym])
                    sink.put(ev, eb)
                    sink.put(0, dist_bits)
        sink.put(*table[256])
    return b"\x78\x01" + sink.finish() + struct.pack(">I", zlib.adler32(p)), types


_K_SYM = np.zeros(259, np.int64)
_K_EB = np.zeros(259, np.int64)
_K_EV = np.zeros(259, np.int64)
for _k, (_s, _eb, _ev) in LEN_SYM.items():
    _K_SYM[_k], _K_EB[_k], _K_EV[_k] = _s, _eb, _ev


def _tokens_fast(p: np.ndarray):
    """tokens_of over every lane chunk of p at once: positions and token values (a literal 0..255, a match 256 + k), in
    stream order.  A match at i is a run of bytes equal to byte i - 1; such runs are the maximal runs of "equals the
    previous byte", cut where a lane chunk starts; a run of m bytes is m // 258 matches of 258 and a rest that is one match
    (>= 3) or literals."""
    n = len(p)
    eq = np.zeros(n, bool)
    eq[1:] = p[1:] == p[:-1]
    idx = np.flatnonzero(eq)
    lit = ~eq
    mpos, mlen = np.zeros(0, np.int64), np.zeros(0, np.int64)
    if idx.size:
        brk = np.ones(idx.size, bool)
        brk[1:] = (idx[1:] != idx[:-1] + 1) | (idx[1:] % CHUNK == 0)
        starts, m = idx[brk], np.bincount(np.cumsum(brk) - 1)
        q, r = m // 258, m % 258
        # the rest: literals where it is shorter than 3
        short = np.flatnonzero(r < 3)
        for d in (0, 1):
            sel = short[r[short] > d]
            lit[starts[sel] + 258 * q[sel] + d] = True
        full = np.repeat(starts, q) + 258 * (np.arange(q.sum()) - np.repeat(np.cumsum(q) - q, q))
        rest = r >= 3
        mpos = np.concatenate([full, starts[rest] + 258 * q[rest]])
        mlen = np.concatenate([np.full(full.size, 258, np.int64), r[rest]])
    lpos = np.flatnonzero(lit)
    pos = np.concatenate([lpos, mpos])
    tok = np.concatenate([p[lpos].astype(np.int64), 256 + mlen])
    order = np.argsort(pos, kind="stable")
    return pos[order], tok[order]


def _pack_bits(vals: np.ndarray, nbs: np.ndarray) -> bytes:
    """The values' low nbs bits, LSB first, one after the other; zero bits up to a whole byte."""
    total = int(nbs.sum())
    starts = np.cumsum(nbs) - nbs
    j = np.arange(total) - np.repeat(starts, nbs)
    bits = ((np.repeat(vals, nbs) >> j) & 1).astype(np.uint8)
    return np.packbits(bits, bitorder="little").tobytes()


def deflate_fast(p: bytes, block_bytes: int, limit: int | None = None):
    """deflate_slow's stream on arrays.  limit: a stream of at least that many bytes is not written out (None for it):
    the caller falls back to the raw bytes."""
    a = np.frombuffer(p, np.uint8)
    n = len(a)
    nblocks = -(-n // block_bytes)
    pos, tok = _tokens_fast(a)
    blk = pos // block_bytes
    is_m = tok >= 256
    k = np.where(is_m, tok - 256, 0)
    sym = np.where(is_m, _K_SYM[k], tok)
    freq = np.bincount(blk * 286 + sym, minlength=nblocks * 286).reshape(nblocks, 286)
    freq[:, 256] = 1
    first = np.searchsorted(blk, np.arange(nblocks + 1))
    vals, nbs, types, bits = [], [], [], 0
    for b in range(nblocks):
        table, dist_bits, head, typ = _block_code([int(v) for v in freq[b]], b == nblocks - 1)
        types.append(typ)
        code = np.array([c for c, _ in table], np.int64)
        clen = np.array([l for _, l in table], np.int64)
        s, kk, m = sym[first[b]:first[b + 1]], k[first[b]:first[b + 1]], is_m[first[b]:first[b + 1]]
        v = code[s] | np.where(m, _K_EV[kk] << clen[s], 0)      # the symbol, its extra bits, the distance's zeros
        l = clen[s] + np.where(m, _K_EB[kk] + dist_bits, 0)
        vals += [np.array([x for x, _ in head], np.int64), v, code[256:257]]
        nbs += [np.array([x for _, x in head], np.int64), l, clen[256:257]]
        bits += sum(x for _, x in head) + int(l.sum()) + int(clen[256])
    z = 2 + (bits + 7) // 8 + 4
    if limit is not None and z >= limit:
        return None, types, z
    return b"\x78\x01" + _pack_bits(np.concatenate(vals), np.concatenate(nbs)) + struct.pack(">I", zlib.adler32(p)), types, z


def raw_fallback(z: int, n: int) -> bool:
    """§18: a stream of z bytes for n raw bytes is dropped for the raw bytes when z >= n."""
    return z >= n


# ---- the file ---------------------------------------------------------------------------------------------
@dataclass
class Encoded:
    data: bytes
    raw: list = field(default_factory=list)         # per chunk: stored as raw bytes
    n: list = field(default_factory=list)           # per chunk: raw bytes
    z: list = field(default_factory=list)           # per chunk: the stream's length (0 for NONE)
    p: list = field(default_factory=list)           # per chunk: the preprocessed bytes (ZIP, ZIPS)
    payload: list = field(default_factory=list)     # per chunk: the data as stored
    block_types: list = field(default_factory=list)


def encode(channels, compression: int = ZIP, block_bytes: int = BLOCK_DEFAULT, mirror_x: bool = False, slow: bool = False) -> Encoded:
    """channels: (name, type, (H, W) plane, divisor) in any order."""
    chans = sorted(channels, key=lambda c: c[0].encode())
    h, w = np.asarray(chans[0][2]).shape
    rows = [value_bytes(np.asarray(pl)[:, ::-1] if mirror_x else np.asarray(pl), t, d) for _, t, pl, d in chans]
    lines = np.concatenate(rows, axis=1)            # (H, bytes of a scanline): the channels' rows one after the other
    L = LINES[compression]
    enc = Encoded(b"")
    for y0 in range(0, h, L):
        r = lines[y0:y0 + L].tobytes()
        enc.n.append(len(r))
        if compression == NONE:
            enc.raw.append(True), enc.z.append(0), enc.payload.append(r)
            continue
        p = preprocess(r)
        if slow:
            stream, types = deflate_slow(p, block_bytes)
            z = len(stream)
        else:
            stream, types, z = deflate_fast(p, block_bytes, len(r))
        enc.p.append(p), enc.z.append(z), enc.block_types.append(types)
        enc.raw.append(raw_fallback(z, len(r)))
        enc.payload.append(r if enc.raw[-1] else stream)
    head = header(w, h, [(n, t) for n, t, _, _ in chans], compression)
    at, table, body = len(head) + 8 * len(enc.payload), [], []
    for k, data in enumerate(enc.payload):
        table.append(struct.pack("<Q", at))
        body.append(struct.pack("<ii", k * L, len(data)) + data)
        at += 8 + len(data)
    enc.data = head + b"".join(table) + b"".join(body)
    assert len(enc.data) <= bound(w, h, [(n, t) for n, t, _, _ in chans], compression)
    return enc


# ---- the reader -------------------------------------------------------------------------------------------
def read_header(data: bytes):
    """The attributes as {name: (type, value bytes)} and the header's length."""
    assert data[:4] == MAGIC[:4] and data[4:8] == MAGIC[4:], "magic or version"
    at, attrs = 8, {}
    while data[at] != 0:
        e = data.index(b"\0", at)
        name, at = data[at:e].decode(), e + 1
        e = data.index(b"\0", at)
        typ, at = data[at:e].decode(), e + 1
        size = struct.unpack_from("<i", data, at)[0]
        attrs[name] = (typ, data[at + 4:at + 4 + size])
        at += 4 + size
    return attrs, at + 1


def read_exr(data: bytes, info: dict | None = None) -> dict:
    """{name: (H, W) array}: HALF as float16, FLOAT as float32, UINT as uint32.  info: gets "raw", per chunk whether it
    was stored as raw bytes, and "attrs"."""
    attrs, at = read_header(data)
    chl, chans, c = attrs["channels"][1], [], 0
    assert attrs["channels"][0] == "chlist"
    while chl[c] != 0:
        e = chl.index(b"\0", c)
        typ, plinear, xs, ys = struct.unpack_from("<iB3xii", chl, e + 1)
        assert (plinear, xs, ys) == (0, 1, 1)
        chans.append((chl[c:e].decode(), typ))
        c = e + 17
    assert c == len(chl) - 1 and [n for n, _ in chans] == sorted((n for n, _ in chans), key=str.encode)
    comp = attrs["compression"][1][0]
    x0, y0, x1, y1 = struct.unpack("<4i", attrs["dataWindow"][1])
    assert (x0, y0) == (0, 0) and attrs["displayWindow"] == attrs["dataWindow"] and attrs["lineOrder"][1] == b"\0"
    w, h, L = x1 + 1, y1 + 1, LINES[comp]
    nchunks = -(-h // L)
    table = struct.unpack_from(f"<{nchunks}Q", data, at)
    at += 8 * nchunks
    size = {UINT: 4, HALF: 2, FLOAT: 4}
    dtype = {UINT: "<u4", HALF: "<f2", FLOAT: "<f4"}
    line = w * sum(size[t] for _, t in chans)
    out = {n: np.empty((h, w), np.dtype(dtype[t]).newbyteorder("=")) for n, t in chans}
    raws = []
    for k in range(nchunks):
        assert table[k] == at, "the offset table and the chunks' positions differ"
        y, dsize = struct.unpack_from("<ii", data, at)
        assert y == k * L
        body = data[at + 8:at + 8 + dsize]
        assert len(body) == dsize
        at += 8 + dsize
        nl = min(L, h - y)
        n = nl * line
        raws.append(dsize == n)
        if comp != NONE and dsize != n:
            assert dsize < n
            body = unpreprocess(zlib.decompress(body))
        assert len(body) == n
        o = 0
        for ly in range(nl):
            for name, t in chans:
                out[name][y + ly] = np.frombuffer(body, dtype[t], w, o)
                o += w * size[t]
    assert at == len(data), "bytes behind the last chunk"
    if info is not None:
        info["raw"], info["attrs"] = raws, attrs
    return out
