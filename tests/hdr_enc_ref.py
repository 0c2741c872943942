"""TEST INFRASTRUCTURE ONLY: the device Radiance HDR encoder's definition restated in vectorised
numpy, in the formulation the kernels use: segment starts, lengths and classes, per-byte contributions and a cumsum,
with no sequential walk over a row.  A mistake in the rule therefore shows on the CPU, against the line-by-line
restatement of the reference's writer (oracle/hdr_oracle.py) and against the host library (encode_hdr)."""
from __future__ import annotations

import numpy as np


def header(w: int, h: int) -> bytes:
    return (b"#?RADIANCE\n# Written by stb_image_write.h\nFORMAT=32-bit_rle_rgbe\n"
            + f"EXPOSURE=          1.0000000000000\n\n-Y {h} +X {w}\n".encode())


def is_flat(w: int) -> bool:
    return w < 8 or w >= 32768


def row_bound(w: int) -> int:
    """A coded plane row takes at most W + ceil(W / 128) bytes."""
    return w + (w + 127) // 128


def bound(w: int, h: int) -> int:
    """pt_hdr_enc_bound."""
    return len(header(w, h)) + (4 * w * h if is_flat(w) else h * (4 + 4 * row_bound(w)))


def code_rows(rows: np.ndarray) -> tuple:
    """Every row of an (N, W) uint8 array coded by the segment rule; returns (the coded bytes of all rows, one
    after the other, and the N lengths).

    Maximal segments of equal bytes; a segment of length >= 3 is a run, every other byte a literal; a stretch is a
    maximal interval of literals.  A literal at offset j of a stretch of n contributes its byte, preceded by the
    count byte min(128, n - j) where j % 128 == 0; a run byte at offset j of a segment of n contributes
    {128 + min(127, n - j), value} where j % 127 == 0 and nothing otherwise; a byte's position is the exclusive
    prefix sum of the contributions."""
    rows = np.ascontiguousarray(rows, np.uint8)
    n_rows, w = rows.shape
    c = rows.reshape(-1)
    total = c.size
    at = np.arange(total)
    first = at % w == 0
    start = first.copy()
    start[1:] |= c[1:] != c[:-1]
    seg_at = np.flatnonzero(start)
    seg_len = np.diff(np.append(seg_at, total))
    seg = np.cumsum(start) - 1
    j, n = at - seg_at[seg], seg_len[seg]
    run = n >= 3
    lit = ~run
    before_run = np.concatenate(([True], run[:-1]))
    st_start = lit & (first | before_run)
    st_at = np.flatnonzero(st_start)
    sid = np.cumsum(st_start) - 1
    sj, sn = np.zeros(total, np.int64), np.zeros(total, np.int64)
    if st_at.size:
        st_len = np.bincount(sid[lit], minlength=st_at.size)
        sj[lit] = at[lit] - st_at[sid[lit]]
        sn[lit] = st_len[sid[lit]]
    lit_head, run_head = lit & (sj % 128 == 0), run & (j % 127 == 0)
    contrib = np.where(run, np.where(run_head, 2, 0), 1 + lit_head)
    pos = np.cumsum(contrib) - contrib
    out = np.zeros(int(contrib.sum()), np.uint8)
    out[(pos + lit_head)[lit]] = c[lit]
    out[pos[lit_head]] = np.minimum(128, sn - sj)[lit_head]
    out[pos[run_head]] = (128 + np.minimum(127, n - j))[run_head]
    out[pos[run_head] + 1] = c[run_head]
    return out, np.add.reduceat(contrib, np.arange(0, total, w))


def code_row(row) -> bytes:
    return code_rows(np.asarray(row, np.uint8).reshape(1, -1))[0].tobytes()


def tokens(coded: bytes) -> list:
    """[("run", n, value) | ("lit", n)] of one coded plane row."""
    out, i = [], 0
    while i < len(coded):
        b = coded[i]
        if b > 128:
            out.append(("run", b - 128, coded[i + 1]))
            i += 2
        else:
            assert b > 0
            out.append(("lit", b))
            i += 1 + b
    assert i == len(coded)
    return out


def host_u8(x: np.ndarray) -> np.ndarray:
    """What the host library's x86 code makes of to_rgbe's (uint8_t)(float) in R and G, given the truncation x
    (int32): two unsigned-saturating packs of signed 16-bit words, each half of the int32 on its own (B goes
    through a scalar conversion and keeps the truncation's low byte).  x in 0..255 (every component that is not
    negative) stays x; a negative x down to -32768 gives 0.  C++ leaves the conversion of a value outside 0..255
    undefined, so this is pinned against encode_hdr, not derived."""
    x = np.asarray(x, np.int32)
    b0 = np.clip(x.astype(np.int16).astype(np.int32), 0, 255)
    b1 = np.clip(x >> 16, 0, 255)
    return np.where(b1 >= 128, 0, np.where(b1 > 0, 255, b0)).astype(np.uint8)


def rgbe(acc: np.ndarray, samples: float) -> np.ndarray:
    """to_rgbe (pt_image.cpp) of every pixel of acc / samples: (..., 4) uint8.  Finite values whose scaled components
    stay below 2^31 in magnitude."""
    lin = np.asarray(acc, np.float32) / np.float32(samples)
    r, g, b = lin[..., 0], lin[..., 1], lin[..., 2]
    m = np.where(g > b, g, b)
    mx = np.where(r > m, r, m)
    zero = mx.astype(np.float64) < 1e-32
    safe = np.where(zero, np.float32(1.0), mx)
    mant, e = np.frexp(safe.astype(np.float64))
    scale = (mant.astype(np.float32) * np.float32(256.0)) / safe
    out = np.empty(lin.shape[:-1] + (4,), np.uint8)
    with np.errstate(over="ignore", invalid="ignore"):
        x = (lin * scale[..., None]).astype(np.float32).astype(np.int32)
        out[..., 0], out[..., 1], out[..., 2] = host_u8(x[..., 0]), host_u8(x[..., 1]), (x[..., 2] & 255).astype(np.uint8)
    out[..., 3] = ((e + 128) & 255).astype(np.uint8)
    out[zero] = 0
    return out


def encode_planes(px: np.ndarray) -> bytes:
    """The file of an (H, W, 4) uint8 RGBE image, columns as given."""
    h, w = px.shape[:2]
    if is_flat(w):
        return header(w, h) + px.tobytes()
    coded, lens = code_rows(np.ascontiguousarray(px.transpose(0, 2, 1)).reshape(4 * h, w))
    ends = np.cumsum(lens)
    marker = bytes([2, 2, (w >> 8) & 255, w & 255])
    parts = [header(w, h)]
    for y in range(h):
        parts.append(marker)
        parts.append(coded[ends[4 * y] - lens[4 * y]:ends[4 * y + 3]].tobytes())
    return b"".join(parts)


def encode(acc: np.ndarray, samples: float, mirror_x: bool = True) -> bytes:
    """The device encoder's file; mirror_x=True is pt_encode_hdr's."""
    px = rgbe(acc, samples)
    return encode_planes(px[:, ::-1] if mirror_x else px)
