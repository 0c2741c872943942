"""Crafted inputs of the OpenEXR encoder's tests.  Each case says what it is for, and
tests/test_exr_enc_cpu.py asserts on the restatement (tests/exr_ref.py) that it gets there."""
from __future__ import annotations

import numpy as np

from tests import exr_ref as R

HALF_PLANE_W = 640


def _f32(bits) -> np.ndarray:
    return np.asarray(bits, np.uint32).view(np.float32)


def half_values() -> np.ndarray:
    """float32 values around every finite half h of both signs: h itself and its two float neighbours, the midpoint of
    h and the next half away from zero (a tie, which goes to the even half; beyond 65504 the next "half" is 2^16, so the
    midpoint is 65520, the first float that rounds to infinity) and that midpoint's two float neighbours.  Then +-0,
    float denormals, 65504, the float below 65520, 65520, FLT_MAX, the infinities, and quiet and signalling NaNs of both
    signs."""
    mag = np.arange(0, 0x7c00, dtype=np.uint16)
    h = mag.view(np.float16).astype(np.float64)                  # exact
    nxt = np.append(h[1:], 65536.0)
    mid = ((h + nxt) / 2).astype(np.float32)                     # 12 significant bits: exact
    assert (mid.astype(np.float64) == (h + nxt) / 2).all()
    hb, mb = h.astype(np.float32).view(np.uint32), mid.view(np.uint32)
    pos = np.concatenate([hb, hb + 1, hb[1:] - 1, mb, mb + 1, mb - 1])
    extra = [0x00000000, 0x00000001, 0x00400000, 0x007fffff, 0x00800000, 0x477fe000, 0x477fefff, 0x477ff000, 0x7f7fffff,
             0x7f800000, 0x7fc00000, 0x7f800001, 0x7fffffff, 0x7fc12345]
    pos = np.concatenate([pos, np.array(extra, np.uint32)])
    return _f32(np.concatenate([pos, pos | np.uint32(0x80000000)]))


def half_plane() -> np.ndarray:
    """half_values() laid out as one (H, HALF_PLANE_W) plane, zeros behind."""
    v = half_values()
    rows = -(-v.size // HALF_PLANE_W)
    out = np.zeros(rows * HALF_PLANE_W, np.float32)
    out.view(np.uint32)[:v.size] = v.view(np.uint32)
    return out.reshape(rows, HALF_PLANE_W)


def noise(w: int, h: int, seed: int = 0) -> np.ndarray:
    """Uniform values in 0..1 with random low bits: a chunk of them does not compress (the raw fallback)."""
    return np.random.default_rng(seed).random((h, w), dtype=np.float32)


def smooth(w: int, h: int) -> np.ndarray:
    """A ramp along x in steps of 1/8, the same in every row: long runs in both halves of the byte split."""
    return np.tile((np.arange(w) // 8).astype(np.float32) * np.float32(0.125), (h, 1))


def noise_and_constant(w: int = 200, h: int = 64) -> list:
    """Three FLOAT channels whose top half is noise (raw chunks) and whose bottom half is constant or smooth (compressed
    chunks), so that one file holds both kinds with ZIP (h a multiple of 32) and with ZIPS."""
    out = []
    for k, name in enumerate("RGB"):
        top = noise(w, h // 2, 10 + k)
        bottom = smooth(w, h - h // 2) if k == 1 else np.full((h - h // 2, w), 0.25 * (k + 1), np.float32)
        out.append((name, R.FLOAT, np.concatenate([top, bottom]), 1.0))
    return out


def mixed(w: int, h: int, seed: int) -> np.ndarray:
    """Rows of noise, of a constant and of a ramp in turn: literals and runs in one stream."""
    a = noise(w, h, seed)
    a[1::3] = np.float32(0.5)
    a[2::3] = smooth(w, h)[2::3]
    return a


NAMES16 = ["zeta", "B", "albedo.R", "N.X", "a", "Z", "id", "UV.V", "R", "G", "P.X", "albedo.G", "N.Y", "UV.U", "_x9", "A.b_c.d"]
TYPES16 = [R.FLOAT, R.HALF, R.HALF, R.FLOAT, R.UINT, R.FLOAT, R.UINT, R.HALF, R.FLOAT, R.HALF, R.FLOAT, R.HALF, R.FLOAT, R.HALF,
           R.FLOAT, R.HALF]


def channel_set(count: int, w: int, h: int, seed: int = 0) -> list:
    """1 (HALF), 3 (FLOAT) or 16 (mixed types) channels, the names unsorted: (name, type, plane, divisor).  A UINT plane holds
    random words (0xffffffff among them)."""
    sets = {1: (["Y"], [R.HALF]), 3: (["R", "G", "B"], [R.FLOAT, R.FLOAT, R.FLOAT]), 16: (NAMES16, TYPES16)}
    names, types = sets[count]
    out = []
    for k, (n, t) in enumerate(zip(names, types)):
        if t == R.UINT:
            pl = np.random.default_rng(seed + 100 + k).integers(0, 4, (h, w), dtype=np.uint32) * np.uint32(0x55555555)
            pl.reshape(-1)[0] = 0xffffffff
            pl = pl.view(np.float32)
        else:
            pl = mixed(w, h, seed + k)
        out.append((n, t, pl, 1.0))
    return out


def stream_sizes(max_w: int = 6, max_lines: int = 16) -> set:
    """Every n that small images reach: lines * W * (the channels' sizes)."""
    sizes = set()
    for w in range(1, max_w + 1):
        for lines in range(1, max_lines + 1):
            for halfs in range(0, 4):
                for floats in range(0, 4):
                    if halfs + floats:
                        sizes.add(lines * w * (2 * halfs + 4 * floats))
    return sizes
