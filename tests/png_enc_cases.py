"""The images the PNG encoder's tests share (tests/test_png_enc_cpu.py checks the restatement's files of them,
tests/test_png_enc_gpu.py compares the device's files with those): name -> (image, filter, block_bytes)."""
from __future__ import annotations

import functools
from pathlib import Path

import numpy as np

from tests import png_enc_ref as R

SIZES = [(1, 1), (2, 1), (7, 5), (17, 9), (64, 48)]
FILTERS = [0, 1, 2, 3, 4, R.ADAPTIVE]
BLOCKS = [R.BLOCK_MIN, R.BLOCK_DEFAULT]
GOLDEN = Path(__file__).resolve().parent / "golden" / "REFERENCE_cornell.5000samp.png"


def noisy(w: int, h: int, seed: int = 0, chans: int = 3) -> np.ndarray:
    """A gradient with noise: every filter type wins some row, and short runs occur."""
    rng = np.random.default_rng(7 * w + h + seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([x * 255 // max(w - 1, 1), y * 255 // max(h - 1, 1), (x + y) * 255 // max(w + h - 2, 1)], -1)
    img = np.clip(base + rng.integers(-6, 7, (h, w, 3)) * (rng.random((h, w, 1)) < 0.5), 0, 255).astype(np.uint8)
    if chans == 4:
        img = np.concatenate([img, rng.integers(0, 256, (h, w, 1), dtype=np.uint8)], -1)   # alpha: ignored
    return img


def fibonacci_row() -> np.ndarray:
    """One row whose literal counts are the Fibonacci numbers 2, 3, 5, ... (18 byte values, the last padded to a
    whole pixel; the filter byte 0 and the end-of-block symbol are the two 1s before them), no two equal bytes
    adjacent: an unrestricted Huffman code is one chain, 19 deep."""
    fib = [2, 3]
    while len(fib) < 18:
        fib.append(fib[-1] + fib[-2])
    fib[-1] += -sum(fib) % 3
    n = sum(fib)
    row = np.zeros(n, np.uint8)
    order = np.concatenate([np.full(c, 1 + k, np.uint8) for k, c in sorted(enumerate(fib), key=lambda kc: -kc[1])])
    row[0::2] = order[:(n + 1) // 2]      # the most frequent value first on the even places, the rest on the odd ones
    row[1::2] = order[(n + 1) // 2:]
    assert (row[1:] != row[:-1]).all() and n + 1 <= R.BLOCK_DEFAULT
    return row.reshape(1, n // 3, 3)


def code_length_7_row() -> np.ndarray:
    """The same for the code-length code.  A byte value that occurs 2^(15 - L) times gets a code of L bits when the
    counts (with the end-of-block symbol's 1) sum to 2^15, so the number of codes of every length can be chosen:
    CODES_PER_LENGTH (found by a random search over complete codes) and the 84 zero lengths give the code-length
    alphabet the counts 84, 1, 5, 12, 3, 7, 13, 10, 10, 1, 9, 1, 102, whose unrestricted Huffman code is 9 deep.
    One row of 32766 bytes behind the filter byte 0 (which is one of value 0's occurrences): one deflate block."""
    lengths = [L for L, m in enumerate(CODES_PER_LENGTH) for _ in range(m)][:-1]    # (the last 15 is end-of-block's)
    counts = [1 << (15 - L) for L in lengths]
    counts[0] -= 1
    n = sum(counts)
    assert n == 32766 and len(counts) == 173
    order = np.concatenate([np.full(c, v, np.uint8) for v, c in enumerate(counts)])   # (counts descend)
    row = np.zeros(n, np.uint8)
    row[0::2] = order[:(n + 1) // 2]
    row[1::2] = order[(n + 1) // 2:]
    assert (row[1:] != row[:-1]).all()
    return row.reshape(1, n // 3, 3)


CODES_PER_LENGTH = [0, 0, 0, 1, 5, 12, 3, 7, 13, 10, 10, 1, 9, 0, 1, 102]


def accumulator() -> np.ndarray:
    """An (8, 33, 3) accumulator of 3 samples: negatives, values above 1, and every k / 255 with both of its float
    neighbours, the places where a wrong rounding or clamp in either conversion would show."""
    k = np.arange(256, dtype=np.float32) / np.float32(255)
    vals = np.concatenate([k, np.nextafter(k, np.float32(-1)), np.nextafter(k, np.float32(2)),
                           np.float32([-1.0, -0.0, 1.5, 1e30, 3e-8, 0.999999])]).astype(np.float32) * np.float32(3)
    return np.resize(vals, (8, 33, 3)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def golden_200() -> np.ndarray:
    from PIL import Image
    return np.ascontiguousarray(np.asarray(Image.open(GOLDEN))[::4, ::4, :3])


@functools.lru_cache(maxsize=None)
def golden_800() -> np.ndarray:
    from PIL import Image
    return np.ascontiguousarray(np.asarray(Image.open(GOLDEN))[..., :3])


def crafted() -> dict:
    rng = np.random.default_rng(11)
    low = rng.integers(0, 16, (48, 64, 3), dtype=np.uint8)
    return {
        # F is all zeros: 3630 bytes = 7 chunks and a part, 3 deflate blocks of 1024 and a part
        "constant": (np.zeros((30, 40, 3), np.uint8), 0, R.BLOCK_MIN),
        "random": (rng.integers(0, 256, (48, 64, 3), dtype=np.uint8), 0, R.BLOCK_DEFAULT),
        "one_pixel": (np.array([[[200, 100, 50]]], np.uint8), R.ADAPTIVE, R.BLOCK_DEFAULT),
        # 16 byte values: dynamic blocks of 1024 bytes, and a last block of 48 bytes that is cheaper fixed
        "both_types": (low, 0, R.BLOCK_MIN),
        "fibonacci": (fibonacci_row(), 0, R.BLOCK_DEFAULT),
        "code_length_7": (code_length_7_row(), 0, R.BLOCK_DEFAULT),
    }


@functools.lru_cache(maxsize=None)
def reference(name: str):
    """The restatement's file of a crafted case, computed once."""
    img, filt, block = crafted()[name]
    return R.encode(img, filt, block)
