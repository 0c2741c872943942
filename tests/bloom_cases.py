"""Inputs of the bloom tests (test_bloom_cpu.py, test_bloom_gpu.py): small images that reach every path."""
from __future__ import annotations

import numpy as np

F = np.float32

# widths and heights on both sides of a lane's pixels, a wave and the tile edges of 16, 32 and 64; 700 x 500 is beyond one
# sweep of a grid of 256 workgroups
SIZES = [(1, 1), (2, 1), (3, 2), (5, 7), (15, 17), (16, 16), (17, 15), (31, 33), (33, 31), (63, 65), (65, 33), (129, 67),
         (257, 5), (700, 500)]
# the float64 comparison's (width, height, levels): the default K and the one beside it where the size allows both
SIZES_64 = [(1, 1, 0), (2, 1, 0), (5, 7, 0), (65, 33, 0), (65, 33, 6), (130, 67, 0), (130, 67, 5)]
# (threshold, strength, spread) beside the defaults: threshold 0, spread 1; the third test case takes its threshold from a pixel
TRIPLES = [(0.0, 0.5, 0.75), (0.5, 1.0, 1.0)]

CLAMP = F(65504.0)
EDGE = np.array([0.0, -0.0, 1e-41, np.nan, np.inf, -np.inf, -3.5, CLAMP, np.nextafter(CLAMP, F(0)), 1e30], np.float32)


def noisy(w: int, h: int, seed: int = 0, lo: float = -6.0, hi: float = 6.0) -> np.ndarray:
    """(h, w, 3) float32, non-negative: 2^uniform(lo, hi), every pixel's channels drawn on their own."""
    rng = np.random.default_rng(1000 * seed + 7 * w + h)
    return np.exp2(rng.uniform(lo, hi, (h, w, 3))).astype(np.float32)


def edge_image(seed: int = 0) -> np.ndarray:
    """9 rows of 3 * len(EDGE) pixels: the first, the middle and the last row hold every value of EDGE in every
    channel (pixel 3 i + ch has EDGE[i] in channel ch), the rest is noise."""
    w = 3 * EDGE.size
    img = noisy(w, 9, seed, -3.0, 4.0)
    for y in (0, 4, 8):
        for i, v in enumerate(EDGE):
            for ch in range(3):
                img[y, 3 * i + ch, ch] = v
    return img


def constant(w: int, h: int, rgb=(0.5, 1.25, 3.0)) -> np.ndarray:
    """One colour whose channels have short significands: every sum and every product by 3 of the filters is exact."""
    return np.broadcast_to(np.array(rgb, np.float32), (h, w, 3)).copy()
