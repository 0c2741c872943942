"""Inputs of the display transform's tests (test_display_cpu.py, test_display_gpu.py): accumulators as (H, W, 3)
float32 arrays."""
from __future__ import annotations

import numpy as np

F = np.float32

# Widths on both sides of a lane's four pixels and of a wave, several workgroups, and one size beyond a single sweep
# of the kernels' grid (256 workgroups x 256 lanes x 4 pixels = 262144 pixels).
SIZES = [(1, 1), (3, 1), (4, 1), (5, 2), (7, 3), (64, 1), (65, 3), (257, 5), (700, 500)]


def noisy(w: int, h: int, seed: int = 0, lo: float = -20.0, hi: float = 20.0) -> np.ndarray:
    """Radiance spanning 2^lo .. 2^hi, every channel on its own."""
    rng = np.random.default_rng([seed, w, h])
    return np.exp2(rng.uniform(lo, hi, (h, w, 3))).astype(np.float32)


def edge_values() -> np.ndarray:
    p16, p_16 = F(2.0 ** 16), F(2.0 ** -16)
    return np.array([0.0, -0.0, 1e-41, p_16, np.nextafter(p_16, F(0)), 0.18, 1.0, p16, np.nextafter(p16, F(0)),
                     np.finfo(np.float32).max, np.inf, -np.inf, np.nan, -0.75], np.float32)


def edge_row() -> np.ndarray:
    """(56, 3): every edge value in each channel position beside 0.25, and in all three at once."""
    vals = edge_values()
    px = []
    for v in vals:
        for k in range(3):
            p = np.full(3, 0.25, np.float32)
            p[k] = v
            px.append(p)
        px.append(np.full(3, v, np.float32))
    return np.array(px, np.float32)


EDGE_W, EDGE_H = 61, 5


def edge_image(seed: int = 7) -> np.ndarray:
    """61 x 5, noise with the edge row as its first, middle and last row (the row's last 5 pixels stay noise)."""
    img = noisy(EDGE_W, EDGE_H, seed, -4.0, 4.0)
    row = edge_row()
    for y in (0, EDGE_H // 2, EDGE_H - 1):
        img[y, :row.shape[0]] = row
    return img


def one_colour(w: int, h: int, rgb=(0.3, 0.5, 0.2)) -> np.ndarray:
    return np.broadcast_to(np.array(rgb, np.float32), (h, w, 3)).copy()


def black(w: int, h: int) -> np.ndarray:
    return np.zeros((h, w, 3), np.float32)


def stepped(w: int, h: int, seed: int = 3) -> np.ndarray:
    """A mid-range image for the exposure tests: luminance within 2^-3 .. 2^3."""
    return noisy(w, h, seed, -3.0, 3.0)
