"""The bloom restated in numpy: the yardstick of test_bloom_cpu.py and test_bloom_gpu.py.  Written
from the definition, one float32 operation per written operation, whole arrays at a time; the gain is Python
doubles.  Beside it the same definition in float64 built differently (dense matrices), for the error bound.
Imports nothing from the package."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

F = np.float32


@dataclass
class Params:
    threshold: float = 1.0
    strength: float = 0.25
    spread: float = 0.75
    clamp: float = 65504.0
    levels: int = 0


def levels_of(w: int, h: int, levels: int = 0) -> int:
    if levels:
        return levels
    return max(1, min(6, min(w, h).bit_length() - 1))   # floor(log2(min(w, h)))


def sizes(w: int, h: int, k: int) -> list:
    """(width, height) of the levels 0 .. k."""
    out = [(w, h)]
    for _ in range(k):
        w, h = (w + 1) >> 1, (h + 1) >> 1
        out.append((w, h))
    return out


def gain(prm: Params, k: int):
    s, p = 0.0, 1.0
    for _ in range(k):
        s += p
        p *= float(F(prm.spread))
    return F(float(F(prm.strength)) / s)


# ---- float32, the definition ------------------------------------------------------------------------------
def luminance(c: np.ndarray) -> np.ndarray:
    return (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]


def clamped(acc: np.ndarray, samples: float, prm: Params) -> np.ndarray:
    c = np.asarray(acc, np.float32) / F(samples)
    c = np.where(c > F(0), c, F(0)).astype(np.float32)
    return np.where(c < F(prm.clamp), c, F(prm.clamp)).astype(np.float32)


def bright(acc: np.ndarray, samples: float, prm: Params) -> np.ndarray:
    with np.errstate(all="ignore"):
        c = clamped(acc, samples, prm)
        lum = luminance(c)
        t = F(prm.threshold)
        w = np.where(lum > t, (lum - t) / lum, F(0)).astype(np.float32)
        return c * w[..., None]


def _taps_down(n: int):
    x = np.arange((n + 1) >> 1)
    return [np.clip(2 * x - 1 + j, 0, n - 1) for j in range(4)]


def down(a: np.ndarray) -> np.ndarray:
    tx, ty = _taps_down(a.shape[1]), _taps_down(a.shape[0])
    hor = (a[:, tx[0]] + a[:, tx[3]]) + F(3) * (a[:, tx[1]] + a[:, tx[2]])
    ver = (hor[ty[0]] + hor[ty[3]]) + F(3) * (hor[ty[1]] + hor[ty[2]])
    return ver * F(1.0 / 64.0)


def _taps_up(n: int, coarse: int):
    x = np.arange(n)
    near = x >> 1
    far = np.clip(np.where(x & 1, near + 1, near - 1), 0, coarse - 1)
    return near, far


def up(t: np.ndarray, w: int, h: int) -> np.ndarray:
    nx, fx = _taps_up(w, t.shape[1])
    ny, fy = _taps_up(h, t.shape[0])
    hor = (F(3) * t[:, nx] + t[:, fx]) * F(0.25)
    return (F(3) * hor[ny] + hor[fy]) * F(0.25)


def glare(acc: np.ndarray, samples: float, prm: Params) -> np.ndarray:
    """up(U_1) * gain: what the composition multiplies by `samples` and adds."""
    acc = np.asarray(acc, np.float32)
    h, w = acc.shape[:2]
    k = levels_of(w, h, prm.levels)
    b = [bright(acc, samples, prm)]
    for _ in range(k):
        b.append(down(b[-1]))
    u = b[k]
    for j in range(k - 1, 0, -1):
        u = b[j] + F(prm.spread) * up(u, b[j].shape[1], b[j].shape[0])
    g = up(u, w, h) * gain(prm, k)
    assert g.dtype == np.float32
    return g


def apply(acc: np.ndarray, samples: float, prm: Params) -> np.ndarray:
    acc = np.asarray(acc, np.float32)
    with np.errstate(all="ignore"):
        out = acc + glare(acc, samples, prm) * F(samples)
    assert out.dtype == np.float32
    return out


# ---- float64, built differently: the 1-D operators as dense matrices ---------------------------------------
def down_matrix(n: int) -> np.ndarray:
    m = np.zeros(((n + 1) >> 1, n))
    for x in range(m.shape[0]):
        for j, wt in enumerate((1.0, 3.0, 3.0, 1.0)):
            m[x, min(max(2 * x - 1 + j, 0), n - 1)] += wt / 8.0
    return m


def up_matrix(n: int, coarse: int) -> np.ndarray:
    m = np.zeros((n, coarse))
    for x in range(n):
        near = x >> 1
        far = near + 1 if x & 1 else near - 1
        m[x, near] += 0.75
        m[x, min(max(far, 0), coarse - 1)] += 0.25
    return m


def _sep(my: np.ndarray, a: np.ndarray, mx: np.ndarray) -> np.ndarray:
    return np.stack([my @ a[..., c] @ mx.T for c in range(3)], axis=-1)


def apply64(acc: np.ndarray, samples: float, prm: Params) -> np.ndarray:
    """The definition in float64 (the parameters, samples and the gain are the float32 values)."""
    v = np.asarray(acc, np.float32).astype(np.float64)
    h, w = v.shape[:2]
    k = levels_of(w, h, prm.levels)
    n, t, cl, sp = float(F(samples)), float(F(prm.threshold)), float(F(prm.clamp)), float(F(prm.spread))
    c = np.minimum(np.where(v / n > 0, v / n, 0.0), cl)
    lum = float(F(0.2126)) * c[..., 0] + float(F(0.7152)) * c[..., 1] + float(F(0.0722)) * c[..., 2]   # (the float constants)
    with np.errstate(all="ignore"):
        wgt = np.where(lum > t, (lum - t) / np.where(lum > 0, lum, 1.0), 0.0)
    b = [c * wgt[..., None]]
    sz = sizes(w, h, k)
    for j in range(1, k + 1):
        b.append(_sep(down_matrix(sz[j - 1][1]), b[-1], down_matrix(sz[j - 1][0])))
    u = b[k]
    for j in range(k - 1, 0, -1):
        u = b[j] + sp * _sep(up_matrix(sz[j][1], sz[j + 1][1]), u, up_matrix(sz[j][0], sz[j + 1][0]))
    g = _sep(up_matrix(h, sz[1][1]), u, up_matrix(w, sz[1][0])) * float(gain(prm, k))
    return v + g * n
