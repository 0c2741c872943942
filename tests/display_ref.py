"""The display transform restated in numpy: the yardstick of test_display_cpu.py and
test_display_gpu.py.  The curves and conversions are float32 operations, one per written operation; the meter's
resolve is Python integers; the tables are built in double as the definition says.  Imports nothing from the
package."""
from __future__ import annotations

import math
from dataclasses import dataclass, replace  # noqa: F401

import numpy as np

F = np.float32
MANUAL, AUTO = 0, 1
NONE, REINHARD, ACES, HABLE = 0, 1, 2, 3
LINEAR, SRGB = 0, 1
LUM_MIN, INF_BITS = 0x37800000, 0x7F800000


@dataclass
class Params:
    exposure_mode: int = MANUAL
    exposure: float = 1.0
    key_value: float = 0.18
    compensation_ev: float = 0.0
    min_ev: float = -8.0
    max_ev: float = 8.0
    pct_lo: int = 102
    pct_hi: int = 922
    rate: int = 256
    curve: int = NONE
    white: float = 4.0
    transfer: int = LINEAR
    mirror_x: int = 0


# ---- tables ------------------------------------------------------------------------------------
def srgb_eotf(x: float) -> float:
    return x / 12.92 if x <= 0.04045 else math.pow((x + 0.055) / 1.055, 2.4)


def srgb_oetf(x: np.ndarray) -> np.ndarray:
    x = np.asarray(x, np.float64)
    return np.where(x <= 0.0031308, 12.92 * x, 1.055 * np.power(x, 1.0 / 2.4) - 0.055)


def hable_f(x):
    a, b, c, d, e, f = F(0.15), F(0.50), F(0.10), F(0.20), F(0.02), F(0.30)
    return (x * (a * x + c * b) + d * e) / (x * (a * x + b) + d * f) - e / f


def tables() -> dict:
    srgb = np.zeros(256, np.float32)
    for b in range(1, 256):
        t = srgb_eotf((b - 0.5) / 255.0)
        f = F(t)
        if float(f) < t:   # rounded up
            f = np.nextafter(f, F(np.inf))
        srgb[b] = f
    pow2 = np.array([F(math.pow(2.0, k / 256.0)) for k in range(256)], np.float32)
    return {"srgb": srgb, "pow2": pow2, "hable_white": F(hable_f(F(11.2)))}


# ---- applying ----------------------------------------------------------------------------------
def curve_values(acc: np.ndarray, samples: float, mult, prm: Params, hable_white) -> np.ndarray:
    """Steps 1 to 5: float32 values in [0, 1], the accumulator's shape."""
    with np.errstate(all="ignore"):
        c = (np.asarray(acc, np.float32) / F(samples)) * F(mult)
        c = np.where(c > F(0), c, F(0)).astype(np.float32)
        c = np.where(c < F(65504), c, F(65504)).astype(np.float32)
        if prm.curve == REINHARD:
            ww = F(prm.white) * F(prm.white)
            c = (c * (F(1) + c / ww)) / (F(1) + c)
        elif prm.curve == ACES:
            c = (c * (F(2.51) * c + F(0.03))) / (c * (F(2.43) * c + F(0.59)) + F(0.14))
        elif prm.curve == HABLE:
            c = hable_f(F(2) * c) / F(hable_white)
        assert c.dtype == np.float32
        c = np.where(c > F(0), c, F(0)).astype(np.float32)
        return np.where(c < F(1), c, F(1)).astype(np.float32)


def to_bytes(c: np.ndarray, transfer: int, srgb: np.ndarray) -> np.ndarray:
    if transfer == LINEAR:
        return (c * F(255)).astype(np.uint8)
    return np.searchsorted(srgb[1:], c, side="right").astype(np.uint8)   # #{b in 1..255 : T[b] <= c}


def layout(b: np.ndarray, mirror_x: int, stride: int) -> np.ndarray:
    if mirror_x:
        b = b[:, ::-1]
    if stride == 4:
        b = np.concatenate([b, np.zeros(b.shape[:2] + (1,), np.uint8)], axis=2)
    return np.ascontiguousarray(b)


def apply(acc: np.ndarray, samples: float, prm: Params, tab: dict, mult=None, stride: int = 3) -> np.ndarray:
    """(H, W, stride) uint8.  mult: the multiplier of auto mode (manual: prm.exposure)."""
    m = F(prm.exposure) if prm.exposure_mode == MANUAL else F(1 if mult is None else mult)
    c = curve_values(acc, samples, m, prm, tab["hable_white"])
    return layout(to_bytes(c, prm.transfer, tab["srgb"]), prm.mirror_x, stride)


# ---- metering ----------------------------------------------------------------------------------
def histogram(acc: np.ndarray, samples: float) -> np.ndarray:
    """257 counts: 256 bins of 1/8 octave from 2^-16 and the uncounted bin."""
    with np.errstate(all="ignore"):
        v = np.asarray(acc, np.float32).reshape(-1, 3) / F(samples)
        lum = (F(0.2126) * v[:, 0] + F(0.7152) * v[:, 1]) + F(0.0722) * v[:, 2]
    bits = np.ascontiguousarray(lum, np.float32).view(np.uint32).astype(np.int64)
    counted = (bits >= LUM_MIN) & (bits < INF_BITS)
    bins = np.where(counted, np.minimum(255, (bits - LUM_MIN) >> 20), 256)
    return np.bincount(bins, minlength=257).astype(np.int64)


def host_constants(prm: Params):
    """G + C, Emin, Emax: in double, from the float32 parameters."""
    r = lambda v: int(math.floor(v + 0.5))   # noqa: E731
    g = r(256.0 * math.log2(float(F(prm.key_value))))
    c = r(256.0 * float(F(prm.compensation_ev)))
    return g + c, r(256.0 * float(F(prm.min_ev))), r(256.0 * float(F(prm.max_ev)))


def window(n: int, lo: int, hi: int):
    a, b = (n * lo) >> 10, (n * hi + 1023) >> 10
    return a, b, b - a


def level(hist, lo: int, hi: int) -> "int | None":
    """K: the mean level of the ranks [a, b) in 1/256 octave relative to luminance 1; None when nothing counted."""
    h = [int(x) for x in hist[:256]]
    n = sum(h)
    if n == 0:
        return None
    a, b, m_ = window(n, lo, hi)
    s, c = 0, 0
    for k, hk in enumerate(h):
        s += k * max(0, min(b, c + hk) - max(a, c))
        c += hk
    return (32 * s + m_ // 2) // m_ + 16 - 4096


def target(hist, prm: Params) -> "int | None":
    big_k = level(hist, prm.pct_lo, prm.pct_hi)
    if big_k is None:
        return None
    gc, emin, emax = host_constants(prm)
    return max(emin, min(emax, gc - big_k))


def step(state, t: "int | None", rate: int):
    """state: (e, metered).  One metering towards the target t."""
    e, has = state
    if t is None:
        return e, has
    if not has:
        return t, 1
    d = t - e
    if d:
        e += (1 if d > 0 else -1) * max(1, (abs(d) * rate) >> 8)
    return e, 1


def multiplier(e: int, pow2: np.ndarray):
    return F(np.ldexp(F(pow2[e & 255]), e >> 8))


def meter(acc: np.ndarray, samples: float, prm: Params, state=(0, 0)):
    """One pt_display_meter: (histogram, new state)."""
    h = histogram(acc, samples)
    return h, step(state, target(h, prm), prm.rate)
