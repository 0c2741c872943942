"""TEST INFRASTRUCTURE ONLY: the inputs shared by tests/test_hdr_enc_cpu.py and tests/test_hdr_enc_gpu.py: crafted
plane rows with the tokens each must produce, accumulators whose R plane is a given row, and the crafted
accumulator."""
from __future__ import annotations

import functools

import numpy as np

RUN_VALUE = 255           # the byte of a crafted run: the literal fillers below stay under 251
STEP_STARTS = (62, 63, 64, 65, 254, 255, 256, 257)   # around the step boundaries of both step widths (64 and 256 bytes)
STEP_LENGTHS = (2, 3, 130)


def filler(n: int, phase: int = 0) -> np.ndarray:
    """n bytes below 251 of which no two neighbours are equal."""
    return ((np.arange(n) + phase) * 7 + 3) % 251


def _chunks(n: int, size: int) -> list:
    return [size] * (n // size) + ([n % size] if n % size else [])


def lits(n: int) -> list:
    return [("lit", k) for k in _chunks(n, 128)]


def runs(n: int, v: int) -> list:
    return [("run", k, v) for k in _chunks(n, 127)]


@functools.lru_cache(maxsize=None)
def rows() -> dict:
    """name -> (the row, the tokens it must be coded as)."""
    out = {}
    for w in (8, 126, 127, 128, 254, 255, 381):   # run pieces of exactly 127 and a remainder of 0 or 1
        out[f"constant_{w}"] = (np.full(w, 9), runs(w, 9))
    for w in (128, 129, 256, 257):                # dumps of exactly 128 and a remainder of 1
        out[f"no_run_{w}"] = (filler(w), lits(w))
    out["pairs"] = (np.repeat(filler(8), 2), lits(16))
    out["run_of_3"] = (np.array([1, 2, 3, 3, 3, 4, 5, 6, 7, 8]), lits(2) + runs(3, 3) + lits(5))
    out["literal_between_runs"] = (np.array([5] * 4 + [9] + [7] * 4), runs(4, 5) + lits(1) + runs(4, 7))
    out["run_to_the_end"] = (np.array([1, 2, 3, 4, 5, 6, 6, 6, 6]), lits(5) + runs(4, 6))
    out["pair_at_the_end"] = (np.array([1, 2, 3, 4, 5, 6, 7, 8, 8]), lits(9))
    out["stretch_128_then_run"] = (np.concatenate([filler(128), [RUN_VALUE] * 5]), lits(128) + runs(5, RUN_VALUE))
    for s in STEP_STARTS:
        for n in STEP_LENGTHS:
            row = np.concatenate([filler(s), [RUN_VALUE] * n, filler(5, 1)])
            out[f"run_at_{s}_len_{n}"] = (row, lits(s + n + 5) if n < 3 else lits(s) + runs(n, RUN_VALUE) + lits(5))
    return {k: (np.asarray(r, np.uint8), t) for k, (r, t) in out.items()}


def by_width() -> dict:
    """width -> (names, the rows of that width stacked (N, W))."""
    groups: dict = {}
    for name, (row, _) in rows().items():
        groups.setdefault(len(row), []).append(name)
    return {w: (names, np.stack([rows()[n][0] for n in names])) for w, names in sorted(groups.items())}


def accumulator_of_rows(r_plane: np.ndarray, others: str, seed: int = 0) -> np.ndarray:
    """A float accumulator (samples = 1) whose R plane codes to r_plane's bytes: every component lies in [0, 2) and
    B is at least 1, so every pixel's exponent is 1, the scale 128 and a component's byte is 128 times its value.
    others: "random" (G and B random bytes' worth) or "constant"."""
    h, w = r_plane.shape
    acc = np.empty((h, w, 3), np.float32)
    acc[..., 0] = r_plane.astype(np.float32) / np.float32(128.0)
    if others == "random":
        rng = np.random.default_rng(seed)
        acc[..., 1] = rng.integers(0, 256, (h, w)).astype(np.float32) / np.float32(128.0)
        acc[..., 2] = rng.integers(128, 256, (h, w)).astype(np.float32) / np.float32(128.0)
    else:
        acc[..., 1] = np.float32(0.25)
        acc[..., 2] = np.float32(1.0)
    return acc


ACC_SAMPLES = (1.0, 3.0, 7.0)


@functools.lru_cache(maxsize=None)
def accumulator() -> np.ndarray:
    """The crafted accumulator, (12, 64, 3): zeros; both float neighbours of 1e-32 in each channel; every power of
    two 2^-100 .. 2^127 and both neighbours as a pixel's maximum (the frexp boundaries), the maximum moving through
    the channels; ties between channels; a negative component beside a positive maximum in each channel (its scaled
    value above -2^31; the host library narrows R and G with saturation and keeps B's low byte); all-negative
    pixels.  Encoded with ACC_SAMPLES, so that the division rounds."""
    f = np.float32
    px = [(0.0, 0.0, 0.0)]
    t = f(1e-32)
    for v in (np.nextafter(t, f(0)), t, np.nextafter(t, f(1))):
        px += [(v, 0.0, 0.0), (0.0, v, 0.0), (0.0, 0.0, v), (v, v, v)]
    for k, e in enumerate(range(-100, 128)):
        p = np.ldexp(f(1), e)
        for v in (np.nextafter(p, f(0)), p, np.nextafter(p, f(np.inf)) if e < 127 else p):
            lo, mid = f(v * f(0.37)), f(v * f(0.81))
            px.append([(v, mid, lo), (lo, v, mid), (mid, lo, v)][k % 3])
    px += [(1.0, 1.0, 0.5), (0.5, 1.0, 1.0), (1.0, 0.5, 1.0), (1.0, 1.0, 1.0), (3.0, 3.0, 3.0)]
    px += [(1.0, -3.7 / 128, 0.25), (-3.7 / 128, 1.0, -0.5 / 128), (0.5, -1.0e6, -255.9 / 256), (2.5e-20, -1.0e-12, 0.0),
           (-300.5 / 128, -32768.0 / 128, 1.0), (1.0, -64536.5 / 128, -32769.0 / 128), (1.0, 0.25, -3.7 / 128)]
    px += [(-1.0, -2.0, -3.0), (-1e-30, -0.0, -5.0)]
    out = np.zeros((12 * 64, 3), np.float32)
    assert len(px) <= len(out)
    out[:len(px)] = np.array(px, np.float32)
    return out.reshape(12, 64, 3)


def noisy(w: int, h: int, seed: int = 1) -> np.ndarray:
    """A non-negative accumulator with flat areas (runs), gradients and noise, and a black band."""
    rng = np.random.default_rng(seed + 1000 * w + h)
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    base = np.stack([np.floor(x / 5.0) * 0.125, np.floor((x + y) / 9.0) * 0.03125 + 0.5, np.full((h, w), 0.75)], -1)
    noise = rng.random((h, w, 3)) * (rng.random((h, w, 1)) < 0.3)
    acc = (base + noise).astype(np.float32) * np.float32(4.0)
    acc[:, w // 3:w // 3 + max(1, w // 7)] = 0.0
    return acc
