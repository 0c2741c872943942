"""The reference's random numbers in plain Python and numpy (a helper, not collected by pytest).

makeSeededRandomEngine (pathtrace.cu:57-62) seeds thrust::default_random_engine — minstd_rand,
x <- 48271 x mod (2^31 - 1), a zero seed replaced by 1 — with utilhash (intersections.h:13-22) of the
(iteration, depth) word xor utilhash of the index; uniform_real_distribution<float>(0, 1) returns
float(x - 1) * 2^-31.  All of it is integer arithmetic up to the last step, so the floats are exact.
test_oracle_cpu.py checks the scalar form against the C++ standard's check value and the oracle; the
vectorised form (one row per index) feeds tests/path_ref.py.
"""
import numpy as np

M31 = 2147483647


def utilhash(a: int) -> int:
    m = 0xFFFFFFFF
    a = ((a + 0x7ed55d16) + (a << 12)) & m
    a = ((a ^ 0xc761c23c) ^ (a >> 19)) & m
    a = ((a + 0x165667b1) + (a << 5)) & m
    a = ((a + 0xd3a2646c) ^ (a << 9)) & m
    a = ((a + 0xfd7046c5) + (a << 3)) & m
    a = ((a ^ 0xb55a4f09) ^ (a >> 16)) & m
    return a


def py_u01(it: int, index: int, depth: int, count: int) -> np.ndarray:
    h = utilhash((1 << 31) | (depth << 22) | it) ^ utilhash(index)
    x = h % M31 or 1
    out = []
    for _ in range(count):
        x = (48271 * x) % M31
        out.append(np.float32(x - 1) * np.float32(2.0 ** -31))
    return np.array(out, np.float32)


def utilhash_np(a) -> np.ndarray:
    """utilhash over an array of unsigned 32-bit words (uint64 arithmetic, masked after every step)."""
    m = np.uint64(0xFFFFFFFF)
    a = np.asarray(a, np.uint64) & m
    a = ((a + np.uint64(0x7ed55d16)) + (a << np.uint64(12))) & m
    a = ((a ^ np.uint64(0xc761c23c)) ^ (a >> np.uint64(19))) & m
    a = ((a + np.uint64(0x165667b1)) + (a << np.uint64(5))) & m
    a = ((a + np.uint64(0xd3a2646c)) ^ (a << np.uint64(9))) & m
    a = ((a + np.uint64(0xfd7046c5)) + (a << np.uint64(3))) & m
    a = ((a ^ np.uint64(0xb55a4f09)) ^ (a >> np.uint64(16))) & m
    return a


def u01_table(it: int, index, depth: int, count: int) -> np.ndarray:
    """The first `count` uniforms of the engine seeded with (it, index[i], depth): (len(index), count)
    float32."""
    index = np.asarray(index, np.int64)
    h = np.uint64(utilhash((1 << 31) | (depth << 22) | it)) ^ utilhash_np(index & 0xFFFFFFFF)
    x = h % np.uint64(M31)
    x = np.where(x == 0, np.uint64(1), x)
    out = np.empty(index.shape + (count,), np.float32)
    for k in range(count):
        x = (np.uint64(48271) * x) % np.uint64(M31)
        out[..., k] = (x - np.uint64(1)).astype(np.float32) * np.float32(2.0 ** -31)
    return out
