"""The closed form behind renorm_unit_core (pt_layout.h unit_rnorm_bits; pt_device.h), without a GPU.

The kernels renormalise directions that are already of unit length (getPointOnRay): for
x = dot(d, d) in [1 - 2^-12, 1 + 2^-12] the factor 1 / sqrt(x) that glm's normalize computes — a
correctly rounded float square root, then a correctly rounded float division of 1 by it — is read off x's
bit pattern instead.  pt_unit_rnorm_host (pt_renorm.cpp) compiles the same constexpr lines for the host.

The check is exhaustive, not an argument: every one of the 6,145 floats of the range, against the two
roundings computed twice (numpy's float32 sqrt and divide, and float64 operations rounded to float32,
which round correctly because 53 >= 2 * 24 + 2); and the first float outside on each side, with other
values further out, must be declared out of range, where the kernels keep the general code.
"""
import ctypes as C

import numpy as np

ONE = 0x3F800000
LO, HI = ONE - 4096, ONE + 2048   # bits of 1 - 2^-12 (ulp 2^-24 below 1) and of 1 + 2^-12 (ulp 2^-23)


def _host(bits):
    from cuda_pathtracer_amd._native import check_pt, lib
    bits = np.ascontiguousarray(bits, dtype=np.uint32)
    out = np.empty(bits.size, np.uint32)
    ok = np.empty(bits.size, np.uint8)
    check_pt(lib().pt_unit_rnorm_host(bits.ctypes.data_as(C.c_void_p), bits.size, out.ctypes.data_as(C.c_void_p),
                                      ok.ctypes.data_as(C.c_void_p)))
    return out, ok


def _two_roundings(x):
    """1.0f / sqrtf(x): each operation correctly rounded to float32."""
    with np.errstate(all="ignore"):
        a = np.float32(1.0) / np.sqrt(x.astype(np.float32))
        s = np.sqrt(x.astype(np.float64)).astype(np.float32)
        b = (1.0 / s.astype(np.float64)).astype(np.float32)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    return a


def test_range_is_the_stated_one():
    assert np.array([LO, HI], np.uint32).view(np.float32).tolist() == [1.0 - 2.0 ** -12, 1.0 + 2.0 ** -12]
    assert HI - LO + 1 == 6145


def test_every_float_in_range():
    bits = np.arange(LO, HI + 1, dtype=np.uint32)
    out, ok = _host(bits)
    assert ok.all()
    want = _two_roundings(bits.view(np.float32)).view(np.uint32)
    bad = np.flatnonzero(out != want)
    assert bad.size == 0, f"{bad.size} of {bits.size} differ, first at bits {hex(int(bits[bad[0]]))}"
    # (the form really varies over the range: it is not a constant that happens to fit)
    assert np.unique(out).size == 1024 + 1 + 1024


def test_outside_takes_the_general_path():
    edge = [LO - 1, HI + 1, LO - 2, HI + 2, 0, 0x80000000, 1, 0x00800000, 0x3F000000, 0x40000000, 0x7F7FFFFF,
            0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0xBF800000, ONE - 2 ** 23, ONE + 2 ** 23, 0xFFFFFFFF]
    rnd = np.random.default_rng(11).integers(0, 2 ** 32, 4096, dtype=np.uint64).astype(np.uint32)
    bits = np.concatenate([np.array(edge, np.uint32), rnd])
    out, ok = _host(bits)
    inside = (bits >= LO) & (bits <= HI)
    assert np.array_equal(ok.astype(bool), inside)
    assert not ok[:len(edge)].any()
    assert (out[~inside] == 0).all()
