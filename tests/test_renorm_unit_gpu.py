"""renorm_unit_core (pt_device.h) against norm_core on the device, bit for bit, in one launch
(pt_selftest_renorm): every one of the 6,145 floats of [1 - 2^-12, 1 + 2^-12] as x, the first float
outside on each side and zero, denormal, huge, infinite, negative and NaN x (the general path), and 4,096
vectors with x = dot(v, v), three of four normalized, for which point_on_ray_unit is compared with
point_on_ray as well.  tests/test_renorm_unit_cpu.py checks the same closed form on the host against a
correctly rounded 1 / sqrt."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

NVEC, IN_RANGE, EDGES = 4096, 6145, 16


def test_renorm_unit_equals_norm_core():
    from cuda_pathtracer_amd._native import check_pt, lib
    bad, inr, mis = C.c_uint64(1), C.c_uint64(0), C.c_uint64(1)
    check_pt(lib().pt_selftest_renorm(NVEC, 2025, C.byref(bad), C.byref(inr), C.byref(mis)))
    print("items", IN_RANGE + EDGES + NVEC, "mismatches", bad.value, "closed form", inr.value, "misranged", mis.value)
    assert bad.value == 0
    assert mis.value == 0
    # the whole range took the closed form, no edge value did, the normalized vectors (3 of 4) did, and
    # some of the others did not
    assert IN_RANGE + 3 * NVEC // 4 <= inr.value < IN_RANGE + NVEC
