"""The exact test's fast path under one range gate (pt_kernels.hip exact_geom, pt_device.h RangeGate;
DESIGN.md §3).

The bounded closest hit runs the cores of every correctly rounded sqrt, division and normalize of an
exact test unconditionally and tests the range of all their operands once, at the end; a lane whose
gate tripped recomputes the whole test through the literal, per-operation-gated path.  That may not
change a bit.  Each case below puts operands the gate must catch into waves of ordinary rays: 64x64
pixels (whole 64-pixel waves), 2 iterations, depth 4, in the fused and in the material-sorted pipeline,
bit for bit against the CPU oracle — and again under PT_AMD_VERIFY_BOUNDS=1 (split pipeline, whose rays
are the fused kernel's, and the sorted producer), where the device re-runs the plain per-geom loop (the
literal forms only) for every ray and counts differences, and counts the exact tests taken and the gates
tripped (pt_ctx_exact_counts): every case must show both a tripped gate and a fast-path test in the
same run, so it cannot pass without reaching the path it is about.

The device self-test (pt_selftest_exact) compares the two paths over random and edge (ray, geom) pairs.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import binding as O

pytestmark = pytest.mark.gpu

SPP, DEPTH, RES = 2, 4, (64, 64)
EYE, LOOK = (0, 4, 4), (0, 4, 0)   # along -z: the centre column's rays have d.x == +-0 without jitter and lens
PLAIN = dict(SSAA=False, DoF=False)


def _materials(sc):
    return dict(light=sc.add_material(rgb=(1, 1, 1), emittance=5.0),
                white=sc.add_material(rgb=(0.98, 0.98, 0.98)),
                red=sc.add_material(rgb=(0.85, 0.35, 0.35)),
                green=sc.add_material(rgb=(0.35, 0.85, 0.35)),
                mirror=sc.add_material(rgb=(0.98, 0.98, 0.98), specrgb=(0.98, 0.98, 0.98), reflective=1.0),
                glass=sc.add_material(rgb=(0.95, 0.95, 0.95), refractive=1.0, ior=1.5),
                dense=sc.add_material(rgb=(0.9, 0.95, 0.9), specrgb=(0.9, 0.9, 0.9), refractive=1.0, ior=2.4))


def _room(sc, m):
    """Unrotated walls (exact axis normals, exact zeros in their maps) around [-5, 5] x [0, 10] x [-5, 5],
    open towards +z."""
    from cuda_pathtracer_amd import CUBE
    sc.add_geom(CUBE, m["light"], (0, 10, 0), (0, 0, 0), (3, 0.3, 3))
    sc.add_geom(CUBE, m["white"], (0, 0, 0), (0, 0, 0), (10, 0.01, 10))
    sc.add_geom(CUBE, m["white"], (0, 10, 0), (0, 0, 0), (10, 0.01, 10))
    sc.add_geom(CUBE, m["white"], (0, 5, -5), (0, 0, 0), (10, 10, 0.01))
    sc.add_geom(CUBE, m["red"], (-5, 5, 0), (0, 0, 0), (0.01, 10, 10))
    sc.add_geom(CUBE, m["green"], (5, 5, 0), (0, 0, 0), (0.01, 10, 10))


def _axis_parallel(sc):
    """Case 1: the camera's centre ray is exactly axis-parallel and nothing jitters it: an object-space
    direction component of 0 — a division by zero — in waves of ordinary rays."""
    from cuda_pathtracer_amd import CUBE, SPHERE
    m = _materials(sc)
    _room(sc, m)
    sc.add_geom(CUBE, m["white"], (-2, 1.5, -1), (0, 0, 0), (2, 3, 2))
    sc.add_geom(SPHERE, m["mirror"], (2, 4, -1), (0, 0, 0), (3, 3, 3))
    sc.set_camera(RES, 45.0, EYE, LOOK, (0, 1, 0))


def _on_slab_plane(sc):
    """Case 2: the same camera, and a cube of scale 2 centred at x = 1: its map takes the camera's x = 0
    to -0.5 exactly, the x slab's plane, so that slab's numerator is 0 for every camera ray and the
    centre column (d.x == 0) divides 0 by 0."""
    from cuda_pathtracer_amd import CUBE, SPHERE
    m = _materials(sc)
    _room(sc, m)
    sc.add_geom(CUBE, m["white"], (1, 4, -1), (0, 0, 0), (2, 2, 2))
    sc.add_geom(SPHERE, m["mirror"], (-2, 4, -1), (0, 0, 0), (3, 3, 3))
    sc.set_camera(RES, 45.0, EYE, LOOK, (0, 1, 0))


def _out_of_range(sc):
    """Case 3: a cube scaled by 2^41 (around everything: every ray is inside it) and a sphere scaled by
    2^-41 on the centre ray, beside ordinary geoms: squared direction lengths of 2^-82 and 2^82 and
    numerators beyond 2^40."""
    from cuda_pathtracer_amd import CUBE, SPHERE
    m = _materials(sc)
    _room(sc, m)
    big, tiny = float(2.0 ** 41), float(2.0 ** -41)
    sc.add_geom(CUBE, m["white"], (0, 5, 0), (0, 0, 0), (big, big, big))
    sc.add_geom(SPHERE, m["red"], (0, 4, 2), (0, 0, 0), (tiny, tiny, tiny))
    sc.add_geom(SPHERE, m["mirror"], (2, 4, -1), (0, 0, 0), (3, 3, 3))
    sc.add_geom(CUBE, m["green"], (-2, 1.5, -1), (0, 20, 0), (2, 3, 2))
    sc.set_camera(RES, 45.0, EYE, LOOK, (0, 1, 0))


def _glass(sc):
    """Case 4: test_render_gpu.py's rotated glass cubes (total internal reflection: NaN directions) in
    the room.  A NaN direction is "no hit" before any exact test (intersect_bounded's early return),
    so the operands that trip the gate here are the zeros of the jitter-free camera's centre column."""
    from cuda_pathtracer_amd import CUBE, SPHERE
    m = _materials(sc)
    _room(sc, m)
    for k in range(6):
        sc.add_geom(CUBE, m["glass"] if k % 2 else m["dense"], (-4 + 1.6 * k, 1.5 + (k % 3), -1 + 0.4 * k),
                    (10.0 * k, 25 + 7.0 * k, 5.0 * k), (1.4, 1.4, 1.4))
    sc.add_geom(SPHERE, m["glass"], (0, 6, 1), (0, 0, 0), (2.0, 2.0, 2.0))
    sc.set_camera(RES, 45.0, (0, 4, 9), LOOK, (0, 1, 0))


CASES = {"axis_parallel": _axis_parallel, "on_slab_plane": _on_slab_plane, "out_of_range": _out_of_range,
         "glass": _glass}


def _make(name, oracle_only=False):
    o = O.OracleScene()
    CASES[name](o)
    o.depth = DEPTH
    if oracle_only:
        return None, o
    from cuda_pathtracer_amd import Scene
    s = Scene()
    CASES[name](s)
    s.set_render(SPP, DEPTH, name)
    s.finalize()
    return s, o


def _gui(**kw):
    from cuda_pathtracer_amd import GuiDataContainer
    g = GuiDataContainer()
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def _oflags(g):
    return O.flags(g.russianRoulette, g.useBVHtree, g.useBBox, g.sortbyMaterial, g.useThrustPartition, g.SSAA,
                   g.DoF, g.aperture, g.focal_len, g.singleAlbedo, g.rngKeyPixel)


_REF = {}


def _reference(name, sort):
    """The oracle's image and live counts of a case, computed once and left unchanged."""
    key = (name, sort)
    if key not in _REF:
        _, o = _make(name, oracle_only=True)
        img, live = O.render_pass(o, _oflags(_gui(sortbyMaterial=sort, **PLAIN)), 1, spp=SPP)
        img.setflags(write=False)
        _REF[key] = (img, live)
    return _REF[key]


def _render(name, sort):
    from cuda_pathtracer_amd import PathTracer
    s, _ = _make(name)
    pt = PathTracer(s, _gui(sortbyMaterial=sort, **PLAIN), spp=SPP)
    pt.render_pass(1)
    img, st, cnt = pt.image(), pt.stats(), pt.exact_counts()
    pt.free()
    return img, st, cnt


def _assert_same(name, img, ref):
    same = (img == ref) | (np.isnan(img) & np.isnan(ref))
    bad = np.argwhere(~same)
    assert bad.size == 0, f"{name}: {len(bad)} mismatching values, first at {bad[:3].tolist()}"


@pytest.mark.parametrize("sort", [False, True], ids=["fused", "sorted"])
@pytest.mark.parametrize("name", list(CASES))
def test_exact_gate_bitexact(name, sort):
    img, st, cnt = _render(name, sort)
    ref, live = _reference(name, sort)
    _assert_same(name, img, ref)
    assert st["bounce_live"][:DEPTH] == live
    assert live[0] == RES[0] * RES[1] * SPP and live[1] > 0
    assert cnt == {"tests": 0, "tripped": 0}   # the shipped kernels carry no counter


@pytest.mark.parametrize("sort", [False, True], ids=["split", "sorted"])
@pytest.mark.parametrize("name", list(CASES))
def test_exact_gate_verified(name, sort, monkeypatch):
    """Every ray's bounded closest hit (fast path, or the literal path behind a tripped gate) equals the
    plain loop's, which runs the literal forms only; some gate tripped and some test took the fast path."""
    monkeypatch.setenv("PT_AMD_VERIFY_BOUNDS", "1")
    monkeypatch.setenv("PT_PIPELINE", "split")
    img, st, cnt = _render(name, sort)
    ref, live = _reference(name, sort)
    print(name, "sorted" if sort else "split", "exact tests", cnt, "segments", st["segments"])
    assert st["bound_mismatch"] == 0
    assert st["segments"] == sum(live)
    _assert_same(name, img, ref)
    assert cnt["tripped"] >= 1
    assert cnt["tests"] - cnt["tripped"] >= 1


def test_exact_selftest():
    """2^20 random (ray, geom) pairs, the edge operands of pt_selftest_math's generator among them: the
    exact test with its gate == the literal exact test, with gates tripped and fast paths taken."""
    from cuda_pathtracer_amd._native import check_pt, lib
    bad, tripped, fast = C.c_uint64(1), C.c_uint64(0), C.c_uint64(0)
    n = 1 << 20
    check_pt(lib().pt_selftest_exact(n, 2024, C.byref(bad), C.byref(tripped), C.byref(fast)))
    print("pairs", n, "mismatches", bad.value, "tripped", tripped.value, "fast", fast.value)
    assert tripped.value + fast.value == n
    assert bad.value == 0
    assert tripped.value >= 1
    assert fast.value >= n // 4
