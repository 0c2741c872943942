"""Render parity for the bounce kernels' cheaper renormalisation of unit vectors (pt_device.h
renorm_unit_core; exact_geom's epilogue and shade's getPointOnRay), bit for bit against the CPU oracle.

32 x 32 pixels, 3 iterations per pass, two passes, depth 8: the Cornell box (every direction a unit
vector: the closed form throughout) and scenes.random_primitives (glass: refracted directions, which are
not renormalised, and the NaN directions of total internal reflection take the general code behind the
branch), in every pipeline that runs the changed code: the fused kernels on one lane and on two, the
material-sorted pipeline (k_sort_produce) and the split pipeline (k_trace).  `bounce_live` must equal the
oracle's counts.  (The 32-bit offsets into the path planes that were measured with this change were not
shipped, profiles/r11_valu_overhead_ab.txt, so there is one addressing path and no switch to force.)

The exact test itself: pt_selftest_exact (exact_geom, whose gate now also carries the unit range, against
exact_geom_literal) over random and edge pairs, and the scene families of tests/bound_cases.py rendered
under PT_AMD_VERIFY_BOUNDS=1, where the device compares every ray's bounded closest hit (exact_geom) with
the plain loop's (the literal forms only) and counts the exact tests and the tripped gates.
"""
import ctypes as C

import numpy as np
import pytest

import bound_cases as BC
from oracle import binding as O

pytestmark = pytest.mark.gpu

RES, SPP, PASSES = (32, 32), 3, (1, 4)
MODES = {
    "fused_1_lane": dict(env={"PT_AMD_LANES": "1"}, sort=False),
    "fused_2_lanes": dict(env={"PT_AMD_LANES": "2"}, sort=False),
    "sorted": dict(env={}, sort=True),
    "split": dict(env={"PT_PIPELINE": "split"}, sort=False),
}


def _gui(**kw):
    from cuda_pathtracer_amd import GuiDataContainer
    g = GuiDataContainer()
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def _oflags(g):
    return O.flags(g.russianRoulette, g.useBVHtree, g.useBBox, g.sortbyMaterial, g.useThrustPartition, g.SSAA,
                   g.DoF, g.aperture, g.focal_len, g.singleAlbedo, g.rngKeyPixel)


@pytest.fixture(scope="module")
def scene_paths(cornell_path, tmp_path_factory):
    from cuda_pathtracer_amd import scenes
    d = tmp_path_factory.mktemp("valu_overhead")
    return {"cornell": cornell_path, "random_primitives": scenes.random_primitives(str(d), n=24, res=RES, seed=7)}


def _scenes(path):
    from cuda_pathtracer_amd import Scene
    s = Scene(path)
    o = O.OracleScene.from_json(path)
    if path.endswith("cornell.json"):
        s.set_camera(RES, 45.0, (0, 5, 10.5), (0, 5, 0), (0, 1, 0))
        o.set_camera(RES, 45.0, (0, 5, 10.5), (0, 5, 0), (0, 1, 0))
    s.finalize()
    return s, o


_REF = {}


def _reference(name, path, sort):
    """The oracle's image and live counts, computed once per (scene, sorted) and left unchanged."""
    key = (name, sort)
    if key not in _REF:
        _, o = _scenes(path)
        img, total = None, [0] * o.depth
        for it in PASSES:
            img, live = O.render_pass(o, _oflags(_gui(sortbyMaterial=sort)), it, spp=SPP, image=img)
            total = [a + b for a, b in zip(total, live)]
        img.setflags(write=False)
        _REF[key] = (img, total)
    return _REF[key]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", ["cornell", "random_primitives"])
def test_render_parity(name, mode, scene_paths, monkeypatch):
    from cuda_pathtracer_amd import PathTracer
    for k in ("PT_AMD_LANES", "PT_PIPELINE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in MODES[mode]["env"].items():
        monkeypatch.setenv(k, v)
    sort = MODES[mode]["sort"]
    s, _ = _scenes(scene_paths[name])
    pt = PathTracer(s, _gui(sortbyMaterial=sort), spp=SPP)
    for it in PASSES:
        pt.render_pass(it)
    img, live = np.asarray(pt.image(), np.float32), pt.stats()["bounce_live"]
    pt.free()
    ref, rlive = _reference(name, scene_paths[name], sort)
    bad = np.argwhere(~((img == ref) | (np.isnan(img) & np.isnan(ref))))
    assert bad.size == 0, f"{name} {mode}: {len(bad)} mismatching values, first at {bad[:3].tolist()}"
    assert live[:len(rlive)] == rlive and rlive[0] == RES[0] * RES[1] * SPP * len(PASSES) and rlive[1] > 0


def test_exact_selftest_with_unit_range():
    """2^20 random and edge (ray, geom) pairs (another seed than tests/test_exact_gate_gpu.py's): 0
    differences from exact_geom_literal; the tripped share is printed."""
    from cuda_pathtracer_amd._native import check_pt, lib
    bad, tripped, fast = C.c_uint64(1), C.c_uint64(0), C.c_uint64(0)
    n = 1 << 20
    check_pt(lib().pt_selftest_exact(n, 11, C.byref(bad), C.byref(tripped), C.byref(fast)))
    print("pairs", n, "mismatches", bad.value, "tripped", tripped.value, "share", tripped.value / n)
    assert tripped.value + fast.value == n
    assert bad.value == 0
    assert tripped.value >= 1 and fast.value >= n // 4


@pytest.mark.parametrize("name", list(BC.FAMILIES))
def test_exact_over_bound_case_families(name, monkeypatch):
    """A family's rays through exact_geom and through the literal loop: no difference, and the tripped
    share of its exact tests (printed)."""
    from cuda_pathtracer_amd import PathTracer
    monkeypatch.setenv("PT_AMD_VERIFY_BOUNDS", "1")
    monkeypatch.setenv("PT_PIPELINE", "split")
    pt = PathTracer(BC.make_scene(name), BC.gui(**BC.FAMILIES[name].flags), spp=BC.SPP)
    pt.render_pass(1)
    st, cnt = pt.stats(), pt.exact_counts()
    pt.free()
    share = cnt["tripped"] / max(cnt["tests"], 1)
    print(name, "exact tests", cnt["tests"], "tripped", cnt["tripped"], "share", share, "segments", st["segments"])
    assert st["bound_mismatch"] == 0
    assert cnt["tests"] > 0 and cnt["tests"] - cnt["tripped"] >= 1
