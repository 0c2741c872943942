"""The grouped bound of a room's walls in the later bounces' closest hit (pt_kernels.hip
bound_room_tagged, pt_bounds.cpp find_room).

The later bounces take the room's walls from two plane parameters per axis instead of one slab test
per wall: a bound for the wall ahead, a miss or a zero bound for the wall behind, wherever the ray
starts (in the room, in a wall's widened slab, or outside).  That may not change a bit of the image,
so every case renders a few small passes in the fused and in the material-sorted pipeline and compares with
the CPU oracle bit for bit, then repeats under PT_AMD_VERIFY_BOUNDS=1 (split pipeline and sorted
producer), where the device re-runs the plain per-geom loop for every ray and counts differences.
pt_ctx_room_info tells which walls the host grouped, so a case cannot pass on the per-wall loop alone.
"""
import functools

import numpy as np
import pytest

from oracle import binding as O
from room_cases import (CASES, DEPTH, EYE, LOOK, PASSES, SPP, _gui, assert_room, make_scene, scene_path,
                        scene_dir)   # noqa: F401  (scene_dir: a fixture)

pytestmark = pytest.mark.gpu


def _make(name, scene_dir, cornell_path, oracle_only=False):
    """(Scene or None, OracleScene) of a case."""
    path = scene_path(name, scene_dir, cornell_path)
    if path is not None:
        o = O.OracleScene.from_json(path)
        if CASES[name][0] is None:
            o.set_camera((64, 64), 45.0, EYE, LOOK, (0, 1, 0))
    else:
        o = O.OracleScene()
        CASES[name][0](o)
        o.depth = DEPTH
    return (None if oracle_only else make_scene(name, scene_dir, cornell_path)), o


def _oflags(g):
    return O.flags(g.russianRoulette, g.useBVHtree, g.useBBox, g.sortbyMaterial, g.useThrustPartition, g.SSAA,
                   g.DoF, g.aperture, g.focal_len, g.singleAlbedo, g.rngKeyPixel)


_REF = {}


def _reference(name, sort, scene_dir, cornell_path):
    """The oracle's image and live counts of a case, computed once and left unchanged."""
    key = (name, sort)
    if key not in _REF:
        _, o = _make(name, scene_dir, cornell_path, oracle_only=True)
        fl = _oflags(_gui(sortbyMaterial=sort, **CASES[name][1]))
        img, live = None, [0] * DEPTH
        for k in range(PASSES):
            img, lv = O.render_pass(o, fl, 1 + SPP * k, spp=SPP, image=img)
            live = [a + b for a, b in zip(live, lv)]
        img.setflags(write=False)
        _REF[key] = (img, live)
    return _REF[key]


def _bits(info):
    """A room_info() with its floats as bit patterns."""
    return (info["walls"], info["faces"], np.array(info["lo"] + info["hi"], np.float32).view(np.uint32).tolist())


@pytest.mark.parametrize("name", list(CASES))
def test_room_found(name, scene_dir, cornell_path):
    """The host groups the walls each case is about (and the oracle alone says the case has live
    paths at every later bounce, so the grouped bound runs at all of them).  The context reports the
    room the scene's host-only preparation derives for the same flags, bit for bit."""
    from cuda_pathtracer_amd import PathTracer
    s, _ = _make(name, scene_dir, cornell_path)
    gui = _gui(**CASES[name][1])
    pt = PathTracer(s, gui, spp=SPP)
    info = pt.room_info()
    pt.free()
    assert_room(info, CASES[name][2])
    assert _bits(info) == _bits(s.room_info(gui))
    _, live = _reference(name, False, scene_dir, cornell_path)
    assert all(v > 0 for v in live), live


@pytest.mark.parametrize("sort", [False, True], ids=["fused", "sorted"])
@pytest.mark.parametrize("name", list(CASES))
def test_room_bitexact(name, sort, scene_dir, cornell_path):
    from cuda_pathtracer_amd import PathTracer
    s, _ = _make(name, scene_dir, cornell_path)
    pt = PathTracer(s, _gui(sortbyMaterial=sort, **CASES[name][1]), spp=SPP)
    for k in range(PASSES):
        pt.render_pass(1 + SPP * k)
    img, st = pt.image(), pt.stats()
    pt.free()
    ref, live = _reference(name, sort, scene_dir, cornell_path)
    same = (img == ref) | (np.isnan(img) & np.isnan(ref))
    bad = np.argwhere(~same)
    assert bad.size == 0, f"{name}: {len(bad)} mismatching values, first at {bad[:3].tolist()}"
    assert st["bounce_live"][:DEPTH] == live
    assert ref.sum() > 0


@pytest.mark.parametrize("sort", [False, True], ids=["split", "sorted"])
@pytest.mark.parametrize("name", list(CASES))
def test_room_bounds_verified(name, sort, scene_dir, cornell_path, monkeypatch):
    """Every ray's bounded closest hit equals the plain loop's, in the split pipeline (the fused
    kernel's rays) and in the sorted producer."""
    from cuda_pathtracer_amd import PathTracer
    monkeypatch.setenv("PT_AMD_VERIFY_BOUNDS", "1")
    monkeypatch.setenv("PT_PIPELINE", "split")
    s, _ = _make(name, scene_dir, cornell_path)
    pt = PathTracer(s, _gui(sortbyMaterial=sort, **CASES[name][1]), spp=SPP)
    for k in range(PASSES):
        pt.render_pass(1 + SPP * k)
    st = pt.stats()
    pt.free()
    _, live = _reference(name, sort, scene_dir, cornell_path)
    assert st["bound_mismatch"] == 0
    assert st["segments"] == sum(live)


def test_room_off_knob(scene_dir, cornell_path, monkeypatch):
    """PT_AMD_ROOM=0 leaves the walls in the per-cube loop: no room reported, the same image."""
    from cuda_pathtracer_amd import PathTracer
    monkeypatch.setenv("PT_AMD_ROOM", "0")
    s, _ = _make("cornell", scene_dir, cornell_path)
    pt = PathTracer(s, _gui(), spp=SPP)
    assert pt.room_info()["walls"] == 0
    for k in range(PASSES):
        pt.render_pass(1 + SPP * k)
    img = pt.image()
    pt.free()
    ref, _ = _reference("cornell", False, scene_dir, cornell_path)
    assert np.array_equal(img, ref)
