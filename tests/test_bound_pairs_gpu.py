"""Every lower bound of the bounded closest hit against the exact test, per (ray, geom) pair
(pt_kernels.hip k_selftest_bounds / pt_selftest_bounds).

The bounds pass rests on a hand-made error analysis (pt_bounds.cpp update_bounds): each bound form claims
a lower bound on the exact test's distance, or a miss the exact test confirms.  A wrong claim changes an
image, or PT_AMD_VERIFY_BOUNDS's count, only when the geom it is about is that ray's closest hit; the
device self-check tests the claim itself, for every form the kernels can apply, on every (ray, geom) pair
of 2^16 rays of six classes (include/pt_amd.h), over the scene families of tests/bound_cases.py that sit
on the edges of the analysis: coordinates of 1e-3 to 1e4, needle scales, both sides of the alignment and
the uniformity thresholds, coincident surfaces, rooms.  Each family is also rendered against the CPU
oracle bit for bit, fused and material-sorted, and under PT_AMD_VERIFY_BOUNDS=1.
"""
import numpy as np
import pytest

import bound_cases as BC
from oracle import binding as O

pytestmark = pytest.mark.gpu

N_RAYS = 1 << 16
MIN_PAIRS = 1000
FAMILIES = list(BC.FAMILIES)
SELF_FLAGS = (dict(), dict(DoF=True, aperture=0.5))


def _assert_report(name, rep, kinds, classes=range(6)):
    """No violation of any form, and the run was about what it claims: every listed kind has pairs, every
    class has rays."""
    print(name, "pairs", rep["pairs"], "rays", rep["rays"], "skipped", rep["skipped"],
          "bad_tagged", rep["bad_tagged"], "bad_float", rep["bad_float"])
    bad = sum(rep["bad_tagged"].values()) + sum(rep["bad_float"].values())
    assert bad == 0, f"{name}: {bad} violations (tagged {rep['bad_tagged']}, float {rep['bad_float']}); first {rep['first']}"
    assert rep["first"] is None
    for k in kinds:
        assert rep["pairs"][str(k)] >= MIN_PAIRS, f"{name}: kind {k} has {rep['pairs'][str(k)]} pairs with t > 0"
    for k in {"1", "2", "3", "4", "room"} - {str(k) for k in kinds}:
        assert rep["pairs"][k] == 0, f"{name}: kind {k} is not listed"
    assert all(rep["rays"][c] > 0 for c in classes), rep["rays"]
    assert sum(rep["rays"]) + sum(rep["skipped"]) == N_RAYS
    # Only a departing ray can leave the precondition: where the reference's float sphere test cancels (a
    # needle's object-space origin of 1e5 and more), it reports hits hundreds of units off, and the next
    # origin lies on the ray at that distance, outside R.  Every other class is inside by construction.
    assert [v for c, v in enumerate(rep["skipped"]) if c != 1] == [0] * 5, rep["skipped"]


@pytest.mark.parametrize("name", FAMILIES)
def test_every_pair_bound_holds(name):
    s = BC.make_scene(name)
    for k, fl in enumerate(SELF_FLAGS):
        rep = s.selftest_bounds(BC.gui(**fl), N_RAYS, 2025 + k)
        _assert_report(f"{name} {fl}", rep, BC.FAMILIES[name].kinds)


def _oflags(g):
    return O.flags(g.russianRoulette, g.useBVHtree, g.useBBox, g.sortbyMaterial, g.useThrustPartition, g.SSAA,
                   g.DoF, g.aperture, g.focal_len, g.singleAlbedo, g.rngKeyPixel)


_REF = {}


def _reference(key, oracle_scene, flags, sort):
    """The oracle's image and live counts, computed once per (scene, pipeline) and left unchanged."""
    if (key, sort) not in _REF:
        o = oracle_scene()
        fl = _oflags(BC.gui(sortbyMaterial=sort, **flags))
        img, live = None, [0] * BC.DEPTH
        for k in range(BC.PASSES):
            img, lv = O.render_pass(o, fl, 1 + BC.SPP * k, spp=BC.SPP, image=img)
            live = [a + b for a, b in zip(live, lv)]
        img.setflags(write=False)
        _REF[(key, sort)] = (img, live)
    return _REF[(key, sort)]


def _render(s, flags, sort):
    from cuda_pathtracer_amd import PathTracer
    pt = PathTracer(s, BC.gui(sortbyMaterial=sort, **flags), spp=BC.SPP)
    for k in range(BC.PASSES):
        pt.render_pass(1 + BC.SPP * k)
    img, st = pt.image(), pt.stats()
    pt.free()
    return img, st


def _assert_same(name, img, ref):
    same = (img == ref) | (np.isnan(img) & np.isnan(ref))
    bad = np.argwhere(~same)
    assert bad.size == 0, f"{name}: {len(bad)} mismatching values, first at {bad[:3].tolist()}"


def _assert_renders(name, scene, oracle_scene, flags, sort, monkeypatch):
    ref, live = _reference(name, oracle_scene, flags, sort)
    img, st = _render(scene(), flags, sort)
    _assert_same(name, img, ref)
    assert st["bounce_live"][:BC.DEPTH] == live
    assert live[0] == BC.RES[0] * BC.RES[1] * BC.SPP * BC.PASSES
    # again with the plain loop re-run for every ray: the split pipeline's rays are the fused kernel's
    monkeypatch.setenv("PT_AMD_VERIFY_BOUNDS", "1")
    monkeypatch.setenv("PT_PIPELINE", "split")
    img, st = _render(scene(), flags, sort)
    assert st["bound_mismatch"] == 0
    assert st["segments"] == sum(live)
    _assert_same(name, img, ref)


@pytest.mark.parametrize("sort", [False, True], ids=["fused", "sorted"])
@pytest.mark.parametrize("name", FAMILIES)
def test_family_renders_equal_the_oracle(name, sort, monkeypatch):
    _assert_renders(name, lambda: BC.make_scene(name), lambda: BC.make_oracle(name), BC.FAMILIES[name].flags, sort,
                    monkeypatch)
    assert _reference(name, None, None, sort)[1][1] > 0   # (paths live on into the later bounces)


def test_far_camera(monkeypatch):
    """Cornell's geoms with the eye so far away that the spheres' bound arithmetic would overflow (the
    tagged form would then call a sphere the ray hits a miss).  The host decides: up to r_limit the scene
    is bounded and every pair's bound holds; beyond it every geom is exact-tested for every ray."""
    lim = BC.make_far_camera(None).bound_info(BC.gui())["r_limit"]
    below, above = lim * (1 - 2.0 ** -10), lim * (1 + 2.0 ** -10)
    s = BC.make_far_camera(below)
    assert s.bound_info(BC.gui())["bounded"]
    rep = s.selftest_bounds(BC.gui(), N_RAYS, 2027)
    # (no departing rays: a ray from a uniform point of a box 4e14 long, in a uniform direction, does not
    # meet the ten units of geometry at its end; such a ray counts in class 0)
    _assert_report("far_camera below", rep, {3, 4}, classes=(0, 2, 3, 4, 5))
    for sort in (False, True):
        _assert_renders(("far", "below"), lambda: BC.make_far_camera(below), lambda: BC.make_far_camera(below, oracle=True),
                        {}, sort, monkeypatch)
        monkeypatch.delenv("PT_AMD_VERIFY_BOUNDS")
        monkeypatch.delenv("PT_PIPELINE")
    s = BC.make_far_camera(above)
    assert not s.bound_info(BC.gui())["bounded"]
    with pytest.raises(Exception, match="beyond the bounds' range"):
        s.selftest_bounds(BC.gui(), 256, 1)
    for sort in (False, True):
        _assert_renders(("far", "above"), lambda: BC.make_far_camera(above), lambda: BC.make_far_camera(above, oracle=True),
                        {}, sort, monkeypatch)
        monkeypatch.delenv("PT_AMD_VERIFY_BOUNDS")
        monkeypatch.delenv("PT_PIPELINE")
