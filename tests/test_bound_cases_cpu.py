"""The host's preparation of the bounded closest hit (pt_bounds.cpp update_bounds) over
the scene families of tests/bound_cases.py, without a GPU: Scene.bound_info(gui) reads the prepared geom
table (pt_scene_bound_info).

 - Classification: every family produces exactly the bound kinds it lists, and the geoms that approach
   the alignment and the uniformity thresholds land on the side bound_cases.py derives for them.
 - Containment, in exact rational arithmetic (a float is a rational: no tolerance): a world-box cube's
   widened box [wlo, whi] holds the image of its widened slabs [slo, shi] under the exact inverse of the
   float matrix `inv`, its tight planes hold the image of the unit cube, and R covers those and the camera.
 - The constants: tslack in (0, 1], back and wback finite wherever the linear part is invertible.
 - The range: every family lies within the bounds' range; Cornell's geoms seen from just inside r_limit
   are bounded, from just beyond it they carry the bounds that claim nothing.
"""
import math
from fractions import Fraction as Fr
from itertools import product

import pytest

import bound_cases as BC

FAMILIES = list(BC.FAMILIES)
_INFO = {}


def _info(name):
    """(scene, bound_info, room_info) of a family with its own flags, computed once."""
    if name not in _INFO:
        s = BC.make_scene(name)
        g = BC.gui(**BC.FAMILIES[name].flags)
        _INFO[name] = (s, s.bound_info(g), s.room_info(g))
    return _INFO[name]


@pytest.mark.parametrize("name", FAMILIES)
def test_family_produces_its_bound_kinds(name):
    s, info, room = _info(name)
    fam = BC.FAMILIES[name]
    assert info["bounded"] and len(info["geoms"]) <= 32
    kinds = {g["bkind"] for g in info["geoms"]} | ({"room"} if room["walls"] > 0 else set())
    assert kinds == fam.kinds
    for gi, want in (fam.geom_kinds or {}).items():
        if want is not None:
            assert info["geoms"][gi]["bkind"] == want, f"geom {gi}"
    if fam.geom_kinds is not None:   # the family is about a threshold: both sides are stated and present
        assert len({k for k in fam.geom_kinds.values() if k is not None}) == 2


def _exact_inverse(inv16):
    """The exact rational inverse of the float map q = M p + t (glm column-major 4x4): p = X (q - t)."""
    M = [[Fr(inv16[4 * k + r]) for k in range(3)] for r in range(3)]
    t = [Fr(inv16[12 + r]) for r in range(3)]
    det = (M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0]) +
           M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]))
    if det == 0:
        return None, t
    X = [[(M[(k + 1) % 3][(r + 1) % 3] * M[(k + 2) % 3][(r + 2) % 3] -
           M[(k + 1) % 3][(r + 2) % 3] * M[(k + 2) % 3][(r + 1) % 3]) / det for k in range(3)] for r in range(3)]
    return X, t


def _image(X, t, q):
    return [sum(X[r][k] * (q[k] - t[k]) for k in range(3)) for r in range(3)]


@pytest.mark.parametrize("name", FAMILIES)
def test_world_boxes_contain_the_widened_cubes_exactly(name):
    s, info, _ = _info(name)
    geoms = s.geoms()
    R = Fr(info["R"])
    cam = s.camera()
    assert all(abs(Fr(float(v))) <= R for v in cam.position)
    checked = 0
    for g, b in zip(geoms, info["geoms"]):
        if b["bkind"] != 3:
            continue
        X, t = _exact_inverse(list(g.inverse_transform))
        assert X is not None
        for corner in product((0, 1), repeat=3):
            q = [Fr(b["shi"][k]) if corner[k] else Fr(b["slo"][k]) for k in range(3)]
            p = _image(X, t, q)
            for r in range(3):
                assert Fr(b["wlo"][r]) <= p[r] <= Fr(b["whi"][r])
            u = _image(X, t, [Fr(1, 2) if corner[k] else Fr(-1, 2) for k in range(3)])
            for r in range(3):
                assert Fr(b["tight"][2 * r]) <= u[r] <= Fr(b["tight"][2 * r + 1])
                assert abs(u[r]) <= R
        checked += 1
    assert checked >= 1


@pytest.mark.parametrize("name", FAMILIES)
def test_slack_and_pull_back_constants(name):
    s, info, _ = _info(name)
    assert 0.0 < info["wb_tslack"] <= 1.0 and math.isfinite(info["abs_slack"]) and info["abs_slack"] > 0.0
    assert info["R"] <= info["r_limit"]
    for gi, (g, b) in enumerate(zip(s.geoms(), info["geoms"])):
        assert 0.0 < b["tslack"] <= 1.0, f"geom {gi}: tslack {b['tslack']}"
        X, _ = _exact_inverse(list(g.inverse_transform))
        if X is not None:
            assert math.isfinite(b["back"]) and math.isfinite(b["wback"]), f"geom {gi}"
            assert b["back"] >= 0.0 and b["wback"] >= 0.0


def test_far_camera_range():
    """Cornell's geoms with the eye on the x axis: just inside r_limit the scene is bounded as ever, just
    beyond it every cube and sphere carries the bound that claims nothing and there is no room."""
    near = BC.make_far_camera(None)
    lim = near.bound_info(BC.gui())["r_limit"]
    # Cornell's sphere has scale 3: S = R / 3 + |inv t|, and the departing test's product 2^-15 (S + 2)^3
    # reaches 2^126 first, at S = 2^47: R = 3 * 2^47 = 4.2e14
    assert 4.0e14 < lim < 4.4e14
    below, above = BC.make_far_camera(lim * (1 - 2.0 ** -10)), BC.make_far_camera(lim * (1 + 2.0 ** -10))
    ib, ia = below.bound_info(BC.gui()), above.bound_info(BC.gui())
    assert ib["bounded"] and ib["R"] <= lim and {g["bkind"] for g in ib["geoms"]} == {3, 4}
    assert all(math.isfinite(v) for g in ib["geoms"] for v in g["wlo"] + g["whi"]) and ib["abs_slack"] > 0.0
    assert not ia["bounded"] and ia["R"] > lim
    assert above.room_info(BC.gui())["walls"] == 0
    for g in ia["geoms"]:
        assert g["bkind"] == 3 and g["tslack"] == 1.0 and g["back"] == 0.0 and g["wback"] == 0.0
        assert all(v == -math.inf for v in g["wlo"]) and all(v == math.inf for v in g["whi"])
    assert ia["abs_slack"] == 0.0 and ia["wb_tslack"] == 1.0
