"""The departure claim of the room's grouped bound (pt_kernels.hip bound_room_tagged, pt_bounds.cpp
find_room's room.in).

A ray that has just left a wall starts inside that wall's padded world slab, so the grouped bound
used to keep the wall as a candidate with bound 0 and the whole wave ran an exact test that always
misses.  The wall behind is now also a miss when the origin coordinate lies strictly beyond the
wall's tight plane (the hull of its widened cube without the pad).  That may not change a bit, so
every case renders a few small passes in the fused and in the material-sorted pipeline and compares
with the CPU oracle bit for bit, then repeats under PT_AMD_VERIFY_BOUNDS=1 (split pipeline and sorted
producer), where the device re-runs the plain per-geom loop for every ray and counts differences —
and counts the rays the tight plane alone removed (pt_ctx_depart_counts), so the cases built for the
claim cannot pass with it idle.
"""
import numpy as np
import pytest

from oracle import binding as O

pytestmark = pytest.mark.gpu

SPP, PASSES, DEPTH = 4, 2, 8
EYE, LOOK = (0, 5, 10.5), (0, 5, 0)


def _materials(sc):
    return dict(light=sc.add_material(rgb=(1, 1, 1), emittance=5.0),
                white=sc.add_material(rgb=(0.98, 0.98, 0.98)),
                red=sc.add_material(rgb=(0.85, 0.35, 0.35)),
                green=sc.add_material(rgb=(0.35, 0.85, 0.35)),
                mirror=sc.add_material(rgb=(0.98, 0.98, 0.98), specrgb=(0.98, 0.98, 0.98), reflective=1.0),
                glass=sc.add_material(rgb=(0.98, 0.98, 0.98), specrgb=(0.98, 0.98, 0.98), refractive=1.0, ior=1.5))


def _add(sc, a, b):
    return tuple(x + y for x, y in zip(a, b))


def _shell(sc, m, off=(0, 0, 0)):
    """cornell.json's shell: light, floor, ceiling (rotated 90 degrees), back (rotated), right, left."""
    from cuda_pathtracer_amd import CUBE
    sc.add_geom(CUBE, m["light"], _add(sc, (0, 10, 0), off), (0, 0, 0), (3, 0.3, 3))
    sc.add_geom(CUBE, m["white"], _add(sc, (0, 0, 0), off), (0, 0, 0), (10, 0.01, 10))
    sc.add_geom(CUBE, m["white"], _add(sc, (0, 10, 0), off), (0, 0, 90), (0.01, 10, 10))
    sc.add_geom(CUBE, m["white"], _add(sc, (0, 5, -5), off), (0, 90, 0), (0.01, 10, 10))
    sc.add_geom(CUBE, m["green"], _add(sc, (5, 5, 0), off), (0, 0, 0), (0.01, 10, 10))
    sc.add_geom(CUBE, m["red"], _add(sc, (-5, 5, 0), off), (0, 0, 0), (0.01, 10, 10))


def _plain_room(sc, m, t, front=False, wall="white", half=5.0, light_y=10.0):
    """A room of unrotated walls of thickness t around [-5, 5] x [0, 10] x [-5, 5] (their inner faces t / 2
    inside it, as in cornell.json)."""
    from cuda_pathtracer_amd import CUBE
    sc.add_geom(CUBE, m["light"], (0, light_y, 0), (0, 0, 0), (3, 0.3, 3))
    sc.add_geom(CUBE, m[wall], (0, 0, 0), (0, 0, 0), (10, t, 10))
    sc.add_geom(CUBE, m["white"], (0, 10, 0), (0, 0, 0), (10, t, 10))
    sc.add_geom(CUBE, m[wall], (0, 5, -half), (0, 0, 0), (10, 10, t))
    sc.add_geom(CUBE, m["red"], (-half, 5, 0), (0, 0, 0), (t, 10, 10))
    sc.add_geom(CUBE, m["green"], (half, 5, 0), (0, 0, 0), (t, 10, 10))
    if front:
        sc.add_geom(CUBE, m[wall], (0, 5, half), (0, 0, 0), (10, 10, t))


def _cornell(sc):
    m = _materials(sc)
    _shell(sc, m)
    from cuda_pathtracer_amd import SPHERE
    sc.add_geom(SPHERE, m["mirror"], (-1, 4, -1), (0, 0, 0), (3, 3, 3))
    sc.set_camera((64, 64), 45.0, EYE, LOOK, (0, 1, 0))


def _grazing(sc):
    """Camera inside the room a hand's breadth from the right wall, looking along it, wide lens: first
    hits at grazing incidence, whose next origins lie between the wall's tight and padded planes."""
    m = _materials(sc)
    _shell(sc, m)
    sc.set_camera((56, 48), 60.0, (4.8, 5.0, 4.5), (4.95, 5.0, -5.0), (0, 1, 0))


def _axis_parallel(sc):
    """A closed room of unrotated walls (exact axis normals) seen along -z from inside, no jitter and
    no lens: the centre column has d_x == +-0 exactly and the mirrors keep it through the bounces."""
    m = _materials(sc)
    _plain_room(sc, m, 0.01, front=True, wall="mirror")
    sc.set_camera((48, 48), 40.0, (0, 4, 4), (0, 4, 0), (0, 1, 0))


def _outside(sc):
    """A camera beside the room that sees the walls' front edge faces and the right wall's outer side,
    and cubes that straddle that wall: origins outside the room's box."""
    from cuda_pathtracer_amd import CUBE, SPHERE
    m = _materials(sc)
    _shell(sc, m)
    sc.add_geom(SPHERE, m["mirror"], (2, 3, 7.5), (0, 0, 0), (3, 3, 3))
    sc.add_geom(CUBE, m["white"], (5, 3, 3), (0, 30, 0), (2.5, 2.5, 2.5))
    sc.add_geom(CUBE, m["red"], (5, 7, 4), (0, 0, 0), (2, 2, 2))
    sc.set_camera((64, 48), 35.0, (11, 6, 13), (5, 4, 2), (0, 1, 0))


def _glass(sc):
    """Glass cubes inside the room, one axis-aligned on the floor and one rotated: origins inside glass,
    and NaN directions after total internal reflection."""
    from cuda_pathtracer_amd import CUBE
    m = _materials(sc)
    _shell(sc, m)
    sc.add_geom(CUBE, m["glass"], (-2, 1.505, 0), (0, 0, 0), (3, 3, 3))
    sc.add_geom(CUBE, m["glass"], (2.2, 3, 1), (20, 35, 10), (2.5, 2.5, 2.5))
    sc.set_camera((56, 48), 45.0, EYE, LOOK, (0, 1, 0))


def _turned(sc):
    """Every wall turned by a multiple of 90 degrees about some axis (cosines of +-4.4e-8 and sines of
    -8.7e-8 / 1.2e-8 in float next to a 0.01 : 10 scale)."""
    from cuda_pathtracer_amd import CUBE, SPHERE
    m = _materials(sc)
    sc.add_geom(CUBE, m["light"], (0, 10, 0), (0, 0, 0), (3, 0.3, 3))
    sc.add_geom(CUBE, m["white"], (0, 0, 0), (180, 0, 0), (10, 0.01, 10))
    sc.add_geom(CUBE, m["white"], (0, 10, 0), (0, 0, 270), (0.01, 10, 10))
    sc.add_geom(CUBE, m["white"], (0, 5, -5), (0, 90, 0), (0.01, 10, 10))
    sc.add_geom(CUBE, m["green"], (5, 5, 0), (90, 0, 0), (0.01, 10, 10))
    sc.add_geom(CUBE, m["red"], (-5, 5, 0), (0, 180, 180), (0.01, 10, 10))
    sc.add_geom(SPHERE, m["mirror"], (1, 4, -1), (0, 0, 0), (3, 3, 3))
    sc.set_camera((56, 48), 45.0, EYE, LOOK, (0, 1, 0))


def _tilted(sc):
    """Walls that are 10-unit cubes around the room, each tilted by 0.003 degrees: the alignment test
    accepts them (5.2e-5 of the row's axis), and the hull is 5e-4 wider than the cube — wider than the
    departure offsets, so the claim mostly rests; the bits may not move."""
    from cuda_pathtracer_amd import CUBE, SPHERE
    m = _materials(sc)
    sc.add_geom(CUBE, m["light"], (0, 9.9, 0), (0, 0, 0), (3, 0.3, 3))
    sc.add_geom(CUBE, m["white"], (0, -5, 0), (0, 0, 0.003), (10, 10, 10))
    sc.add_geom(CUBE, m["white"], (0, 15, 0), (0.003, 0, 0), (10, 10, 10))
    sc.add_geom(CUBE, m["white"], (0, 5, -10), (0, 0.003, 0), (10, 10, 10))
    sc.add_geom(CUBE, m["green"], (10, 5, 0), (0, 0.003, 0.003), (10, 10, 10))
    sc.add_geom(CUBE, m["red"], (-10, 5, 0), (0, 0, -0.003), (10, 10, 10))
    sc.add_geom(CUBE, m["white"], (0, 5, 10), (-0.003, 0, 0), (10, 10, 10))   # closed: the camera is inside
    sc.add_geom(SPHERE, m["mirror"], (-1, 4, -1), (0, 0, 0), (3, 3, 3))
    sc.set_camera((56, 48), 45.0, (0, 5, 4.5), LOOK, (0, 1, 0))


def _thick(sc):
    """Walls one unit thick (the light hangs below the ceiling's inner face at 9.5)."""
    m = _materials(sc)
    _plain_room(sc, m, 1.0, half=5.5, light_y=9.3)
    sc.set_camera((56, 48), 45.0, EYE, LOOK, (0, 1, 0))


def _thin(sc):
    """Walls 1e-4 thick: mu is 0.4 of the object-space slab, 4e-5 in the world."""
    m = _materials(sc)
    _plain_room(sc, m, 1e-4)
    sc.set_camera((56, 48), 45.0, EYE, LOOK, (0, 1, 0))


def _far(sc):
    """The shell and the camera moved a few hundred units away: ulp(coordinate) (3e-5 at 400) nears the
    1e-4 offsets and mu grows past them.  The claims may vanish; the bits may not change."""
    from cuda_pathtracer_amd import SPHERE
    m = _materials(sc)
    off = (300, -200, 400)
    _shell(sc, m, off)
    sc.add_geom(SPHERE, m["mirror"], _add(sc, (-1, 4, -1), off), (0, 0, 0), (3, 3, 3))
    sc.set_camera((56, 48), 45.0, _add(sc, EYE, off), _add(sc, LOOK, off), (0, 1, 0))


# name -> (builder, flags, least number of walls the host must group, the claim must fire)
CASES = {
    "cornell": (_cornell, dict(), 5, True),
    "grazing": (_grazing, dict(aperture=1.0, focal_len=4.0), 5, True),
    "axis_parallel": (_axis_parallel, dict(SSAA=False, DoF=False), 6, False),
    "outside": (_outside, dict(), 5, True),
    "glass": (_glass, dict(), 5, True),
    "turned": (_turned, dict(), 5, True),
    "tilted": (_tilted, dict(), 3, False),
    "thick": (_thick, dict(), 5, False),
    "thin": (_thin, dict(), 5, False),
    "far": (_far, dict(), 3, False),
}


def _make(name, oracle_only=False):
    how = CASES[name][0]
    o = O.OracleScene()
    how(o)
    o.depth = DEPTH
    if oracle_only:
        return None, o
    from cuda_pathtracer_amd import Scene
    s = Scene()
    how(s)
    s.set_render(PASSES * SPP, DEPTH, name)
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
        fl = _oflags(_gui(sortbyMaterial=sort, **CASES[name][1]))
        img, live = None, [0] * DEPTH
        for k in range(PASSES):
            img, lv = O.render_pass(o, fl, 1 + SPP * k, spp=SPP, image=img)
            live = [a + b for a, b in zip(live, lv)]
        img.setflags(write=False)
        _REF[key] = (img, live)
    return _REF[key]


def _render(name, sort):
    from cuda_pathtracer_amd import PathTracer
    s, _ = _make(name)
    pt = PathTracer(s, _gui(sortbyMaterial=sort, **CASES[name][1]), spp=SPP)
    walls = pt.room_info()["walls"]
    for k in range(PASSES):
        pt.render_pass(1 + SPP * k)
    img, st, cnt = pt.image(), pt.stats(), pt.depart_counts()
    pt.free()
    return img, st, cnt, walls


def _assert_same(name, img, ref):
    same = (img == ref) | (np.isnan(img) & np.isnan(ref))
    bad = np.argwhere(~same)
    assert bad.size == 0, f"{name}: {len(bad)} mismatching values, first at {bad[:3].tolist()}"


@pytest.mark.parametrize("sort", [False, True], ids=["fused", "sorted"])
@pytest.mark.parametrize("name", list(CASES))
def test_depart_bitexact(name, sort):
    img, st, cnt, walls = _render(name, sort)
    ref, live = _reference(name, sort)
    assert walls >= CASES[name][2], walls
    _assert_same(name, img, ref)
    assert st["bounce_live"][:DEPTH] == live
    assert all(v > 0 for v in live), live
    assert ref.sum() > 0
    assert cnt["room"] == 0   # the shipped kernels do not count


@pytest.mark.parametrize("sort", [False, True], ids=["split", "sorted"])
@pytest.mark.parametrize("name", list(CASES))
def test_depart_verified(name, sort, monkeypatch):
    """Every ray's bounded closest hit equals the plain loop's, in the split pipeline (the fused
    kernel's rays) and in the sorted producer; where the case is built for it, the tight plane alone
    removed a wall for some rays."""
    monkeypatch.setenv("PT_AMD_VERIFY_BOUNDS", "1")
    monkeypatch.setenv("PT_PIPELINE", "split")
    img, st, cnt, walls = _render(name, sort)
    ref, live = _reference(name, sort)
    print(name, "sorted" if sort else "split", "walls", walls, "counts", cnt, "segments", st["segments"])
    assert st["bound_mismatch"] == 0
    assert st["segments"] == sum(live)
    _assert_same(name, img, ref)
    if CASES[name][3]:
        assert cnt["room"] > 0


def test_depart_off_knob(monkeypatch):
    """PT_AMD_ROOM_DEPART=0: the same room, the same image, no claim."""
    monkeypatch.setenv("PT_AMD_ROOM_DEPART", "0")
    ref, live = _reference("cornell", False)
    img, st, _, walls = _render("cornell", False)
    assert walls == 5
    _assert_same("cornell", img, ref)
    assert st["bounce_live"][:DEPTH] == live
    monkeypatch.setenv("PT_AMD_VERIFY_BOUNDS", "1")
    monkeypatch.setenv("PT_PIPELINE", "split")
    img, st, cnt, _ = _render("cornell", False)
    _assert_same("cornell", img, ref)
    assert st["bound_mismatch"] == 0 and st["segments"] == sum(live)
    assert cnt["room"] == 0
