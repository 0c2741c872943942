"""The scene families shared by tests/test_bound_pairs_gpu.py (the device's per-pair check of every
bound form, and renders against the oracle) and tests/test_bound_cases_cpu.py (the host's scene
preparation alone): scenes on the edges of the error analysis behind the bounded closest hit
(pt_bounds.cpp update_bounds).

Every builder takes any scene object with add_material / add_geom / set_camera — the product's Scene
or the oracle's — and adds at most 32 geoms (the bounded pass's table).  FAMILIES maps a name to a
Family: the builder, the flags its renders use, the bound kinds it must produce (1 oriented cube, 2
sphere, 3 world-box cube, 4 uniformly scaled sphere, "room" a grouped room) and, for the two families
that approach a classification threshold, the kind each listed geom must get.
"""
import atexit
import json
import shutil
import tempfile
from collections import namedtuple
from pathlib import Path

import numpy as np

RES, DEPTH, SPP, PASSES = (48, 36), 6, 2, 2   # passes start at iterations 1 and 3
EYE, LOOK = (0.0, 5.0, 10.5), (0.0, 5.0, 0.0)
CUBE, SPHERE = 1, 0                            # (cuda_pathtracer_amd.CUBE / SPHERE, the reference's GeomType)

Family = namedtuple("Family", "build flags kinds geom_kinds")


def _materials(sc):
    return dict(light=sc.add_material(rgb=(1, 1, 1), emittance=5.0),
                white=sc.add_material(rgb=(0.98, 0.98, 0.98)),
                red=sc.add_material(rgb=(0.85, 0.35, 0.35)),
                green=sc.add_material(rgb=(0.35, 0.85, 0.35)),
                mirror=sc.add_material(rgb=(0.98, 0.98, 0.98), specrgb=(0.98, 0.98, 0.98), reflective=1.0),
                glass=sc.add_material(rgb=(0.98, 0.98, 0.98), specrgb=(0.98, 0.98, 0.98), refractive=1.0, ior=1.5))


_CYCLE = ("white", "mirror", "glass", "red", "green")


class _Moved:
    """A scene seen through a uniform scale and a translation: every geom's translation and scale and the
    camera's eye and target are multiplied by `scale` and moved by `shift`; the camera's resolution (and,
    when given, its eye and target before the move) are the family's own."""

    def __init__(self, sc, scale=1.0, shift=(0.0, 0.0, 0.0), eye=None, look=None):
        self.sc, self.scale, self.shift, self.eye, self.look = sc, float(scale), shift, eye, look

    def _at(self, p):
        return tuple(float(v) * self.scale + float(d) for v, d in zip(p, self.shift))

    def add_material(self, *a, **kw):
        return self.sc.add_material(*a, **kw)

    def add_geom(self, type_, material, trans, rotat, scale):
        return self.sc.add_geom(type_, material, self._at(trans), rotat, tuple(float(v) * self.scale for v in scale))

    def set_camera(self, res, fovy, eye, lookat, up=(0, 1, 0)):
        self.sc.set_camera(RES, fovy, self._at(self.eye or eye), self._at(self.look or lookat), up)


def _json_scene(sc, path):
    """A scene file's materials, objects and camera through add_material / add_geom / set_camera, as the
    loaders read them (materials in name order, the refraction extension on)."""
    data = json.loads(Path(path).read_text())
    ids = {}
    for name in sorted(data["Materials"]):
        p = data["Materials"][name]
        rgb = p.get("RGB", [0.0, 0.0, 0.0])
        ids[name] = sc.add_material(rgb=rgb, specrgb=p.get("SPECRGB", rgb), specex=p.get("SPECEX", 1.0),
                                    reflective=p.get("REFLECTIVE", 0.0), emittance=p.get("EMITTANCE", 0.0),
                                    refractive=p.get("REFRACTIVE", 0.0), ior=p.get("IOR", 0.0))
    for o in data["Objects"]:
        sc.add_geom({"sphere": SPHERE, "cube": CUBE}[o["TYPE"]], ids.get(o["MATERIAL"], 0), o["TRANS"], o["ROTAT"],
                    o["SCALE"])
    c = data["Camera"]
    sc.set_camera(RES, c["FOVY"], c["EYE"], c["LOOKAT"], c["UP"])


_GENERATED = {}


def _random_primitives(**kw):
    """scenes.random_primitives' file for these arguments (written once, to a directory of its own)."""
    key = tuple(sorted(kw.items()))
    if key not in _GENERATED:
        from cuda_pathtracer_amd import scenes
        d = tempfile.mkdtemp(prefix="bound_cases_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        _GENERATED[key] = scenes.random_primitives(d, res=RES, depth=DEPTH, **kw)
    return _GENERATED[key]


def _base(sc):
    """scenes.random_primitives as it is: the Cornell shell and 24 rotated cubes and spheres, 30 geoms."""
    _json_scene(sc, _random_primitives(n=24, seed=7))


def _small(sc):
    _base(_Moved(sc, 2.0 ** -10))


def _large(sc):
    _base(_Moved(sc, 2.0 ** 10))


def _offset(sc):
    """At these coordinates one float step is 2^-10 to 2^-11: the 1e-4 offsets are below it."""
    _base(_Moved(sc, 1.0, (1e4, -3e3, 7e3)))


def _lit_floor(sc, m):
    sc.add_geom(CUBE, m["light"], (0, 10, 0), (0, 0, 0), (6, 0.3, 6))
    sc.add_geom(CUBE, m["white"], (0, 0, 0), (0, 0, 0), (14, 0.01, 14))


def _needles(sc):
    """Cubes and spheres whose scales differ by up to 1e-4 : 1e2 between axes, under arbitrary rotations:
    object-space origins of 1e5 and more, where the exact tests' own differences cancel (the reference's
    sphere test then reports hits far from the sphere, and the renderer follows it).  glm's float inverse
    stays good for these maps (transform * inverse is I within 1e-6), so tslack does not drop."""
    m = _materials(sc)
    _lit_floor(sc, m)
    rng = np.random.default_rng(31)
    ratios = [(1e-4, 1.0, 1e2), (1e2, 1e-4, 1.0), (1.0, 1e2, 1e-4), (1e-3, 1e2, 1e-1), (1e1, 1e-3, 1e-3),
              (1e-4, 1e-4, 1e2), (1e2, 1e2, 1e-4), (3e-4, 3.0, 30.0), (1e-2, 1e2, 1e-2), (50.0, 2e-3, 0.5),
              (1e-4, 0.5, 0.5), (2.0, 2.0, 1e-4)]
    for k, s in enumerate(ratios):
        for typ in (CUBE, SPHERE):
            sc.add_geom(typ, m[_CYCLE[(2 * k + typ) % len(_CYCLE)]],
                        [float(v) for v in rng.uniform((-4.0, 1.0, -4.0), (4.0, 8.0, 2.0))],
                        [float(v) for v in rng.uniform(0.0, 360.0, 3)], s)
    sc.set_camera(RES, 45.0, EYE, LOOK, (0, 1, 0))


# nearly_aligned.  update_bounds calls a cube axis-aligned (bkind 3) when every row of the exact inverse X
# of its float map has one entry above 1e-4 of the row's largest.  X's entries are rotation entry x scale:
#  - scale 1:1:1 (or a rotation about the axis of the odd scale): the second entry of a row is tan(angle)
#    of the first, so the threshold is atan(1e-4) = 5.73e-3 degrees: 0, 1e-3 and 5e-3 degrees stay bkind 3,
#    6e-3, 1e-2 and 0.1 degrees become bkind 1 (tan(5e-3 deg) = 8.73e-5, tan(6e-3 deg) = 1.047e-4: 5 and 13 %
#    from the threshold, against 1e-7 of float rounding).  ROTAT 90 has cos = -4.4e-8 in float: bkind 3.
#  - scale 0.002 : 2 : 2 turned about z, which mixes the thin axis with a long one: the row holds
#    0.002 cos and 2 sin, a ratio of 1000 tan(angle), above 1e-4 from 5.7e-6 degrees on: every nonzero
#    small angle is bkind 1; 0 is bkind 3, and 90 degrees has the ratios 4.4e-5 and 4.4e-11: bkind 3 (the
#    Cornell ceiling's case, with its 1 : 1000 ratio).
_ANGLES = (0.0, 90.0, 1e-3, 5e-3, 6e-3, 1e-2, 0.1)
_ALIGNED_KINDS = {}


def _nearly_aligned(sc):
    m = _materials(sc)
    _lit_floor(sc, m)
    rows = (("cube", (1.2, 1.2, 1.2), 2, (3, 3, 3, 3, 1, 1, 1)),      # about z
            ("wall_z", (0.002, 2.0, 2.0), 2, (3, 3, 1, 1, 1, 1, 1)),  # about z: thin axis into a long one
            ("wall_x", (0.002, 2.0, 2.0), 0, (3, 3, 3, 3, 1, 1, 1)))  # about x: the two long axes
    for r, (name, scale, axis, kinds) in enumerate(rows):
        for k, ang in enumerate(_ANGLES):
            rot = [0.0, 0.0, 0.0]
            rot[axis] = ang
            g = sc.add_geom(CUBE, m[_CYCLE[(k + r) % len(_CYCLE)]], (-4.5 + 1.5 * k, 1.5 + 2.5 * r, -1.0 - r), rot, scale)
            _ALIGNED_KINDS[g] = kinds[k]
    sc.set_camera(RES, 45.0, EYE, LOOK, (0, 1, 0))


# nearly_uniform.  A sphere is bkind 4 when G = L^T L (L: the linear part of the float inverse) is within
# 2^-20 of (tr G / 3) I, relative.  With scale (s, s, s (1 + e)), G's diagonal is (1, 1, (1 + e)^-2) / s^2:
# the mean is (1 - 2 e / 3) / s^2 and the largest deviation 4 e / 3 of it, so the threshold is
# e = 0.75 * 2^-20 = 7.2e-7; the float rounding of the rotated map's nine entries moves G by a few 2^-24
# (about 2e-7 relative).  e = 0 and 2^-22 (deviation 3.2e-7 + rounding) stay bkind 4; e = 2^-19, 2^-18 and
# 2^-12 (deviation >= 2.5e-6) are bkind 2.  e = 2^-21 and 2^-20 (6.4e-7 and 1.3e-6 before rounding) lie
# within the rounding of the threshold: either kind, and their bounds are checked whichever they get.
_EPS = (0.0, 2.0 ** -22, 2.0 ** -21, 2.0 ** -20, 2.0 ** -19, 2.0 ** -18, 2.0 ** -12)
_EPS_KIND = (4, 4, None, None, 2, 2, 2)
_UNIFORM_KINDS = {}


def _nearly_uniform(sc):
    m = _materials(sc)
    _lit_floor(sc, m)
    rng = np.random.default_rng(47)
    for r, s in enumerate((1e-3, 1.0, 1e3)):
        for k, e in enumerate(_EPS):
            s32 = np.float32(s)
            sz = np.float32(float(s32) * (1.0 + e))   # (exact in double, rounded once: s (1 + e) as a float)
            if s == 1.0:
                pos = (-4.5 + 1.5 * k, 2.0 + 0.6 * (k % 3), -1.0)
            elif s < 1.0:
                pos = (-0.003 + 0.001 * k, 5.0, 10.49)   # in front of the lens
            else:
                pos = (0.3 * k, 5.0, 0.0)                # around everything, the camera included
            g = sc.add_geom(SPHERE, m[_CYCLE[(k + r) % len(_CYCLE)]], pos, [float(v) for v in rng.uniform(0.0, 360.0, 3)],
                            (float(s32), float(s32), float(sz)))
            _UNIFORM_KINDS[g] = _EPS_KIND[k]
    sc.set_camera(RES, 45.0, EYE, LOOK, (0, 1, 0))


def _mixed_sizes(sc):
    """Geoms of size 1e-3 and of size 1e3 in one scene, of every bound kind; the large ones enclose the
    camera, the small ones sit in front of it."""
    m = _materials(sc)
    _lit_floor(sc, m)
    big, tiny = 1e3, 1e-3
    kinds = ((CUBE, (0, 0, 0), (1, 1, 1)), (CUBE, (20, 35, 10), (1, 1, 1)), (SPHERE, (15, 40, 70), (1, 1, 1)),
             (SPHERE, (25, 5, 50), (1, 0.7, 1.3)))
    for k, (typ, rot, sh) in enumerate(kinds):
        sc.add_geom(typ, m["white" if k % 2 else "light"], (3.0 * k, 5.0 + 2.0 * k, -1.0 * k), rot,
                    tuple(big * (1.0 + 0.1 * k) * v for v in sh))
        sc.add_geom(typ, m[_CYCLE[k % len(_CYCLE)]], (-0.003 + 0.002 * k, 5.0, 10.49), rot, tuple(tiny * v for v in sh))
        sc.add_geom(typ, m[_CYCLE[(k + 1) % len(_CYCLE)]], (-3.0 + 2.0 * k, 2.0, 0.0), rot, tuple(1.5 * v for v in sh))
    sc.set_camera(RES, 45.0, EYE, LOOK, (0, 1, 0))


def _coincident(sc):
    """Identical geoms, nested geoms and geoms that share a face, aligned and rotated."""
    m = _materials(sc)
    _lit_floor(sc, m)
    rot = (20.0, 35.0, 10.0)
    for r, x in ((0, -3.0), (1, 3.0)):
        ro = rot if r else (0.0, 0.0, 0.0)
        sc.add_geom(CUBE, m["red"], (x, 2.0, 0.0), ro, (2, 2, 2))        # identical twice
        sc.add_geom(CUBE, m["green"], (x, 2.0, 0.0), ro, (2, 2, 2))
        sc.add_geom(CUBE, m["glass"], (x, 2.0, 0.0), ro, (3, 3, 3))      # around them
        sc.add_geom(SPHERE, m["mirror"], (x, 6.0, -1.0), ro, (2, 2, 2))  # identical twice
        sc.add_geom(SPHERE, m["white"], (x, 6.0, -1.0), ro, (2, 2, 2))
        sc.add_geom(SPHERE, m["glass"], (x, 6.0, -1.0), ro, (3, 3, 3))   # around them
        sc.add_geom(SPHERE, m["red"], (x, 8.5, -1.0), ro, (1.0, 2.0, 1.5))
        sc.add_geom(SPHERE, m["glass"], (x, 8.5, -1.0), ro, (2.0, 4.0, 3.0))
    sc.add_geom(CUBE, m["white"], (-0.5, 1.0, 2.0), (0, 0, 0), (1, 1, 1))   # share the face x = 0
    sc.add_geom(CUBE, m["mirror"], (0.5, 1.0, 2.0), (0, 0, 0), (1, 1, 1))
    sc.add_geom(CUBE, m["white"], (-0.5, 4.0, 2.0), (0, 0, 30), (1, 1, 1))  # share a face, rotated about z
    sc.add_geom(CUBE, m["mirror"], (-0.5 + 0.8660254, 4.5, 2.0), (0, 0, 30), (1, 1, 1))
    sc.set_camera(RES, 45.0, EYE, LOOK, (0, 1, 0))


def _room_case(name, scale=1.0, eye=None, look=None):
    import room_cases

    def build(sc):
        how = room_cases.CASES[name][0]
        moved = _Moved(sc, scale, eye=eye, look=look)
        if how is None:
            _json_scene(moved, Path(__file__).resolve().parent / "scenes" / "cornell.json")
        elif isinstance(how, dict):
            _json_scene(moved, _random_primitives(**how))
        else:
            how(moved)
    return build


def _room_flags(name):
    import room_cases
    return dict(room_cases.CASES[name][1])


FAMILIES = {
    "base": Family(_base, {}, {1, 2, 3, 4, "room"}, None),
    "small": Family(_small, {}, {1, 2, 3, 4, "room"}, None),
    "large": Family(_large, {}, {1, 2, 3, 4, "room"}, None),
    "offset": Family(_offset, {}, {1, 2, 3, 4, "room"}, None),
    "needles": Family(_needles, {}, {1, 2, 3}, None),
    "nearly_aligned": Family(_nearly_aligned, {}, {1, 3}, _ALIGNED_KINDS),
    "nearly_uniform": Family(_nearly_uniform, {}, {2, 3, 4}, _UNIFORM_KINDS),
    "mixed_sizes": Family(_mixed_sizes, {}, {1, 2, 3, 4}, None),
    "coincident": Family(_coincident, {}, {1, 2, 3, 4}, None),
}
# rooms: the cases of room_cases.py that find a room, one of them again 2^10 times the size, and one with
# the camera outside the room, looking in through the open face from well beyond it
_ROOM_KINDS = {   # beside the walls (3, room): a sphere of one scale is 4, a rotated cube 1
    "cornell": {4}, "inside_aperture": {4}, "axis_parallel": set(), "window": {4}, "outside": {1, 4},
    "coplanar_floor": {4}, "glass_cube": {1}, "random_primitives_room": {1, 2, 4},
}
for _name, (_how, _flags, _want) in __import__("room_cases").CASES.items():
    if _want != 0:
        FAMILIES["rooms_" + _name] = Family(_room_case(_name), _room_flags(_name), {3, "room"} | _ROOM_KINDS[_name], None)
FAMILIES["rooms_glass_cube_x1024"] = Family(_room_case("glass_cube", 2.0 ** 10), {}, {1, 3, "room"}, None)
FAMILIES["rooms_inside_aperture_from_outside"] = Family(_room_case("inside_aperture", eye=(2.0, 6.0, 30.0), look=LOOK),
                                                        {}, {3, 4, "room"}, None)


def far_camera(sc, eye_z):
    """cornell.json's geoms seen along -z from (0, 5, eye_z) (None: the file's own camera).  Beyond
    Scene.bound_info()'s r_limit the arithmetic of the sphere's bound forms would overflow."""
    cornell = Path(__file__).resolve().parent / "scenes" / "cornell.json"
    if eye_z is None:
        _json_scene(sc, cornell)
    else:
        _json_scene(_Moved(sc, eye=(0.0, 5.0, float(eye_z)), look=LOOK), cornell)


def make_far_camera(eye_z, oracle=False):
    if oracle:
        o = make_oracle(None, lambda sc: far_camera(sc, eye_z))
        return o
    from cuda_pathtracer_amd import Scene
    s = Scene()
    far_camera(s, eye_z)
    s.set_render(PASSES * SPP, DEPTH, "far_camera")
    s.finalize()
    return s


def make_scene(name):
    """The product's Scene of a family."""
    from cuda_pathtracer_amd import Scene
    s = Scene()
    FAMILIES[name].build(s)
    s.set_render(PASSES * SPP, DEPTH, name)
    s.finalize()
    return s


def make_oracle(name, build=None):
    from oracle import binding as O
    o = O.OracleScene()
    (build or FAMILIES[name].build)(o)
    o.depth = DEPTH
    return o


def gui(**kw):
    from cuda_pathtracer_amd import GuiDataContainer
    g = GuiDataContainer()
    for k, v in kw.items():
        setattr(g, k, v)
    return g
