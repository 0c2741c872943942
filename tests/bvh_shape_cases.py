"""Small scenes whose flattened BVH has a degenerate shape (a helper, not collected by pytest).

The walk a context runs is chosen by the tree's shape (DESIGN.md §4.3 "degenerate shapes"): a leaf of
more than 255 triangles leaves the pair and the quad layout off, the tree's depth picks the stack of
the inline walk and lets k_traverse drop the pair walk, a stack bound past 64 leaves the quad layout
off, and a root that is a leaf has no interior entry at all.  Each case here lands in one of those
classes; classify() reads the class back from the flattened tree, and every test asserts it.

A scene is one mesh geom, an emissive cube (the light, behind the camera) and a sphere; every triangle has one texture coordinate of
its own at all three corners (uv_of), so the G-buffer's uv names the triangle.

Big leaves (build_bvh makes a leaf of a whole range when its centre box is degenerate, BVH_tree.cpp:46):
    every triangle of the leaf has the box [c - h, c + h] about one common centre c on all three axes
    (h per triangle and axis), with coordinates on a 2^-10 grid so that min + max is exact.  A few are
    large and face the camera; the many others are small, lie around c and are hidden behind the
    large ones.  Loose triangles on both sides in x put leaves before and after the big one in
    triangle order: its `first` is > 0, and a wrapped leaf code lands in other leaves' triangles.
Chains (the SAH split peels exactly the largest triangle per level):
    level e has its box centre at 2^(e - 10) on axis e mod 3 and 0 on the other two, and half that size:
    along the split axis every other centre lies in region 0 (a ratio of 8 per axis, above 7), so
    split 0 wins and the right child is the leaf of the largest triangle.  n triangles give n - 1
    interior nodes, one per depth 0 .. n - 2.  The x levels lie on -x (the camera's orbit keeps it at
    x >= its look-at point).  The camera sits at the small end and looks along (-1, 1, 1): rays with
    d_x <= 0, d_y >= 0, d_z >= 0 descend to the smallest triangle first and push one entry per level;
    with the sign of an axis the other way the near child on that axis' levels is the peeled leaf, and
    those levels leave nothing on the stack.

`depth` is the context's bvh_depth: the depth of the deepest INTERIOR node (root = 0), the number the
kernels' dispatch compares (pt_create); the deepest leaf lies one level below.  chainN has depth N.
"""
import ctypes as C
import json
from pathlib import Path

import numpy as np

import cuda_pathtracer_amd as P
from cuda_pathtracer_amd import _native as N
from oracle import binding as O

RES = (32, 24)
GRID = 2.0 ** -10
MESH_MAT, CUBE_MAT, SPHERE_MAT = 0, 1, 2      # material ids: the names sort as m0 < m1 < m2


def uv_of(i):
    """Triangle i's texture coordinate (all three corners): distinct from every other by >= 2^-9."""
    return ((i + 1) / 512.0, ((5 * i) % 16 + 1) / 32.0)


# ---- triangles ------------------------------------------------------------------------------------------------
def _sheet(c, h, s, mirror=False):
    """A triangle facing +z whose box is [c - (h, h, s), c + (h, h, s)]; its plane passes c + (0, 0, s/2)."""
    z = (-s, s) if mirror else (s, -s)        # (mirror: tilted the other way in x)
    return np.array([[-h, -h, z[0]], [h, -h, z[1]], [0.0, h, s]]) + np.asarray(c, np.float64)


def _big_leaf(c, n, big=6):
    """n triangles with one common box centre c: `big` large sheets, nested with the smaller in front,
    and n - big small ones within 2^-4 of c, behind every large sheet's plane."""
    out = []
    for k in range(big):
        h = 2.0 - 0.25 * k
        out.append(_sheet(c, h, 0.25 + 0.125 * k, mirror=k % 2 == 1))
    for j in range(n - big):
        h = 2.0 ** -6 * (1 + (j % 8) / 8.0)
        s = 2.0 ** -7 * (1 + (j % 5))
        out.append(_sheet(c, h, s, mirror=j % 3 == 0))
    v = np.array(out)
    assert np.array_equal(v / GRID, np.round(v / GRID))
    return v


def _loose(rng, n, xlo, xhi):
    """n random triangles of size about 1 facing +z with centres in [xlo, xhi] x [-2.5, 2.5] x [-1, 1]."""
    cen = np.stack([rng.uniform(xlo, xhi, n), rng.uniform(-2.5, 2.5, n), rng.uniform(-1, 1, n)], -1)
    v = cen[:, None, :] + rng.uniform(-0.6, 0.6, (n, 3, 3)) * np.array([1.0, 1.0, 0.4])
    v = np.round(v / GRID) * GRID
    flip = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])[:, 2] < 0
    v[flip] = v[flip][:, [0, 2, 1]]
    return v


def _chain(n, mirror_x=True):
    out = []
    for e in range(n):
        c = 2.0 ** (e - 10)
        h = c / 4
        t = np.roll(np.array([[c - h, h, 0.0], [c + h, 0.0, -h], [c, -h, h]]), e % 3, axis=1)
        if mirror_x:
            t[:, 0] = -t[:, 0]                 # x levels lie on -x: the camera's orbit keeps it at x >= look-at
            t = t[[0, 2, 1]]                   # (the mirror turned the winding: faces (1, -1, -1) again)
        out.append(t)
    v = np.array(out)
    face = np.array([1.0, -1.0, -1.0]) if mirror_x else np.array([-1.0, -1.0, -1.0])
    assert (np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]) @ face > 0).all()
    return v


def orbit_eye(eye, lookat):
    """The EYE to ask for so that the camera ends at `eye`: the loaded view is put on runCuda's orbit
    (main.cpp:59-73 and 117-136), which keeps its angles as arc cosines and so mirrors the eye about the
    look-at point in y and, where the view has x > 0, in x.  `eye` must lie at x > look-at's."""
    cp = np.asarray(eye, np.float64) - np.asarray(lookat, np.float64)
    zoom = np.linalg.norm(cp)
    assert cp[0] > 0 and cp[2] != 0
    theta, phi = np.arccos(cp[1] / zoom), np.arctan2(cp[0], cp[2])
    vz = -np.cos(phi)
    v = np.array([np.sin(phi), abs(vz) * np.cos(theta) / np.sin(theta), vz])
    return tuple((np.asarray(lookat, np.float64) - zoom * v / np.linalg.norm(v)).tolist())


BIG_VIEW = dict(eye=(0.5, 0.3, 12.0), lookat=(0.0, 0.0, 0.0), fovy=17.0,
                cube=((0.0, 0.0, 20.0), (30.0, 30.0, 0.5)), sphere=((2.5, -1.5, 1.5), 0.5))
ROOT_VIEW = dict(eye=(0.5, 0.3, 12.0), lookat=(0.0, 0.0, 0.0), fovy=11.0,
                 cube=((0.0, 0.0, 20.0), (30.0, 30.0, 0.5)), sphere=((1.2, -1.0, 1.5), 0.3))
_E = 2.0 ** -6
CHAIN_VIEW = dict(eye=(_E, -_E, -_E), lookat=(-1.0, 1.0, 1.0), fovy=40.0,
                  cube=((4.0, -4.0, -4.0), (6.0, 6.0, 6.0)), sphere=((-0.5, 0.1, 0.1), 0.06))


def _leaf_case(sizes):
    def make():
        rng = np.random.default_rng(300 + sum(sizes))
        if len(sizes) == 1:
            return np.concatenate([_big_leaf((0.0, 0.0, 0.0), sizes[0]), _loose(rng, 20, -4.5, -2.6), _loose(rng, 20, 2.6, 4.5)])
        return np.concatenate([_big_leaf((-2.5, 0.0, 0.0), sizes[0]), _big_leaf((2.5, 0.0, 0.0), sizes[1]),
                               _loose(rng, 14, -7, -5), _loose(rng, 14, 5, 7), _loose(rng, 6, -0.3, 0.3)])
    return make


# name -> (triangles, view, expected class: dict of classify() keys that must match, quad table expected)
CASES = {
    "leaf255": (_leaf_case([255]), BIG_VIEW, dict(largest_leaf=255, big_leaves=0, root_leaf=False), True),
    "leaf256": (_leaf_case([256]), BIG_VIEW, dict(largest_leaf=256, big_leaves=1, root_leaf=False), False),
    "leaf300": (_leaf_case([300]), BIG_VIEW, dict(largest_leaf=300, big_leaves=1, root_leaf=False), False),
    "leaf300x2": (_leaf_case([300, 300]), dict(BIG_VIEW, fovy=26.0), dict(largest_leaf=300, big_leaves=2, root_leaf=False), False),
    "root1": (lambda: _big_leaf((0.0, 0.0, 0.0), 1, big=1), ROOT_VIEW, dict(depth=0, largest_leaf=1, root_leaf=True), True),
    "root5": (lambda: _big_leaf((0.0, 0.0, 0.0), 5, big=5), ROOT_VIEW, dict(depth=0, largest_leaf=5, root_leaf=True), True),
    "chain30": (lambda: _chain(32), CHAIN_VIEW, dict(depth=30, largest_leaf=1, root_leaf=False), True),
    "chain31": (lambda: _chain(33), CHAIN_VIEW, dict(depth=31, largest_leaf=1, root_leaf=False), True),
    "chain32": (lambda: _chain(34), CHAIN_VIEW, dict(depth=32, largest_leaf=1, root_leaf=False), True),
    "chain61": (lambda: _chain(63), CHAIN_VIEW, dict(depth=61, largest_leaf=1, root_leaf=False), True),
    "chain62": (lambda: _chain(64), CHAIN_VIEW, dict(depth=62, largest_leaf=1, root_leaf=False), True),
    "chain63": (lambda: _chain(65), CHAIN_VIEW, dict(depth=63, largest_leaf=1, root_leaf=False), True),
    "chain_over": (lambda: _chain(71), CHAIN_VIEW, dict(depth=69, largest_leaf=1, root_leaf=False), False),
}
BIG = ("leaf256", "leaf300", "leaf300x2")
# For the device builder only (never walked in view): the same chains with the x levels on +x.  On a
# mirrored level the peeled leaf is the LEFT child, which k_bvh_small finishes before it goes on, so the
# mirrored chains fill only two thirds of its task stack; here every level leaves one task pending.
BUILDER_CASES = {
    "chain62_pos": (lambda: _chain(64, mirror_x=False), CHAIN_VIEW, dict(depth=62, largest_leaf=1, root_leaf=False), True),
    "chain63_pos": (lambda: _chain(65, mirror_x=False), CHAIN_VIEW, dict(depth=63, largest_leaf=1, root_leaf=False), True),
}


def case_of(name):
    return CASES[name] if name in CASES else BUILDER_CASES[name]


# ---- scene files ----------------------------------------------------------------------------------------------
def scene_file(tmp, case, emissive=False, depth=4):
    """Writes the case's OBJ and JSON under tmp; returns the JSON's path.  emissive=True: every material
    emits its own colour and the trace depth is 1, so one iteration shows the geom of every pixel."""
    tris, view, _, _ = case_of(case)
    v = tris()
    d = Path(tmp) / (case + ("_e" if emissive else ""))
    (d / "Models").mkdir(parents=True, exist_ok=True)
    lines = [f"v {x:.17g} {y:.17g} {z:.17g}" for x, y, z in v.reshape(-1, 3)]
    lines += ["vt {:.10f} {:.10f}".format(*uv_of(i)) for i in range(len(v))]
    nrm = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)                    # flat: the front side's unit normal
    lines += ["vn {:.9f} {:.9f} {:.9f}".format(*n) for n in nrm]
    lines += [f"f {3 * i + 1}/{i + 1}/{i + 1} {3 * i + 2}/{i + 1}/{i + 1} {3 * i + 3}/{i + 1}/{i + 1}" for i in range(len(v))]
    (d / "Models" / "shape.obj").write_text("\n".join(lines) + "\n")
    if emissive:
        mats = {"m0": {"RGB": [0.25, 0.5, 0.75], "EMITTANCE": 1.0}, "m1": {"RGB": [1.0, 0.5, 0.25], "EMITTANCE": 1.0},
                "m2": {"RGB": [0.5, 1.0, 0.125], "EMITTANCE": 1.0}}
    else:
        mats = {"m0": {"RGB": [0.8, 0.7, 0.6]}, "m1": {"RGB": [1.0, 1.0, 1.0], "EMITTANCE": 6.0},
                "m2": {"RGB": [0.4, 0.6, 0.9]}}
    (ct, cs), (st, sr) = view["cube"], view["sphere"]
    objs = [{"TYPE": "mesh", "MATERIAL": "m0", "OBJ_FILE": "shape.obj", "TRANS": [0, 0, 0], "ROTAT": [0, 0, 0], "SCALE": [1, 1, 1]},
            {"TYPE": "cube", "MATERIAL": "m1", "TRANS": list(ct), "ROTAT": [0, 0, 0], "SCALE": list(cs)},
            {"TYPE": "sphere", "MATERIAL": "m2", "TRANS": list(st), "ROTAT": [0, 0, 0], "SCALE": [2 * sr] * 3}]
    spec = {"Materials": mats, "Objects": objs,
            "Camera": {"RES": list(RES), "FOVY": view["fovy"], "ITERATIONS": 2, "DEPTH": 1 if emissive else depth,
                       "FILE": case, "EYE": list(orbit_eye(view["eye"], view["lookat"])), "LOOKAT": list(view["lookat"]), "UP": [0.0, 1.0, 0.0]}}
    path = d / f"{case}.json"
    path.write_text(json.dumps(spec))
    return str(path)


def _aim(sc, case):
    v = case_of(case)[1]
    sc.set_camera(RES, v["fovy"], orbit_eye(v["eye"], v["lookat"]), v["lookat"], (0, 1, 0))


def load(path, case, device_bvh=False):
    """The native scene with the case's camera (set directly: the loader's orbit does not apply)."""
    sc = P.Scene(path, device_bvh=device_bvh)
    _aim(sc, case)
    sc.finalize()
    return sc


def load_oracle(path, case):
    sc = O.OracleScene.from_json(path)
    _aim(sc, case)
    return sc


# ---- the tree's class -----------------------------------------------------------------------------------------
def nodes_of(scene):
    nn = scene.counts()[3]
    nodes = (N.BvhNode * max(nn, 1))()
    assert N.lib().pt_scene_get_bvh(scene.handle, nodes, nn) == nn
    return np.frombuffer(bytes(nodes), O.NODE_DTYPE)[:nn]


def quads_of(scene):
    """(number of quad entries, root code, stack bound) of pt_scene_bvh_quads; (0, 0, 0): no quad layout."""
    root, bound = C.c_int32(), C.c_int32()
    nq = N.lib().pt_scene_bvh_quads(scene.handle, None, 0, C.byref(root), C.byref(bound))
    assert nq >= 0
    return (nq, root.value, bound.value) if nq else (0, 0, 0)


def builder_stack(scene):
    """The task-stack entries k_bvh_small needs for this tree when one thread builds all of it (a range of
    at most 128 primitives): at every split, the right ranges still pending plus the two it pushes.
    More than 64 sets the builder's error bit 2, and the host builds."""
    pn = nodes_of(scene)
    pending = np.zeros(len(pn), np.int64)
    need = 0
    for i, n in enumerate(pn):
        if n["sub_areas"] == 0:
            need = max(need, int(pending[i]) + 2)
            pending[i + 1] = pending[i] + 1               # the left range is built first, the right one waits
            pending[int(n["rchild_idx"])] = pending[i]
    return need


def classify(scene):
    """dict(depth: of the deepest interior node (the context's bvh_depth; 0 when the root is a leaf),
    height: of the deepest leaf, largest_leaf, big_leaves: leaves over 255 triangles, root_leaf,
    big_first: `first` of the first such leaf or of the largest leaf, leaves_after: leaves behind it in
    triangle order)."""
    pn = nodes_of(scene)
    depth = np.zeros(len(pn), np.int64)
    for i, n in enumerate(pn):
        if n["sub_areas"] == 0:
            depth[i + 1] = depth[int(n["rchild_idx"])] = depth[i] + 1
    leaf = pn["sub_areas"] > 0
    sizes = pn["sub_areas"][leaf]
    firsts = pn["first_area_idx"][leaf]
    k = int(np.argmax(sizes > 255)) if (sizes > 255).any() else int(np.argmax(sizes))
    return dict(depth=int(depth[~leaf].max()) if (~leaf).any() else 0, height=int(depth.max()),
                largest_leaf=int(sizes.max()), big_leaves=int((sizes > 255).sum()), root_leaf=bool(leaf[0]),
                big_first=int(firsts[k]), leaves_after=int((firsts > firsts[k]).sum()), nodes=len(pn))
