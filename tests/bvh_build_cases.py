"""Inputs for the BVH build tests (test_bvh_build_ref_{cpu,gpu}.py): name -> load-order vertices
(n, 3, 3) float32, each with one line saying which code of the builders it aims at (bvh_build.hip's
k_bvh_big / k_bvh_small, pt_mesh.cpp's Builder).  Plain numpy; the two scene-file cases are made by
`scene_file`."""
from __future__ import annotations

from pathlib import Path

import numpy as np

SCENES = Path(__file__).resolve().parent / "scenes"


def adversarial(n, seed):
    """The recipe of test_bvh_device_gpu.py: random triangles mixed with exact duplicates of triangle 0,
    triangles collapsed to the origin, y-flat slivers and a shared x coordinate."""
    rng = np.random.default_rng(seed)
    v = rng.uniform(-3, 3, size=(n, 3, 3)).astype(np.float32)
    if n >= 3:
        k = max(1, n // 7)
        v[rng.choice(n, k, replace=False)] = v[0]
        v[rng.choice(n, k, replace=False)] = 0.0
        s = rng.choice(n, k, replace=False)
        v[s, :, 1] = v[s, :1, 1]
        v[rng.choice(n, k, replace=False), :, 0] = np.float32(1.25)
    return v


def _random(n, seed, lo=-3.0, hi=3.0):
    return np.random.default_rng(seed).uniform(lo, hi, size=(n, 3, 3)).astype(np.float32)


def _zeros_first():
    v = _random(600, 21, 0.5, 3.0)            # away from the origin, so that a union with zeros shows
    v[:50] = 0.0
    v[300:320] = 0.0
    return v


def _collinear(n, seed):
    v = _random(n, seed)
    v[:, :, 1:] = 0.0
    return v


def _lattice():
    return np.random.default_rng(23).integers(0, 8, size=(3000, 3, 3)).astype(np.float32)


def _lopsided():
    rng = np.random.default_rng(24)
    v = rng.uniform(-3, 3, size=(1500, 3, 3)).astype(np.float32)
    corner = np.array([-2.9, -2.9, -2.9], np.float32)
    v[:1400] = corner + v[:1400] / np.float32(1000.0)
    return v


def _descending():
    rng = np.random.default_rng(25)
    n = 1200
    centre = np.stack([np.linspace(3, -3, n), rng.uniform(-3, 3, n), rng.uniform(-3, 3, n)], 1)
    return (centre[:, None, :] + rng.uniform(-0.01, 0.01, size=(n, 3, 3))).astype(np.float32)


def _signed_zero(n, seed, dups):
    """Values in [0, 3] with y negated and 30 % of the components +0 or -0; `dups` triangles more are copies
    with the sign of every zero flipped: equal centres, so a copy shares a leaf with its original and the
    leaf's fold has to choose between +0 and -0."""
    rng = np.random.default_rng(seed)
    v = rng.uniform(0, 3, size=(n, 3, 3)).astype(np.float32)
    v[:, :, 1] = -v[:, :, 1]
    zero = rng.random(v.shape) < 0.3
    v[zero] = np.where(rng.random(int(zero.sum())) < 0.5, np.float32(0.0), np.float32(-0.0))
    if dups:
        src = rng.choice(n, dups, replace=False)
        copy = v[src].copy()
        copy[copy == 0.0] = -copy[copy == 0.0]
        v = np.concatenate([v, copy])[rng.permutation(n + dups)]
    return np.ascontiguousarray(v)


# name -> (builder of the vertices, what it aims at)
ARRAY_CASES = {
    "adv130": (lambda: adversarial(130, 130), "k_bvh_big just above the 128 threshold: per = 1, 126 empty runs"),
    "adv255": (lambda: adversarial(255, 255), "per = 1 with one empty run"),
    "adv256": (lambda: adversarial(256, 256), "per = 1, every thread one prim"),
    "adv257": (lambda: adversarial(257, 257), "per = 2: 129 threads with runs, the last of one prim"),
    "adv1023": (lambda: adversarial(1023, 1023), "per = 4 with a short last run"),
    "adv1025": (lambda: adversarial(1025, 1025), "per = 5: 205 threads with runs, 51 without"),
    "adv4097": (lambda: adversarial(4097, 4097), "per = 17; several levels of big ranges"),
    "zeros_first": (_zeros_first, "all-zero boxes over the whole runs of the leading threads (ufold_cat's !a.nz) "
                                  "and in the middle of the range (its lead0 union)"),
    "collinear40": (lambda: _collinear(40, 26), "a zero-area range box in k_bvh_small: every cost is 0/0, "
                                                "min_cost stays FLT_MAX"),
    "collinear300": (lambda: _collinear(300, 27), "the same in k_bvh_big"),
    "lattice": (_lattice, "many equal centres; offsets exactly on bucket boundaries and on 1.0 (7 -> 6)"),
    "lopsided": (_lopsided, "one far cluster: partitions that swap almost nothing, splits of 1400 : 100"),
    "descending": (_descending, "descending along the split axis: partitions that swap the most pairs"),
    "signed_zero": (lambda: _signed_zero(700, 28, 0), "+0 / -0 ties in the min/max folds (CPU only)"),
    "signed_zero_dups": (lambda: _signed_zero(700, 29, 60), "+0 / -0 ties inside one leaf (CPU only)"),
}
SIGNED_ZERO = ("signed_zero", "signed_zero_dups")    # -0 cannot reach a builder through the scene API
FILE_CASES = {
    "room.json": "several OBJ meshes under transforms",
    "lantern_mesh": "path_ref.lantern's mesh scene: two OBJ meshes under rotated, non-uniform scales",
}


def vertices(name):
    return ARRAY_CASES[name][0]()


def scene_file(name, tmp):
    """The path of a scene-file case (lantern_mesh is written under tmp)."""
    if name == "room.json":
        return str(SCENES / "room.json")
    assert name == "lantern_mesh"
    import path_ref
    return path_ref.lantern(tmp, k=2, mesh=True)[0]


def api_scene(verts, device=False):
    """The triangles through pt_scene_add_mesh under the identity transform (as test_bvh_device_gpu.py's
    _api_mesh_scene), the BVH built on the host or on the device."""
    import ctypes as C

    from cuda_pathtracer_amd import Scene
    from cuda_pathtracer_amd import _native as N
    sc = Scene()
    m = sc.add_material(rgb=(0.9, 0.9, 0.9))
    n = len(verts)
    pos = np.ascontiguousarray(verts.reshape(-1), np.float32)
    fs = np.full(n, 3, np.int32)
    ip = np.arange(3 * n, dtype=np.int32)
    gid = C.c_int32()
    f3 = lambda v: (C.c_float * 3)(*v)  # noqa: E731
    assert N.lib().pt_scene_add_mesh(sc.handle, m, f3([0, 0, 0]), f3([0, 0, 0]), f3([1, 1, 1]),
                                     pos.ctypes.data_as(N._FP), 3 * n, None, 0, None, 0,
                                     fs.ctypes.data_as(N._IP), n, ip.ctypes.data_as(N._IP), None, None,
                                     C.byref(gid)) == 0
    sc.set_camera((16, 16), 45.0, (0, 0, 10), (0, 0, 0))
    sc.set_bvh_builder(device)
    sc.finalize()
    return sc


TRI_DTYPE = np.dtype([("id", "<i4"), ("v", "<f4", (3, 3)), ("uv", "<f4", (3, 2)), ("n", "<f4", (3, 3)),
                      ("bmin", "<f4", (3,)), ("bmax", "<f4", (3,))])   # pt_triangle (include/pt_amd.h)


def tables(scene, node_dtype):
    """A finalized scene's triangle table (leaf order) and flattened node table, as numpy records."""
    import ctypes as C

    from cuda_pathtracer_amd import _native as N
    _, _, nt, nn, _ = scene.counts()
    tris = (N.Triangle * max(nt, 1))()
    nodes = (N.BvhNode * max(nn, 1))()
    assert C.sizeof(N.Triangle) == TRI_DTYPE.itemsize and C.sizeof(N.BvhNode) == node_dtype.itemsize
    assert N.lib().pt_scene_get_triangles(scene.handle, tris, nt) == nt
    assert N.lib().pt_scene_get_bvh(scene.handle, nodes, nn) == nn
    return np.frombuffer(bytes(tris), TRI_DTYPE)[:nt].copy(), np.frombuffer(bytes(nodes), node_dtype)[:nn].copy()


def load_order(tris):
    """The load-order vertices of a leaf-order triangle table (ids are load indices)."""
    assert sorted(tris["id"].tolist()) == list(range(len(tris)))
    return np.ascontiguousarray(tris["v"][np.argsort(tris["id"], kind="stable")])


def level_counts(nodes, above=128):
    """Ranges of more than `above` triangles per tree level of a flattened table: the ranges k_bvh_big
    handles on that level.  Plain numpy over the preorder table, one step per level: the leaves tile
    [0, n) in preorder, so a node's range starts at the triangles counted before it and ends where its
    parent's right child starts (left child) or where the parent ends (right child)."""
    sub = nodes["sub_areas"].astype(np.int64)
    right = nodes["rchild_idx"].astype(np.int64)
    start = np.cumsum(sub) - sub
    end = np.zeros(len(nodes), np.int64)
    end[0] = sub.sum()
    cur, counts = np.zeros(1, np.int64), []
    while len(cur):
        counts.append(int(((end[cur] - start[cur]) > above).sum()))
        inner = cur[sub[cur] == 0]
        lc, rc = inner + 1, right[inner]
        end[lc], end[rc] = start[rc], end[inner]
        cur = np.concatenate([lc, rc])
    return np.asarray(counts)
