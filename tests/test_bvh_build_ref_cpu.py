"""The BVH build pinned against a restatement that shares none of its code.

tests/bvh_build_ref.py states BVH_tree.cpp:27-181, boundingbox.h and sceneStructs.h:128-143 in numpy
float32; here the oracle's builder (oracle/mesh_oracle.cpp) and the host Builder (pt_mesh.cpp) must give
its flattened nodes and its triangle order byte for byte on every case of tests/bvh_build_cases.py, on a
20,000-triangle mesh and on config 5's 100k scene.  Every comparison is == on bytes; no tolerance exists.

A restatement that cannot tell a wrong builder from a right one pins nothing, so every deliberate error
it knows (bvh_build_ref.VARIANTS) must change the bytes on some case; the test prints which.  Measured:

    cost_includes_i   12 of 14: all but collinear40 and collinear300 (every cost there is NaN)
    no_zero_rule      12 of 14: all but collinear40 and collinear300
    stable_partition  13 of 14: all but signed_zero
    no_swap2          13 of 14: all but collinear40
    rint_bucket       14 of 14
    inner_from_fold    4 of 14: adv1025, zeros_first, signed_zero, signed_zero_dups
    tie_keeps_new      2 of 14: signed_zero, signed_zero_dups (the only cases that hold -0)

The signed-zero cases reach the oracle's builder directly.  The scene API cannot carry -0 (the last test
asserts it), so the host Builder is compared with the restatement of what the scene holds for them.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

import bvh_build_cases as K
import bvh_build_ref as R
from oracle import binding as O

SENSITIVITY_CASES = [c for c in K.ARRAY_CASES if c != "adv4097"]   # (adv4097 adds a second per variant)


@functools.lru_cache(maxsize=None)
def _ref(name):
    return R.build(K.vertices(name))


def _oracle_build(v):
    """oracle_build_bvh on load-order vertices: the node table and the leaf order as load indices."""
    bb, _ = R.triangle_boxes(v)
    t = np.zeros(len(v), O.TRI_DTYPE)
    t["id"], t["v"], t["bmin"], t["bmax"] = np.arange(len(v)), v, bb[:, 0], bb[:, 1]
    nodes = np.zeros(2 * len(v), O.NODE_DTYPE)
    k = O.lib().oracle_build_bvh(t.ctypes.data, len(v), nodes.ctypes.data, len(nodes))
    assert 0 < k <= len(nodes)
    return nodes[:k].copy(), t["id"].astype(np.int64)


def _assert_same(what, nodes, order, ref_nodes, ref_order):
    assert nodes.tobytes() == ref_nodes.tobytes(), f"{what}: {R.first_difference(nodes, ref_nodes)}"
    assert np.array_equal(order, ref_order), \
        f"{what}: triangle order differs first at position {int(np.flatnonzero(order != ref_order)[0])}"


def _assert_host_table(what, tris, nodes, v_load, ref_nodes, ref_order):
    """The host scene's tables against the restatement of its own load-order vertices."""
    _assert_same(what, nodes, tris["id"].astype(np.int64), ref_nodes, ref_order)
    assert tris["v"].tobytes() == v_load[ref_order].tobytes(), f"{what}: reordered vertices differ"
    bb, _ = R.triangle_boxes(tris["v"])      # sceneStructs.h:128-143 from v alone
    assert tris["bmin"].tobytes() == bb[:, 0].tobytes() and tris["bmax"].tobytes() == bb[:, 1].tobytes(), \
        f"{what}: a triangle's stored box is not glm::min/max of its vertices"


@pytest.mark.parametrize("name", list(K.ARRAY_CASES))
def test_array_case_three_ways(name):
    v = K.vertices(name)
    ref_nodes, ref_order = _ref(name)
    _assert_same(f"{name}: oracle", *_oracle_build(v), ref_nodes, ref_order)
    tris, nodes = K.tables(K.api_scene(v), R.NODE_DTYPE)
    v_host = K.load_order(tris)
    if name in K.SIGNED_ZERO:                # the scene holds +0 where v holds -0: restate what it holds
        assert np.array_equal(v_host, v) and v_host.tobytes() != v.tobytes()
        ref_nodes, ref_order = R.build(v_host)
    else:
        assert v_host.tobytes() == v.tobytes()
    _assert_host_table(f"{name}: host Builder", tris, nodes, v_host, ref_nodes, ref_order)


@pytest.mark.parametrize("name", list(K.FILE_CASES))
def test_scene_file_three_ways(name, tmp_path):
    import cuda_pathtracer_amd as P
    path = K.scene_file(name, tmp_path)
    tris, nodes = K.tables(P.Scene(path), R.NODE_DTYPE)
    v = K.load_order(tris)
    ref_nodes, ref_order = R.build(v)
    _assert_host_table(f"{name}: host Builder", tris, nodes, v, ref_nodes, ref_order)
    o = O.OracleScene.from_json(path)
    assert o.tris_load["v"].tobytes() == v.tobytes(), f"{name}: the oracle loads other world vertices"
    _assert_same(f"{name}: oracle", o.nodes, o.tris["id"].astype(np.int64), ref_nodes, ref_order)
    print(f"{name}: {len(v)} triangles, {len(nodes)} nodes")


def _random_mesh_three_ways(v, what):
    ref_nodes, ref_order = R.build(v)
    _assert_same(f"{what}: oracle", *_oracle_build(v), ref_nodes, ref_order)
    tris, nodes = K.tables(K.api_scene(v), R.NODE_DTYPE)
    assert K.load_order(tris).tobytes() == v.tobytes()
    _assert_host_table(f"{what}: host Builder", tris, nodes, v, ref_nodes, ref_order)


def test_random_20k_three_ways():
    _random_mesh_three_ways(np.random.default_rng(31).uniform(-3, 3, size=(20_000, 3, 3)).astype(np.float32),
                            "random 20k")


@pytest.mark.slow
def test_100k_scene_three_ways(tmp_path):
    """Config 5's scene (scenes.random_triangles): the tables of the loaded file."""
    import cuda_pathtracer_amd as P
    from cuda_pathtracer_amd import scenes
    path = scenes.random_triangles(tmp_path, n=100_000)
    tris, nodes = K.tables(P.Scene(path), R.NODE_DTYPE)
    v = K.load_order(tris)
    assert len(v) == 100_000
    ref_nodes, ref_order = R.build(v)
    _assert_host_table("100k: host Builder", tris, nodes, v, ref_nodes, ref_order)
    o = O.OracleScene.from_json(path)
    _assert_same("100k: oracle", o.nodes, o.tris["id"].astype(np.int64), ref_nodes, ref_order)


def test_every_variant_is_seen():
    """Each deliberate error of the restatement changes the nodes or the order of at least one case, so
    a builder that made it would fail test_array_case_three_ways."""
    seen = {}
    for variant in R.VARIANTS:
        seen[variant] = []
        for name in SENSITIVITY_CASES:
            nodes, order = R.build(K.vertices(name), variant)
            ref_nodes, ref_order = _ref(name)
            if nodes.tobytes() != ref_nodes.tobytes() or not np.array_equal(order, ref_order):
                seen[variant].append(name)
        print(f"{variant:17s} seen by {len(seen[variant]):2d} of {len(SENSITIVITY_CASES)}: "
              f"{' '.join(seen[variant])}")
    assert all(seen.values()), f"unseen: {[k for k, s in seen.items() if not s]}"
    # the tie rule shows only where +0 meets -0, which is why the signed-zero cases exist
    assert set(seen["tie_keeps_new"]) <= set(K.SIGNED_ZERO)


def _ancestor_misses(nodes, order, v):
    """Per leaf-order triangle: some ancestor's box does not contain its box (exact comparisons)."""
    bb, _ = R.triangle_boxes(v[order])
    sub = nodes["sub_areas"].astype(np.int64)
    start = np.cumsum(sub) - sub
    end = np.zeros(len(nodes), np.int64)
    end[0] = len(v)
    outside = np.zeros(len(v), bool)
    for i in range(len(nodes)):              # preorder: a parent sets its children's ends first
        if sub[i] == 0:
            r = nodes["rchild_idx"][i]
            end[i + 1], end[r] = start[r], end[i]
        s, e = start[i], end[i]
        outside[s:e] |= ((bb[s:e, 0] < nodes["bmin"][i]) | (bb[s:e, 1] > nodes["bmax"][i])).any(axis=1)
    return outside


@pytest.mark.parametrize("name", list(K.ARRAY_CASES))
def test_structure(name):
    v = K.vertices(name)
    nodes, order = _ref(name)
    n = len(v)
    assert sorted(order.tolist()) == list(range(n)), "every triangle appears once"
    leaves = nodes[nodes["sub_areas"] > 0]
    sub = leaves["sub_areas"].astype(np.int64)
    assert np.array_equal(leaves["first_area_idx"], np.cumsum(sub) - sub) and sub.sum() == n, \
        "the leaf ranges tile [0, n) in preorder"
    inner = np.flatnonzero(nodes["sub_areas"] == 0)
    assert (nodes["rchild_idx"][inner] > inner + 1).all() and (nodes["axis"][inner] >= 0).all()
    outside = _ancestor_misses(nodes, order, v)
    bb, _ = R.triangle_boxes(v[order])
    zero = (bb == 0.0).all(axis=(1, 2))
    print(f"{name}: {n} triangles, {len(nodes)} nodes, {int(zero.sum())} all-zero boxes, "
          f"{int(outside.sum())} triangles that some ancestor does not enclose")
    # `||` can drop only an all-zero box: every other triangle lies inside every ancestor, and without
    # all-zero boxes that is every triangle.  The count on the other cases is the rule's reach, a property
    # of the reference (DESIGN.md section 6 records it: adv1025 130 of 130, zeros_first 70 of 70, else 0).
    assert not outside[~zero].any()


def test_folds_and_partition_equal_their_literal_forms():
    """The restatement works on whole runs; here its run forms equal the element-by-element text: `||`
    folded one box at a time with glm's min and max, and libstdc++'s __partition statement by statement."""
    rng = np.random.default_rng(41)
    values = np.array([0.0, -0.0, 1.0, -1.0, 2.0], np.float32)

    def union(acc, b):                       # boundingbox.h:46-63
        if (acc == 0.0).all():
            return b
        return np.stack([R.glm_min(b[0], acc[0]), R.glm_max(b[1], acc[1])])

    for _ in range(300):
        k = int(rng.integers(1, 9))
        lo = rng.choice(values, size=(k, 3))
        hi = R.glm_max(lo, rng.choice(values, size=(k, 3)))
        seq = np.stack([lo, hi], 1)
        acc = seq[0]
        for b in seq[1:]:
            acc = union(acc, b)
        assert R.fold_boxes(seq).tobytes() == np.ascontiguousarray(acc).tobytes()
        passing = rng.random(int(rng.integers(1, 40))) < rng.random()
        perm, mid = R.partition_literal(passing)
        left, right = R.partition_swaps(passing)
        mine = np.arange(len(passing))
        mine[left], mine[right] = right, left
        assert mine.tolist() == perm and mid == int(passing.sum())


def test_no_negative_zero_reaches_the_world_table():
    """-0 in vertices, translation and rotation, under mirrored scales: the world table holds none.  A
    world coordinate is (T0 x + T4 y) + (T8 z + T12); the translation column is a sum with +0 terms, and
    in round-to-nearest a sum with a +0 term is never -0.  This is what makes the +0 zero box that
    bvh_build.hip's ufold_box writes for a run of all-zero boxes unobservable; were it to fail, the
    signed-zero cases would belong in the GPU test."""
    import cuda_pathtracer_amd as P
    from cuda_pathtracer_amd import _native as N
    grid = np.array([-0.0, 0.0, 1.0, -1.0, 0.5, -2.0], np.float32)
    pos = np.stack(np.meshgrid(grid, grid, grid, indexing="ij"), -1).reshape(-1, 3)
    assert np.signbit(pos[pos == 0.0]).any()
    n = len(pos) // 3
    fs = np.full(n, 3, np.int32)
    ip = np.arange(3 * n, dtype=np.int32)
    f3 = lambda v: (C.c_float * 3)(*v)  # noqa: E731
    nz = -0.0
    transforms = [([nz, nz, nz], [nz, nz, nz], [-1, 1, 1]), ([nz, nz, nz], [nz, nz, nz], [-1, -1, -1]),
                  ([nz, nz, nz], [nz, nz, nz], [1, 1, 1]), ([nz, 1, nz], [nz, 90, nz], [1, -1, 1]),
                  ([nz, nz, -1], [180, nz, 270], [-2, 1, -0.5]), ([0, nz, 0], [nz, 180, 0], [1, 1, -1])]
    sc = P.Scene()
    m = sc.add_material(rgb=(0.9, 0.9, 0.9))
    flat = np.ascontiguousarray(pos.reshape(-1))
    for t, r, s in transforms:
        assert N.lib().pt_scene_add_mesh(sc.handle, m, f3(t), f3(r), f3(s), flat.ctypes.data_as(N._FP), len(pos),
                                         None, 0, None, 0, fs.ctypes.data_as(N._IP), n, ip.ctypes.data_as(N._IP),
                                         None, None, None) == 0
    sc.set_camera((16, 16), 45.0, (0, 0, 10), (0, 0, 0))
    sc.finalize()
    tris, _ = K.tables(sc, R.NODE_DTYPE)
    assert len(tris) == n * len(transforms)
    for field in ("v", "bmin", "bmax"):
        a = tris[field]
        assert (a == 0.0).any() and not np.signbit(a[a == 0.0]).any(), f"-0 in the world table's {field}"
