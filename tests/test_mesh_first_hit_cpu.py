"""The float64 first-hit reference of tests/mesh_ref.py judged on its own (no GPU): that its scenes show
what they are for, that it excludes few pixels, that float32's own error stays at the constants
test_mesh_first_hit_gpu.py allows 8x of, and — on the reference alone, never by breaking the kernels —
that a wrong interpolation of the smooth normals or texture coordinates, or a mesh seen through the
wrong side, would exceed those tolerances a hundredfold."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

import cuda_pathtracer_amd as P
from cuda_pathtracer_amd import _native as N

sys.path.insert(0, str(Path(__file__).resolve().parent))
import mesh_ref as M  # noqa: E402
from test_mesh_first_hit_gpu import D, PATHS  # noqa: E402


@pytest.fixture(scope="module")
def evaluated(tmp_path_factory):
    """(scene name, mesh path, dtype) -> the reference's result; scene name -> (scene, triangle table).
    Each is computed once and left unchanged."""
    tmp = tmp_path_factory.mktemp("mesh_first_hit_cpu")
    scenes, cache = {}, {}

    def scene(name):
        if name not in scenes:
            sc = P.Scene(M.mesh_scene(tmp, name))
            scenes[name] = (sc, M.triangle_table(sc))
        return scenes[name]

    def get(name, path, dt=np.float64):
        if (name, path, dt) not in cache:
            sc, tris = scene(name)
            mode, bbox = PATHS.get(path, (path, False))
            cache[name, path, dt] = M.mesh_first_hit_ref(tris, sc.geoms(), sc.camera(), dt, mode, use_bbox=bbox)
        return cache[name, path, dt]
    get.scene = scene
    return get


def test_scene_triangles_accessor_is_the_native_table(evaluated):
    sc, tris = evaluated.scene("smooth")
    nt = sc.counts()[2]
    raw = (N.Triangle * nt)()
    assert N.lib().pt_scene_get_triangles(sc.handle, raw, nt) == nt
    assert tris.tobytes() == bytes(raw)[:nt * C.sizeof(N.Triangle)]
    assert sorted(tris["id"].tolist()) == list(range(nt)) and nt <= 3000     # a permutation: BVH leaf order
    assert (tris["id"] != np.arange(nt)).any()
    meshes = [g for g in sc.geoms() if g.type == P.MESH]
    assert len(meshes) >= 4 and len({g.material_id for g in sc.geoms()}) == len(sc.geoms())
    assert [(g.tri_start, g.tri_end) for g in meshes] == [(0, 720), (720, 1296), (1296, 2016), (2016, 2592)]
    assert P.Scene().triangles() == []


def test_loaded_triangles_are_the_transformed_obj(tmp_path, evaluated):
    """scene.cpp:126-143 on curved meshes under rotated, non-uniform and mirrored scales: a world vertex is
    transform * (v, 1), a normal invTranspose * (n, 0) and NOT renormalised, the texture coordinate as read
    — against a float64 product of the geom's own float32 matrices with the corners the OBJ writer wrote.
    Bounds: the file's decimal rounds to float32 once and the four products and three sums of a row once
    each, 8 roundings of at most half an ulp — of a coordinate below 16 (2^-21 each: 3.9e-6 in all), of a
    normal component below 2 (2^-24 each: 4.8e-7); a texture coordinate in [0, 1] rounds once (2^-25)."""
    sc, tris = evaluated.scene("smooth")
    corners = {"uvsphere.obj": M.uv_sphere_obj(tmp_path / "s.obj"), "torus.obj": M.torus_obj(tmp_path / "t.obj")}
    by_id = tris[np.argsort(tris["id"])]
    for g, (typ, obj, _, _, _) in zip(sc.geoms(), M.SMOOTH_OBJECTS):
        if typ != "mesh":
            continue
        pos, nrm, uv = corners[obj]
        got = by_id[g.tri_start:g.tri_end]
        assert len(got) == len(pos)
        want_v = M.R._mv(g.transform, pos, 1, np.float64)
        want_n = M.R._mv(g.inv_transpose, nrm, 0, np.float64)
        assert np.abs(want_v).max() < 16 and np.abs(want_n).max() < 2
        assert np.abs(got["v"] - want_v).max() <= 8 * 2.0 ** -21
        assert np.abs(got["n"] - want_n).max() <= 8 * 2.0 ** -24
        assert np.abs(got["uv"] - uv).max() <= 2.0 ** -25
        assert np.abs(np.linalg.norm(want_n, axis=-1) - 1).max() > 0.1       # (a renormalised normal would differ)


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", M.MESH_SCENES)
def test_excluded_share_is_at_most_5_percent(evaluated, name, path):
    ref = evaluated(name, path)
    excluded = 1.0 - ref["keep"].mean()
    print(f"{name} {path}: excluded {100 * excluded:.2f} %")
    assert excluded <= 0.05


@pytest.mark.parametrize("name", M.MESH_SCENES)
def test_scenes_show_meshes(evaluated, name):
    ref = evaluated(name, "bvh")
    mesh = ref["keep"] & (ref["tri"] >= 0)
    assert mesh.mean() >= 1 / 3
    assert len(np.unique(ref["tri"][mesh])) >= 25
    assert evaluated.scene(name)[0].counts()[2] <= 3000
    if name == "smooth":                                        # open, and every geom in view
        assert (ref["mat"][ref["keep"]] < 0).mean() > 0.1
        assert set(np.unique(ref["geom"][ref["keep"]]).tolist()) == set(range(-1, len(M.SMOOTH_OBJECTS)))
    else:                                                       # a closed room
        assert (ref["mat"] >= 0).all()
    # without the box cull both mesh paths meet the same triangle at the same distance
    lin = evaluated(name, "linear")
    both = ref["keep"] & lin["keep"]
    assert np.array_equal(ref["tri"][both], lin["tri"][both]) and np.array_equal(ref["t"][both], lin["t"][both])


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", M.MESH_SCENES)
def test_float32_own_error_stays_at_the_recorded_constants(evaluated, name, path):
    """deviations() also asserts that float32 picks the float64 geom and triangle on every kept pixel."""
    dev = M.deviations(evaluated(name, path), evaluated(name, path, np.float32))
    for kind in ("tri", "prim"):
        print(f"{name} {path} {kind}: D_t={dev[kind][0]:.3e} D_p={dev[kind][1]:.3e} D_n={dev[kind][2]:.3e} "
              f"D_uv={dev[kind][3]:.3e}")
        for what, got, d in zip(("t", "P", "n", "uv"), dev[kind], D[name, path][kind]):
            assert got <= d, (name, path, kind, what, got, d)


# ---- teeth ------------------------------------------------------------------------------------------------
def test_smooth_scene_has_smooth_normals(evaluated):
    _, tris = evaluated.scene("smooth")
    n = tris["n"].astype(np.float64)
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    spread = np.max([np.abs(n[:, i] - n[:, j]).max(-1) for i, j in ((0, 1), (0, 2), (1, 2))], axis=0)
    assert (spread > 0.05).mean() > 0.9
    # the bundled meshes, for contrast: flat
    _, room = evaluated.scene("room_chair")
    m = room["n"].astype(np.float64)
    m /= np.linalg.norm(m, axis=-1, keepdims=True)
    assert np.max([np.abs(m[:, i] - m[:, j]).max() for i, j in ((0, 1), (0, 2), (1, 2))]) < 1e-5
    # and the normals arrive unnormalised, through the inverse transpose of a non-uniform scale
    length = np.linalg.norm(tris["n"].astype(np.float64), axis=-1)
    assert length.min() < 0.7 and length.max() > 0.8


def test_the_three_interpolations_differ_by_100x_the_gpu_tolerance(evaluated):
    """Triangle::intersect's weights, meshIntersectionTest's and the textbook's give normals that differ,
    pairwise, by more than 100x what the GPU test allows on more than half of the kept mesh pixels; so do
    the two paths' texture coordinates."""
    res = {m: evaluated("smooth", m) for m in ("bvh", "linear", "textbook")}
    k = (res["bvh"]["tri"] >= 0) & res["bvh"]["keep"] & res["linear"]["keep"]
    assert k.sum() > 500
    tol_n = 8 * max(D["smooth", "bvh"]["tri"][2], D["smooth", "linear"]["tri"][2])
    tol_uv = 8 * max(D["smooth", "bvh"]["tri"][3], D["smooth", "linear"]["tri"][3])
    for a, b in (("bvh", "linear"), ("bvh", "textbook"), ("linear", "textbook")):
        assert np.array_equal(res[a]["tri"][k], res[b]["tri"][k])
        dn = np.abs(res[a]["n"][k] - res[b]["n"][k]).max(-1)
        share = (dn > 100 * tol_n).mean()
        print(f"normals {a} vs {b}: {100 * share:.1f} % of {int(k.sum())} pixels differ by > {100 * tol_n:.2e}")
        assert share > 0.5
    du = np.abs(res["bvh"]["uv"][k] - res["linear"]["uv"][k]).max(-1)
    share = (du > 100 * tol_uv).mean()
    print(f"uv bvh vs linear: {100 * share:.1f} % differ by > {100 * tol_uv:.2e}")
    assert share > 0.5


def test_mirrored_mesh_is_seen_from_inside_only(evaluated):
    """The geom scaled by -1 in x has its winding reversed: the culling test (a < FLT_EPSILON is a miss)
    lets the ray through its near side, so every pixel that shows it has crossed exactly one of its
    triangles from behind; the other meshes are met on their near side."""
    sc, _ = evaluated.scene("smooth")
    assert sc.geoms()[M.SMOOTH_REVERSED].scale[0] < 0
    for path in ("bvh", "linear"):
        ref = evaluated("smooth", path)
        k = ref["keep"] & (ref["tri"] >= 0)
        owner = M.geom_of_triangle(ref["tri"], sc.geoms())         # (by id: linear lends other geoms' materials)
        rev = k & (owner == M.SMOOTH_REVERSED)
        assert rev.sum() > 100
        assert (ref["back"][rev] == 1).all()
        assert (ref["back"][k & ~rev] == 0).all()
        rays = M.R.camera_rays(sc.camera(), np.float64)
        facing = (ref["n"] * rays).sum(-1)
        assert (facing[rev] > 0).mean() > 0.95 and (facing[k & ~rev] < 0).mean() > 0.95


def test_linear_path_follows_array_positions(evaluated):
    """meshIntersectionTest's loop runs over positions of the reordered array: on the smooth scene many
    kept pixels get the material of another mesh than the one the triangle was loaded for, and the box
    cull hides triangles that lie in the range of a geom whose box the ray misses."""
    sc, _ = evaluated.scene("smooth")
    bvh, lin, box = (evaluated("smooth", p) for p in ("bvh", "linear", "linear_bbox"))
    k = bvh["keep"] & lin["keep"] & (bvh["tri"] >= 0)
    assert (bvh["geom"][k] == M.geom_of_triangle(bvh["tri"], sc.geoms())[k]).all()
    assert (lin["geom"][k] != bvh["geom"][k]).mean() > 0.25
    kb = k & box["keep"]
    assert ((box["tri"][kb] != bvh["tri"][kb]).mean() > 0.25)
    seen = kb & (box["tri"] >= 0)
    assert seen.any() and (box["t"][seen] >= lin["t"][seen]).all()      # (the cull only ever hides)
