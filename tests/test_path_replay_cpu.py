"""The float64 path replay of tests/path_ref.py judged on its own and against the oracle (no GPU):

* the reference alone — it excludes few pixels, most kept pixels are lit, and every branch of the shading
  occurs on kept paths;
* the yardstick — the float32 evaluation of the same replay takes the same route and stays at the constants
  test_path_replay_gpu.py allows 8x of;
* the oracle against the replay — oracle.render_pass with the global-pixel key agrees on every kept pixel
  within that tolerance: the kernels equal the oracle bit for bit, so a disagreement here puts the shared
  reading of the reference in question before any GPU is involved;
* sensitivity — one deliberate error in the replay, or singleAlbedo on one side only, disagrees with the
  oracle on at least 1 % of the kept pixels."""
import sys
from pathlib import Path

import numpy as np
import pytest

import cuda_pathtracer_amd as P
from oracle import binding as O

sys.path.insert(0, str(Path(__file__).resolve().parent))
import path_ref as R  # noqa: E402
import rng_ref  # noqa: E402
from test_path_replay_gpu import CASES, D, PATHS, REPLAYS, SCENES, Replays, replay_requests  # noqa: E402

REQUESTS = replay_requests()


def _id(req):
    key, iters, rank, world = req
    return f"{key}-it{iters[0]}..{iters[-1]}x{len(iters)}-r{rank}of{world}"


@pytest.fixture(scope="module")
def replays(tmp_path_factory):
    return Replays(tmp_path_factory.mktemp("path_replay_cpu"))


@pytest.fixture(scope="module")
def oracle_image(replays):
    """(replay, iterations, rank, world, flag overrides) -> the oracle's image with the global-pixel key."""
    scenes, cache = {}, {}

    def get(key, iters, rank=0, world=1, **more):
        req = (key, tuple(iters), rank, world, tuple(sorted(more.items())))
        if req not in cache:
            name, depth, fl, path = REPLAYS[key]
            if name not in scenes:
                scenes[name] = O.OracleScene.from_json(replays.scene(key)[2])
            fl = R.default_flags(**dict(fl, **more))
            ofl = O.flags(russian_roulette=fl["russianRoulette"], use_bvh=path == "bvh", use_bbox=path != "linear",
                          ssaa=fl["ssaa"], dof=fl["dof"], aperture=fl["aperture"], focal_dist=fl["focal_len"],
                          single_albedo=fl["singleAlbedo"], rng_key_pixel=True)
            img = None
            for it in iters:
                img, _ = O.render_pass(scenes[name], ofl, it, rank=rank, world=world, image=img, depth=depth)
            cache[req] = img
        return cache[req]
    return get


# ---- the tables the replay reads ---------------------------------------------------------------------------
def test_vectorised_uniforms_equal_the_scalar_restatement():
    idx = np.array([0, 1, 47, 48, 1727])
    for it, depth in ((1, 8), (7, 2), (5, 1)):
        tab = rng_ref.u01_table(it, idx, depth, 5)
        for i, row in zip(idx.tolist(), tab):
            np.testing.assert_array_equal(row, rng_ref.py_u01(it, i, depth, 5))


@pytest.mark.parametrize("key", ["d8", "k4_d8", "mats_d8", "mesh_bvh"])
def test_scenes_are_what_the_cases_need(replays, key):
    name = REPLAYS[key][0]
    scene, textures, _ = replays.scene(key)
    assert scene.state().traceDepth == REPLAYS[key][1]
    geoms, mats, cam = scene.geoms(), scene.materials(), scene.camera()
    k = SCENES[name]["k"]
    assert len(geoms) == 6 * k * k + len(R.OBJECTS) and (len(geoms) <= 32) == (k == 2)        # kLdsGeoms
    assert (len(mats) > 128) == (name == "lantern2_mats")                                      # kLdsMats
    assert tuple(cam.res) == (48, 36)
    lo = np.array(R.BOX_CENTRE) - R.BOX_SIZE / 2
    pos = np.array(list(cam.position))
    assert (pos > lo + 1).all() and (pos < lo + R.BOX_SIZE - 1).all()                         # inside the box
    face = replays.scene("face_d2_default")[0].camera()
    assert ((np.array(list(face.position)) > lo + 1) & (np.array(list(face.position)) < lo + R.BOX_SIZE - 1)).all()
    assert (np.abs(pos - np.array(R.BOX_CENTRE)) > 0.25).all() and (np.abs(np.array(list(cam.view))) > 0.1).all()
    # the tiles emit, each its own colour; the objects do not, and their materials differ pairwise
    tiles = [mats[g.material_id] for g in geoms[len(R.OBJECTS):]]
    assert {m.emittance for m in tiles} == {1.0, 2.0, 3.0}
    assert len({tuple(m.color) for m in tiles}) == len(tiles)
    objs = [mats[g.material_id] for g in geoms[:len(R.OBJECTS)]]
    for i, a in enumerate(objs):
        assert a.emittance == 0
        for b in objs[:i]:
            assert max(abs(x - y) for x, y in zip(a.color, b.color)) >= 0.02
    m = objs[R.MIRROR_OBJ]
    assert m.has_reflective == 1 and tuple(m.spec_color) != tuple(m.color)
    assert objs[R.HALF_OBJ].has_reflective == 0.5
    assert (objs[R.GLASS_15].ior, objs[R.GLASS_075].ior) == (1.5, 0.75) and objs[R.GLASS_15].has_refractive != 0
    if name == "lantern_mesh":
        assert geoms[R.DIFFUSE_SPHERE].type == P.MESH and geoms[R.EXTRA_CUBE].type == P.MESH
        assert objs[R.EXTRA_CUBE].texture_id == 0 and len(textures) == 1
        px = textures[0].reshape(-1, 3)
        assert len({tuple(t) for t in px.tolist()}) == len(px)                                 # distinct texels
        tris = R.M.triangle_table(scene)
        own = tris[np.argsort(tris["id"])][geoms[R.DIFFUSE_SPHERE].tri_start:geoms[R.DIFFUSE_SPHERE].tri_end]
        n = own["n"].astype(np.float64)
        n /= np.linalg.norm(n, axis=-1, keepdims=True)
        assert (np.abs(n[:, 0] - n[:, 1]).max(-1) > 0.05).mean() > 0.9                         # smooth normals
    else:
        assert scene.counts()[2] == 0 and not textures


def test_face_view_shows_one_material_so_the_material_sort_moves_nothing(replays):
    """What the sorted reference-key case of the GPU test rests on, on the float64 side alone: every camera
    ray of every iteration meets the half-mirror cube first, and none of these hits is uncertain."""
    for req in REQUESTS:
        if req[0] == "face_d2_default":
            ref = replays(*req)
            assert (ref["geom"][:, 0] == R.HALF_OBJ).all() and not ref["hit_risky"][:, 0].any()
            both = [((ref["route"][:, 0] & bit) != 0).sum() for bit in (R.MIRROR, R.DIFFUSE)]
            assert min(both) >= 500, both


# ---- the reference alone -------------------------------------------------------------------------------------
@pytest.mark.parametrize("req", REQUESTS, ids=_id)
def test_few_pixels_are_excluded_and_most_kept_pixels_are_lit(replays, req):
    ref = replays(*req)
    excluded = 1.0 - ref["keep"].mean()
    lit = (ref["image"][ref["keep"]].max(-1) > 0).mean()
    print(f"{_id(req)}: excluded {100 * excluded:.2f} %, lit {100 * lit:.1f} % of the kept pixels")
    assert excluded <= 0.05
    assert lit >= 0.80


def _branch_counts(replays, keys):
    """branch -> the number of kept paths (iteration, pixel) on which it occurs, over the requests of `keys`."""
    total = {}
    for req in REQUESTS:
        if req[0] not in keys:
            continue
        ref = replays(*req)
        geoms = replays.scene(req[0])[0].geoms()
        gtype = np.array([g.type for g in geoms] + [-1])[ref["geom"]]
        rt, gm = ref["route"], ref["geom"]
        on = {
            "diffuse on a cube": ((rt & R.DIFFUSE) != 0) & (gtype == P.CUBE),
            "diffuse on a sphere": ((rt & R.DIFFUSE) != 0) & (gtype == P.SPHERE),
            "mirror": ((rt & R.MIRROR) != 0) & (gm == R.MIRROR_OBJ),
            "half mirror reflects": ((rt & R.MIRROR) != 0) & (gm == R.HALF_OBJ),
            "half mirror scatters": ((rt & R.DIFFUSE) != 0) & (gm == R.HALF_OBJ),
            "refraction": (rt & R.REFRACT) != 0,
            "refraction at ior 0.75": ((rt & R.REFRACT) != 0) & (gm == R.GLASS_075),
            "Fresnel reflection": (rt & R.FRESNEL) != 0,
            "refraction with k < 0": (rt & R.REFRACT_NAN) != 0,
            "roulette kill": (rt & R.RR_KILL) != 0,
            "roulette survival": (rt & R.RR_LIVE) != 0,
            "remaining == 0 exit": (rt & R.EXIT) != 0,
            "miss after a NaN direction": ((rt & R.MISS) != 0) & ((rt & R.NAN_RAY) != 0),
            "textured hit that continues": ((rt & R.TEX) != 0) & ((rt & (R.EXIT | R.RR_KILL)) == 0),
            "smooth-normal hit": (gtype == P.MESH) & (gm == R.DIFFUSE_SPHERE) & ((rt & R.DIFFUSE) != 0),
            "bounce off a surface": ((rt & (R.DIFFUSE | R.MIRROR | R.FRESNEL)) != 0) & ((rt & (R.EXIT | R.RR_KILL)) == 0),
        }
        for name, where in on.items():
            paths = where.any(axis=1) & ref["keep"][None]            # (iterations, rows, W)
            total[name] = total.get(name, 0) + int(paths.sum())
        # a miss happens only after a NaN direction: the box is closed
        assert not (((rt & R.MISS) != 0) & ((rt & R.NAN_RAY) == 0) & ref["keep"][None, None]).any()
    return total


def test_every_branch_occurs_on_kept_paths(replays):
    analytic = {k for k, v in REPLAYS.items() if v[0] not in ("lantern_mesh", "lantern2_face")}
    got = _branch_counts(replays, analytic)
    print(got)
    for name, n in got.items():
        if name not in ("textured hit that continues", "smooth-normal hit"):
            assert n >= 10, (name, n)
    mesh = _branch_counts(replays, {k for k, v in REPLAYS.items() if v[0] == "lantern_mesh"})
    print(mesh)
    for name in ("textured hit that continues", "smooth-normal hit", "diffuse on a cube", "refraction", "mirror"):
        assert mesh[name] >= 10, (name, mesh[name])


# ---- the yardstick ---------------------------------------------------------------------------------------------
def test_no_tolerance_is_below_one_rounding():
    assert set(D) == set(REPLAYS) and min(D.values()) >= 6e-8
    assert {c["replay"] for c in CASES.values()} == set(REPLAYS)
    assert all(REPLAYS[k][3] in PATHS for k in REPLAYS)


@pytest.mark.parametrize("req", REQUESTS, ids=_id)
def test_float32_takes_the_same_route_and_stays_at_the_recorded_constants(replays, req):
    r64, r32 = replays(*req), replays(*req, dt=np.float32)
    assert r32["image"].dtype == np.float32
    keep = r64["keep"]
    assert np.array_equal(r64["route"][:, :, keep], r32["route"][:, :, keep])
    assert np.array_equal(r64["geom"][:, :, keep], r32["geom"][:, :, keep])
    d = R.deviation(r32["image"], r64["image"])[keep].max()
    print(f"{_id(req)}: D_c = {d:.3e}")
    assert d <= D[req[0]], (req, d)


# ---- the oracle against the replay ------------------------------------------------------------------------------
@pytest.mark.parametrize("req", REQUESTS, ids=_id)
def test_oracle_agrees_with_the_replay_on_every_kept_pixel(replays, oracle_image, req):
    ref = replays(*req)
    got = oracle_image(*req)
    dev = R.deviation(got, ref["image"])
    bad = ref["keep"] & ~(dev <= 8 * D[req[0]])
    print(f"{_id(req)}: largest deviation {dev[ref['keep']].max():.3e}, allowed {8 * D[req[0]]:.3e}")
    assert not bad.any(), (req, int(bad.sum()), [(yx, got[tuple(yx)].tolist(), ref["image"][tuple(yx)].tolist(),
                                                  R.describe(ref, tuple(yx))) for yx in np.argwhere(bad)[:4].tolist()])


# ---- sensitivity ---------------------------------------------------------------------------------------------------
def _disagreeing_share(wrong, right, oracle, tol):
    keep = wrong["keep"] & right["keep"]
    return float((R.deviation(oracle, wrong["image"])[keep] > tol).mean())


@pytest.mark.parametrize("variant,key", [("sincos_swap", "d8_jitter"), ("up_linear", "d8_jitter"),
                                         ("xy_order", "d8_jitter"), ("jitter_swap", "d3")])
def test_one_deliberate_error_in_the_replay_disagrees_with_the_oracle(replays, oracle_image, variant, key):
    iters = (1, 7)
    share = _disagreeing_share(replays(key, iters, variant=variant), replays(key, iters), oracle_image(key, iters),
                               8 * D[key])
    print(f"{variant} on {key}: {100 * share:.1f} % of the kept pixels disagree")
    assert share >= 0.01


@pytest.mark.parametrize("variant,key", [("lens_pi", "d3"), ("inv_ior", "d8_jitter"), ("schlick4", "d8_jitter"),
                                         ("rr_gate", "d8")])
def test_rarer_errors_are_seen_too(replays, oracle_image, variant, key):
    """Errors that change few paths — the lens angle pi * u, 1 / ior passed to refract, X^4 in the Schlick
    term, the roulette gate at bounces >= 3: each still moves kept pixels beyond the tolerance (the shares
    are printed; they are small because few paths pass through the decision)."""
    iters = (1, 7)
    share = _disagreeing_share(replays(key, iters, variant=variant), replays(key, iters), oracle_image(key, iters),
                               8 * D[key])
    print(f"{variant} on {key}: {100 * share:.2f} % of the kept pixels disagree")
    assert share > 0


def test_single_albedo_on_one_side_only_disagrees(replays, oracle_image):
    iters = (1, 7)
    share = _disagreeing_share(replays("d8", iters, singleAlbedo=True), replays("d8", iters), oracle_image("d8", iters),
                               8 * D["d8"])
    print(f"singleAlbedo in the replay only: {100 * share:.1f} %")
    assert share >= 0.01
    share = _disagreeing_share(replays("d8", iters), replays("d8", iters), oracle_image("d8", iters, singleAlbedo=True),
                               8 * D["d8"])
    print(f"singleAlbedo in the oracle only: {100 * share:.1f} %")
    assert share >= 0.01
