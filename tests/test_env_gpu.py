"""Environment lighting on the GPU: the lookup, the ENV instantiations of the bounce kernels,
and the public interface.

1. env_eval (the bounce kernels' own lookup function behind a small kernel) equals env_ref.lookup in float32
   bit for bit.
2. A constant map with no geom in view: every accumulator channel is the float32 running sum of scale x colour.
3. An all-zero map renders the bits of the same scene without an environment (open lantern and its mesh variant).
4. Whole paths against env_path_ref.replay_env in float64, on every kept pixel, within 8 x D_c (never below
   2^-24), every case with rngKeyPixel.  D_c is the float32-vs-float64 deviation of the same replay, measured on
   the CPU at 48x36 (env_path_ref.D holds these values, the fourth digit rounded up; test_env_cpu.py asserts that
   the measurement stays at or below them, that both dtypes take the same routes, and the conditions on the scene):

   replay       scene                         depth  flags                    D_c        excluded  env     via specular
   open_d2      open lantern                    2    no jitter, no lens       3.004e-04   0.93 %   70.2 %    7.6 %
   open_d8      open lantern                    8    jitter, lens, roulette   4.020e-04   2.89 %   71.9 %   10.1 %
   open_mats    open lantern, 131 materials     8    open_d8's                6.934e-05   1.39 %   74.1 %   10.2 %
   open_mesh    open lantern, mesh variant      4    open_d8's, BVH           1.342e-04   1.27 %   72.3 %   10.3 %
   glass_d2     open lantern, glass view        2    no jitter, no lens       5.352e-07   0.58 %     -        -

   (open_d8's figures are the extremes over its iteration sets: 1 and 7 - D_c 6.934e-05 -, 5..7 and 3..7 - both
   4.020e-04 -, and the two tiles of world = 2.  glass_d2 is the NaN tooth's view and has no share to meet: 99.5 %
   of its kept pixels carry a k < 0 refraction at the first bounce.)

   (excluded: the largest share over the replay's iteration sets and tiles; env: the smallest share of kept
   pixels with a path that ends in the environment; via specular: the smallest share that reaches it only after
   a mirror or glass bounce.)  D_c is far above one float32 rounding here because a direction that has been
   through a curved mirror or a lens carries float32's error magnified, and the N = 8 map turns a direction
   error into a colour error at up to ~10 per radian: it is the format's error on THIS scene, as the rule asks.
5. Teeth: the map transposed, the rotation dropped, or a NaN ray shaded with L instead of 0, each applied on the
   replay side, moves at least 20 % of the kept pixels beyond the tolerance.  The first two on the open lantern;
   the NaN ray on its glass view, where nearly every camera path becomes one (on the open lantern's own view that
   error moves 9.7 % of the kept pixels, measured on the CPU: test_env_cpu.py prints it, nothing asserts it).
6. One batched pass of 6 iterations equals six one-iteration passes bit for bit; render-ahead claims too.
7. Refusals (PT_ERR_ARG before any launch), a JSON scene with Extensions.ENVIRONMENT against set_environment,
   and clear_environment.
"""
import json
import shutil
import sys
from pathlib import Path

import numpy as np
import pytest

import cuda_pathtracer_amd as P

sys.path.insert(0, str(Path(__file__).resolve().parent))
import env_path_ref as EP  # noqa: E402
import env_ref as E  # noqa: E402
import path_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
from env_path_ref import (CASES, D, GOLDEN_HDR, REPLAYS, TEETH, Replays, case_iterations, the_environment)  # noqa: E402

@pytest.fixture(scope="module")
def replays(tmp_path_factory):
    return Replays(tmp_path_factory.mktemp("env_replay"))


def gui_of(key, **more):
    fl = R.default_flags(**REPLAYS[key][3])
    g = P.GuiDataContainer()
    g.SSAA, g.DoF, g.aperture, g.focal_len = fl["ssaa"], fl["dof"], fl["aperture"], fl["focal_len"]
    g.russianRoulette, g.singleAlbedo, g.rngKeyPixel = fl["russianRoulette"], fl["singleAlbedo"], True
    for k, v in more.items():
        assert hasattr(g, k), k
        setattr(g, k, v)
    return g


def tolerance(key):
    return 8 * max(D[key], 2.0 ** -24)


def mismatches(name, got, ref, tol):
    """The kept pixels whose deviation from the replay exceeds tol, as text (empty: none)."""
    dev = R.deviation(got, ref["image"])
    bad = ref["keep"] & ~(dev <= tol)
    print(f"{name}: largest deviation on the kept pixels {dev[ref['keep']].max():.3e}, allowed {tol:.3e}")
    if not bad.any():
        return ""
    lines = [f"{name}: {int(bad.sum())} of {int(ref['keep'].sum())} kept pixels deviate by more than {tol:.3e}"]
    for r, c in np.argwhere(bad)[:5]:
        lines.append(f"  (row {r}, x {c}): got {got[r, c].tolist()} replay {ref['image'][r, c].tolist()} "
                     f"deviation {dev[r, c]:.3e} route {R.describe(ref, (r, c))}")
    return "\n".join(lines)


def render(scene, gui, passes=(1, 7), spp=1, rank=0, world=1, expect=None):
    """The image after the passes.  expect: what the context must report, so that a case is known to have run the
    variant it names: lanes (pt_ctx_stream_info), traverse (the BVH walk was launched as a kernel of its own: kMeshPre;
    False: it was not, the walk is inside the bounce kernel: kMeshInline), materials_over (past the LDS table)."""
    expect = expect or {}
    pt = P.PathTracer(scene, gui, rank=rank, world=world, spp=spp)
    try:
        assert pt.cmask_info()["on"] == (scene.environment() is None and scene.counts()[2] == 0 and scene.counts()[0] <= 32)
        if "lanes" in expect:
            assert pt.stream_info()["lanes"] == expect["lanes"]
        if "materials_over" in expect:
            assert scene.counts()[1] > expect["materials_over"] and scene.counts()[0] <= 32 and scene.counts()[2] == 0
        if "traverse" in expect:
            pt.profile(True)
        for first in passes:
            pt.render_pass(first)
        img = pt.image()
        if "traverse" in expect:
            kinds = pt.profile_read()
            walks = kinds["traverse"][1] + kinds["first_traverse"][1]
            assert kinds["first_bounce"][1] == len(passes) and (walks > 0) == expect["traverse"], kinds
        return img
    finally:
        pt.free()


# ---- 1. the lookup ---------------------------------------------------------------------------------------------
def directions():
    rng = np.random.default_rng(19)
    axes = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    edges = [tuple(s * (k == a) + t * (k == b) for k in range(3)) for a in range(3) for b in range(a + 1, 3)
             for s in (1, -1) for t in (1, -1)]
    diags = [(a, b, c) for a in (1, -1) for b in (1, -1) for c in (1, -1)]
    assert len(edges) == 12 and len(diags) == 8
    zeros = [tuple(np.where(np.array(m), np.array(v), z)) for m in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1))
             for v in ((0.3, -0.7, 0.45), (-0.6, 0.2, -0.9)) for z in (0.0, -0.0)]
    base = np.array(axes + edges + diags + zeros, np.float32)
    lengths = np.concatenate([base * np.float32(s) for s in (1e-30, 1e-12, 1e-3, 7.0, 1e12, 1e30)])
    yzero = np.array([(x, y, z) for x in (0.4, -0.8) for z in (0.5, -0.3) for y in (0.0, -0.0)], np.float32)
    bad = np.array([(0, 0, 0), (-0.0, 0.0, -0.0), (np.nan, 1, 0), (1, np.nan, 0), (0, 1, np.nan), (np.nan,) * 3,
                    (np.inf, 0, 0), (0, -np.inf, 1), (1, 1, np.inf), (-np.inf, np.inf, 0), (3e38, 3e38, 3e38)], np.float32)
    rand = rng.normal(size=(65536, 3)).astype(np.float32)
    return np.concatenate([base, lengths, yzero, bad, rand]), len(base) + len(lengths) + len(yzero), len(bad)


@pytest.mark.parametrize("n", [1, 2, 5, 64])
@pytest.mark.parametrize("rotate,scale", [((0.0, 0.0, 0.0), 1.0), ((25.0, -40.0, 15.0), 0.37)])
def test_env_eval_equals_the_float32_restatement_bit_for_bit(gpu_device, n, rotate, scale):
    rng = np.random.default_rng(n)
    texels = (rng.random((n, n, 3), dtype=np.float32) * np.float32(4.0)).astype(np.float32)
    scene = P.Scene()
    scene.set_environment_octa(texels, scale=scale, rotate=rotate)
    got = scene.environment()
    assert got["n"] == n and np.array_equal(got["map"], E.pad(texels))
    dirs, first_bad, nbad = directions()
    out = P.env_eval(scene, dirs)
    want = E.lookup(got["map"], scale, E.rotation(rotate), dirs, np.float32)
    assert not out[first_bad:first_bad + nbad].any()                         # zero, NaN, infinite and overflowing: 0
    diff = out.view(np.uint32) != want.view(np.uint32)
    assert not diff.any(), (int(diff.any(-1).sum()), dirs[diff.any(-1)][:4].tolist(), out[diff.any(-1)][:4].tolist(),
                            want[diff.any(-1)][:4].tolist())
    if rotate == (0.0, 0.0, 0.0):                                            # +y is the centre of the square
        up = P.env_eval(scene, np.array([[0, 2, 0]], np.float32))[0]
        c = got["map"][1:-1, 1:-1, :3]
        centre = c[n // 2, n // 2] if n % 2 else c[n // 2 - 1:n // 2 + 1, n // 2 - 1:n // 2 + 1].reshape(-1, 3).mean(0)
        np.testing.assert_allclose(up, centre * np.float32(scale), rtol=1e-6)


# ---- 2. a constant map, no geom in view ------------------------------------------------------------------------
@pytest.mark.parametrize("spp,passes", [(1, (1, 2, 3, 4, 5)), (5, (1,))])
def test_constant_map_with_no_geom_in_view_sums_exactly(gpu_device, spp, passes):
    colour, scale = np.array([0.7, 1.9, 0.1], np.float32), 0.37
    scene = P.Scene(str(Path(__file__).resolve().parent / "scenes" / "cornell.json"))
    scene.set_camera((32, 24), 40.0, (0, 5, 30.0), (0, 5, 60.0), (0, 1, 0))     # turned away from the box
    scene.finalize()
    scene.set_environment_octa(np.broadcast_to(colour, (4, 4, 3)), scale=scale, rotate=(10.0, 20.0, 30.0))
    img = render(scene, P.GuiDataContainer(), passes=passes, spp=spp)
    want = np.zeros(3, np.float32)
    for _ in range(5):
        want = want + colour * np.float32(scale)
    assert img.shape == (24, 32, 3) and np.array_equal(img.view(np.uint32), np.broadcast_to(want, img.shape).view(np.uint32))


# ---- 3. zero is nothing ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["open_d8", "open_mesh"])
def test_an_all_zero_map_renders_the_bits_of_no_environment(gpu_device, replays, key):
    scene = replays.scene(key)[0]
    env = the_environment()
    try:
        scene.clear_environment()
        bare = render(scene, gui_of(key))
        scene.set_environment_octa(np.zeros((EP.ENV_N, EP.ENV_N, 3), np.float32), scale=env["scale"], rotate=env["rotate"])
        zero = render(scene, gui_of(key))
    finally:
        scene.set_environment_octa(env["texels"], scale=env["scale"], rotate=env["rotate"])
    assert bare.any() and np.array_equal(bare.view(np.uint32), zero.view(np.uint32))


# ---- 4. whole paths against the float64 replay ----------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_render_agrees_with_the_float64_replay_on_every_kept_pixel(gpu_device, replays, monkeypatch, name):
    case = CASES[name]
    key = case["replay"]
    scene = replays.scene(key)[0]
    for k, v in case.get("env", {}).items():
        monkeypatch.setenv(k, v)
    world, spp = case.get("world", 1), case.get("spp", 1)
    for rank in range(world):
        ref = replays(key, case_iterations(case), rank, world)
        assert 1.0 - ref["keep"].mean() <= 0.10                   # (float64 side alone)
        got = render(scene, gui_of(key, **case.get("gui", {})), case.get("passes", (1, 7)), spp, rank, world,
                     {k: case[k] for k in ("lanes", "traverse", "materials_over") if k in case})
        text = mismatches(f"{name} rank {rank}/{world}", got, ref, tolerance(key))
        assert not text, text


# ---- 5. teeth ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(TEETH))
def test_one_deliberate_error_in_the_replay_moves_a_fifth_of_the_kept_pixels(gpu_device, replays, variant):
    key = TEETH[variant]
    right, wrong = replays(key, (1, 7)), replays(key, (1, 7), variant=variant)
    got = render(replays.scene(key)[0], gui_of(key))
    assert not mismatches(f"{key} (as it is)", got, right, tolerance(key))
    keep = right["keep"] & wrong["keep"]
    share = float((R.deviation(got, wrong["image"])[keep] > tolerance(key)).mean())
    print(f"{variant} on {key}: {100 * share:.1f} % of the kept pixels move beyond the tolerance")
    assert share >= 0.20


# ---- 6. batched equals sequential ------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["open_d8", "open_mesh"])
def test_one_pass_of_six_iterations_equals_six_passes(gpu_device, replays, key):
    scene = replays.scene(key)[0]
    seq = render(scene, gui_of(key), passes=(2, 3, 4, 5, 6, 7))
    bat = render(scene, gui_of(key), passes=(2,), spp=6)
    assert seq.any() and np.array_equal(seq.view(np.uint32), bat.view(np.uint32))


def test_render_ahead_claims_give_the_same_bits(gpu_device, replays):
    scene = replays.scene("open_d8")[0]
    seq = render(scene, gui_of("open_d8"), passes=(1, 2, 3))
    pt = P.PathTracer(scene, gui_of("open_d8"))
    try:
        pt.render_pass(1)
        for it in (2, 3):
            pt.render_ahead(it)
            pt.render_pass(it)
        ahead = pt.image()
    finally:
        pt.free()
    assert np.array_equal(seq.view(np.uint32), ahead.view(np.uint32))


# ---- 7. refusals and end to end ----------------------------------------------------------------------------------
def test_unsupported_combinations_are_refused_with_a_message(gpu_device, replays, monkeypatch):
    scene = replays.scene("open_d2")[0]
    with pytest.raises(P.PtError, match="environment.*sort_by_material") as e:
        P.PathTracer(scene, gui_of("open_d2", sortbyMaterial=True))
    assert e.value.code == 1                                       # PT_ERR_ARG
    pt = P.PathTracer(scene, gui_of("open_d2"))
    try:
        with pytest.raises(P.PtError, match="environment.*sort_by_material") as e:
            pt.set_flags(gui_of("open_d2", sortbyMaterial=True))
        assert e.value.code == 1
        with pytest.raises(P.PtError, match="adaptive sampling with an environment") as e:
            pt.adaptive(True)
        assert e.value.code == 1
        assert pt.stats()["passes"] == 0                           # nothing was launched
    finally:
        pt.free()
    monkeypatch.setenv("PT_PIPELINE", "split")
    with pytest.raises(P.PtError, match="environment.*PT_PIPELINE=split") as e:
        P.PathTracer(scene, gui_of("open_d2"))
    assert e.value.code == 1
    monkeypatch.delenv("PT_PIPELINE")
    bare = P.Scene()
    with pytest.raises(P.PtError, match="no environment"):
        P.env_eval(bare, np.zeros((1, 3), np.float32))


def test_a_scene_file_with_an_environment_equals_set_environment(gpu_device, replays, tmp_path):
    assert GOLDEN_HDR.stat().st_size < 10 * 1024
    src = Path(replays.scene("open_d2")[2])
    spec = json.loads(src.read_text())
    params = dict(scale=0.8, rotate=(0.0, 70.0, 5.0), size=6)
    d = tmp_path / "with_env"
    (d / "Textures").mkdir(parents=True)
    shutil.copy(GOLDEN_HDR, d / "Textures" / "sky.hdr")
    (d / "plain.json").write_text(json.dumps(spec))
    spec["Extensions"]["ENVIRONMENT"] = {"FILE": "sky.hdr", "SCALE": params["scale"], "ROTATE": list(params["rotate"]),
                                         "SIZE": params["size"]}
    (d / "env.json").write_text(json.dumps(spec))
    from_file, by_hand = P.Scene(str(d / "env.json")), P.Scene(str(d / "plain.json"))
    assert by_hand.environment() is None
    bare = render(by_hand, gui_of("open_d2"))
    by_hand.set_environment(P.decode_hdr(GOLDEN_HDR.read_bytes()), **params)
    a, b = from_file.environment(), by_hand.environment()
    assert a["n"] == 6 and a["scale"] == b["scale"] and a["rotate"] == b["rotate"] and np.array_equal(a["map"], b["map"])
    one, two = render(from_file, gui_of("open_d2")), render(by_hand, gui_of("open_d2"))
    assert np.array_equal(one.view(np.uint32), two.view(np.uint32)) and not np.array_equal(one, bare)
    path_scene = P.Scene(str(d / "plain.json"))
    path_scene.set_environment(d / "Textures" / "sky.hdr", **params)
    assert np.array_equal(path_scene.environment()["map"], a["map"])
    # clear_environment restores the bits of a scene that never had one
    from_file.clear_environment()
    assert from_file.environment() is None
    assert np.array_equal(render(from_file, gui_of("open_d2")).view(np.uint32), bare.view(np.uint32))


def test_cli_env_flags_equal_the_scene_file_s_environment(gpu_device, replays, tmp_path):
    """pathtracer_amd --env FILE --env-scale X --env-rotate X,Y,Z writes the file of the same scene with
    Extensions.ENVIRONMENT, and another one than without an environment."""
    import subprocess
    from cuda_pathtracer_amd import build
    spec = json.loads(Path(replays.scene("open_d2")[2]).read_text())
    d = tmp_path / "cli"
    (d / "Textures").mkdir(parents=True)
    shutil.copy(GOLDEN_HDR, d / "Textures" / "sky.hdr")
    (d / "plain.json").write_text(json.dumps(spec))
    spec["Extensions"]["ENVIRONMENT"] = {"FILE": "sky.hdr", "SCALE": 0.75, "ROTATE": [10.0, 70.0, 5.0]}
    (d / "env.json").write_text(json.dumps(spec))
    outs = {}
    for name, args in (("file", ["env.json"]), ("bare", ["plain.json"]),
                       ("flags", ["plain.json", "--env", str(d / "Textures" / "sky.hdr"), "--env-scale", "0.75", "--env-rotate",
                                  "10,70,5"])):
        out = d / name
        out.mkdir()
        subprocess.run([str(build.CLI), str(d / args[0]), *args[1:], "--iterations", "2", "--out", str(out), "--no-png", "--hdr"],
                       check=True, capture_output=True, timeout=120)
        files = sorted(out.glob("*.hdr"))
        assert len(files) == 1
        outs[name] = files[0].read_bytes()
    assert outs["file"] == outs["flags"] and outs["file"] != outs["bare"]
    bad = subprocess.run([str(build.CLI), str(d / "plain.json"), "--env", str(d / "missing.hdr")], capture_output=True, timeout=120)
    assert bad.returncode != 0 and b"--env" in bad.stderr
