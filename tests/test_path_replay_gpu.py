"""Whole paths on the GPU against a float64 replay that shares no code with the oracle (tests/path_ref.py).

Every other render test compares the kernels with oracle/pt_oracle.cpp bit for bit; both come from one
reading of the reference.  Here PathTracer.render_pass(...).image() must agree, on EVERY kept pixel, with a
numpy restatement of ray generation, shading, scattering and gathering evaluated in float64 with the
kernels' own uniforms (path_ref's header: the order of the draws, the float32 constants, and the rules by
which the float64 side alone excludes a pixel whose path passes a discrete choice too closely).  The scenes
(path_ref.lantern) are closed boxes of emissive tiles, every tile and every object its own colour, so a
pixel is the product of everything its path met: a wrong turn anywhere changes it.

Tolerance: 8 x D_c, where D_c is the largest deviation max_c |a_c - b_c| / max(max_c b_c, 1e-3) of the SAME
replay evaluated in float32 from the float64 one over the kept pixels (float32's own error; the rule of
test_mesh_first_hit_gpu.py).  Measured on the CPU at 48x36 over every tile and iteration set the cases below
use (test_path_replay_cpu.py asserts that the measurement stays at or below D and that both evaluations
take the same route), with the largest share of pixels the float64 side excludes and the smallest share of
kept pixels that are lit:

   replay            scene          depth  flags                             D_c       excluded   lit
   d2                lantern2         2    no jitter, no lens                1.29e-07   1.10 %   82.7 %
   d3                lantern2         3    jitter, lens, roulette            1.36e-07   1.79 %   85.8 %
   d8                lantern2         8    jitter, lens, roulette            1.72e-07   4.46 %   86.1 %
   d8_jitter         lantern2         8    jitter only                       1.62e-07   1.85 %   86.9 %
   d8_single         lantern2         8    d8 with singleAlbedo              1.19e-07   1.74 %   86.2 %
   d2_default        lantern2         2    the default flags                 1.29e-07   1.10 %   83.7 %
   face_d2_default   lantern2_face    2    the default flags                 9.74e-08   0.41 %   99.6 %
   k4_d8             lantern4         8    d8's                              1.64e-07   1.62 %   86.2 %
   mats_d8           lantern2_mats    8    d8's                              1.50e-07   1.74 %   86.2 %
   mesh_bvh          lantern_mesh     4    d8's, BVH                         1.61e-07   1.74 %   85.3 %
   mesh_linear       lantern_mesh     4    d8's, linear without the box      1.61e-07   1.97 %   85.2 %
   mesh_linear_bbox  lantern_mesh     4    d8's, linear with the box cull    1.61e-07   0.98 %   85.7 %

(d8's figures are the extremes over its iteration sets: 1 and 7 — 1.50e-07, 1.74 % — 5..7, 3..7 — the five
iterations of one pass exclude 4.46 %, a pixel being dropped if any of its iterations is — and the two
tiles of world = 2.)

D below holds these rounded up, and never less than 6e-8 = 2^-24.

With rng_key_pixel the image depends neither on the material sort nor on the layout of the paths, so one
replay serves every pipeline variant of a case.  The reference's own key (the compacted index) is covered
at depth 2 only: there the one shading that draws is bounce 0's, where the compacted index of the fused
pipeline is the pixel.  With sortbyMaterial it is not: the reference sorts the paths by material BEFORE it
shades them (pathtrace.cu:479-495), so bounce 0's index is the path's place in the sorted array — on lantern2
the sorted default pipeline differs from the replay on a quarter of the kept pixels (measured on the GPU: 431
of 1709), as it must.  The sorted case therefore looks at one face of the half-mirror cube from so close
that every pixel's first hit has the same material (lantern2_face; test_path_replay_cpu.py asserts it on the
float64 side, with no uncertain first hit): the stable sort then moves nothing, the index is the pixel again,
and the sorted default instantiation — sort, shading, compaction — is held to the same replay.
"""
import sys
from pathlib import Path

import numpy as np
import pytest

import cuda_pathtracer_amd as P

sys.path.insert(0, str(Path(__file__).resolve().parent))
import path_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

LENS = dict(aperture=0.15, focal_len=6.5)
# replay -> (scene, depth, the replay's flags (path_ref.default_flags), mesh path)
REPLAYS = {
    "d2": ("lantern2", 2, dict(ssaa=False, dof=False), "bvh"),
    "d3": ("lantern2", 3, LENS, "bvh"),
    "d8": ("lantern2", 8, LENS, "bvh"),
    "d8_jitter": ("lantern2", 8, dict(dof=False, russianRoulette=False), "bvh"),
    "d8_single": ("lantern2", 8, dict(LENS, singleAlbedo=True), "bvh"),
    "d2_default": ("lantern2", 2, dict(), "bvh"),
    "k4_d8": ("lantern4", 8, LENS, "bvh"),
    "mats_d8": ("lantern2_mats", 8, LENS, "bvh"),
    "face_d2_default": ("lantern2_face", 2, dict(), "bvh"),
    "mesh_bvh": ("lantern_mesh", 4, LENS, "bvh"),
    "mesh_linear": ("lantern_mesh", 4, LENS, "linear"),
    "mesh_linear_bbox": ("lantern_mesh", 4, LENS, "linear_bbox"),
}
D = {"d2": 1.3e-07, "d3": 1.4e-07, "d8": 1.8e-07, "d8_jitter": 1.7e-07, "d8_single": 1.2e-07, "d2_default": 1.3e-07,
     "face_d2_default": 1.0e-07, "k4_d8": 1.7e-07, "mats_d8": 1.5e-07, "mesh_bvh": 1.7e-07, "mesh_linear": 1.7e-07,
     "mesh_linear_bbox": 1.7e-07}
# scene -> path_ref.lantern's arguments
SCENES = {"lantern2": dict(k=2), "lantern4": dict(k=4), "lantern2_mats": dict(k=2, extra_materials=100),
          "lantern_mesh": dict(k=2, mesh=True), "lantern2_face": dict(k=2, face=True)}
# mesh path -> (mesh_ref mode, use_bbox)
PATHS = {"bvh": ("bvh", False), "linear": ("linear", False), "linear_bbox": ("linear", True)}

# case -> replay, further GuiDataContainer attributes, environment, spp, first iteration of every pass, world
CASES = {
    # plain passes: iterations 1 and 7
    "d2": dict(replay="d2"),
    "d3": dict(replay="d3"),
    "d8": dict(replay="d8"),
    "d8_jitter": dict(replay="d8_jitter"),
    "d8_single": dict(replay="d8_single"),
    # pipeline variants of d8
    "d8_sorted": dict(replay="d8", gui=dict(sortbyMaterial=True)),
    "d8_split": dict(replay="d8", env=dict(PT_PIPELINE="split")),
    "d8_spp3": dict(replay="d8", spp=3, passes=(5,)),
    "d8_lanes2_spp5": dict(replay="d8", env=dict(PT_AMD_LANES="2"), spp=5, passes=(3,)),
    "d8_world2": dict(replay="d8", world=2),
    "d8_thrust": dict(replay="d8", gui=dict(useThrustPartition=True), env=dict(PT_PIPELINE="split")),
    # many geoms (the plain loop over the global table), many materials (past the LDS table)
    "k4_d8": dict(replay="k4_d8"),
    "k4_d8_sorted": dict(replay="k4_d8", gui=dict(sortbyMaterial=True)),
    "mats_d8": dict(replay="mats_d8"),
    "mats_d8_sorted": dict(replay="mats_d8", gui=dict(sortbyMaterial=True)),
    # meshes
    "mesh_bvh": dict(replay="mesh_bvh"),
    "mesh_bvh_sorted": dict(replay="mesh_bvh", gui=dict(sortbyMaterial=True)),
    "mesh_linear": dict(replay="mesh_linear"),
    "mesh_linear_bbox": dict(replay="mesh_linear_bbox"),
    # the reference's key: the default instantiations, fused and sorted (the header says why the sorted one
    # needs the face view)
    "d2_refkey": dict(replay="d2_default", gui=dict(rngKeyPixel=False)),
    "face_d2_refkey": dict(replay="face_d2_default", gui=dict(rngKeyPixel=False)),
    "face_d2_refkey_sorted": dict(replay="face_d2_default", gui=dict(rngKeyPixel=False, sortbyMaterial=True)),
}


def case_iterations(case):
    spp = case.get("spp", 1)
    return tuple(it for first in case.get("passes", (1, 7)) for it in range(first, first + spp))


def replay_requests():
    """Every (replay, iterations, rank, world) the cases need, each once."""
    out = []
    for case in CASES.values():
        world = case.get("world", 1)
        for rank in range(world):
            req = (case["replay"], case_iterations(case), rank, world)
            if req not in out:
                out.append(req)
    return out


class Replays:
    """The scenes and the float64 (or dt) replays of a test module: each computed once, left unchanged."""

    def __init__(self, tmp):
        self.tmp, self.scenes, self.cache = tmp, {}, {}

    def scene(self, key):
        """(Scene, texel arrays by texture id, path of its JSON file) of a replay: its scene at its depth."""
        name, depth = REPLAYS[key][:2]
        if (name, depth) not in self.scenes:
            path, textures = R.lantern(self.tmp, depth=depth, **SCENES[name])
            self.scenes[name, depth] = (P.Scene(path), textures, path)
        return self.scenes[name, depth]

    def __call__(self, key, iters, rank=0, world=1, dt=np.float64, variant=None, **flags):
        req = (key, tuple(iters), rank, world, dt, variant, tuple(sorted(flags.items())))
        if req not in self.cache:
            name, depth, fl, path = REPLAYS[key]
            scene, textures, _ = self.scene(key)
            mode, bbox = PATHS[path]
            self.cache[req] = R.replay(scene, textures, tuple(iters), depth, R.default_flags(**dict(fl, **flags)), rank,
                                       world, mode, bbox, dt, variant)
        return self.cache[req]


@pytest.fixture(scope="module")
def replays(tmp_path_factory):
    return Replays(tmp_path_factory.mktemp("path_replay"))


def gui_of(key, **more):
    """The GuiDataContainer of a replay's flags: the global-pixel key unless `more` says otherwise."""
    _, _, fl, path = REPLAYS[key]
    fl = R.default_flags(**fl)
    g = P.GuiDataContainer()
    g.SSAA, g.DoF, g.aperture, g.focal_len = fl["ssaa"], fl["dof"], fl["aperture"], fl["focal_len"]
    g.russianRoulette, g.singleAlbedo, g.rngKeyPixel = fl["russianRoulette"], fl["singleAlbedo"], True
    g.useBVHtree, g.useBBox = path == "bvh", path != "linear"
    for k, v in more.items():
        assert hasattr(g, k), k
        setattr(g, k, v)
    return g


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


@pytest.mark.parametrize("name", list(CASES))
def test_render_agrees_with_the_float64_replay_on_every_kept_pixel(gpu_device, replays, monkeypatch, name):
    case = CASES[name]
    key = case["replay"]
    scene, _, _ = replays.scene(key)
    assert scene.state().traceDepth == REPLAYS[key][1]
    for k, v in case.get("env", {}).items():
        monkeypatch.setenv(k, v)
    world, spp = case.get("world", 1), case.get("spp", 1)
    for rank in range(world):
        ref = replays(key, case_iterations(case), rank, world)
        assert 1.0 - ref["keep"].mean() <= 0.05                   # (float64 side alone)
        pt = P.PathTracer(scene, gui_of(key, **case.get("gui", {})), rank=rank, world=world, spp=spp)
        for first in case.get("passes", (1, 7)):
            pt.render_pass(first)
        got = pt.image()
        pt.free()
        text = mismatches(f"{name} rank {rank}/{world}", got, ref, 8 * D[key])
        assert not text, text
