"""Mesh first hits on the GPU against a float64 brute-force reference (tests/mesh_ref.py).

The G-buffer's material, t, P, n and uv of every kept pixel are compared with a float64 evaluation of
the reference's text over EVERY triangle (no BVH), for the pair walk, the node-at-a-time walk with its
cull and the two linear modes; a depth-1 render of emissive geoms shows that the render path's walks
(4-wide, pairs, sorted) pick the same geom; and the smooth-normal scene renders bit for bit like the
oracle.  The scenes (mesh_ref.smooth_scene, mesh_ref.room_view) have what the bundled ones lack:
smooth per-vertex normals and texture coordinates under rotated, non-uniform and mirrored scales, and
cameras that fill the frame with triangles.

Tolerances: 8x the error the same reference shows when evaluated in float32 (float32's own error;
the rule of test_denoise_gpu.py), taken apart by the kind of surface the pixel shows — "tri" a
triangle, "prim" a cube or sphere (whose 1e-4 back-off costs two decimal digits more) — and by the mesh
path ("bvh", "linear", "linear_bbox": mesh_ref's modes).  Measured on the CPU at 48x36, float32 against
float64 on the kept pixels (mesh_ref.deviations; test_mesh_first_hit_cpu.py asserts that the measurement
stays at or below D), with the share of pixels the float64 side excludes:

                                          tri: D_t      D_p      D_n      D_uv     prim: D_t      D_p      D_n
   smooth     bvh         excluded 0.98 %     6.74e-07 6.64e-07 6.88e-06 2.05e-06       1.15e-05 1.13e-05 1.79e-04
   smooth     linear      excluded 0.98 %     6.74e-07 6.64e-07 3.32e-06 4.71e-05       1.15e-05 1.13e-05 1.79e-04
   smooth     linear_bbox excluded 0.12 %     4.29e-07 4.56e-07 2.05e-07 1.40e-06       1.15e-05 1.13e-05 1.79e-04
   room_chair bvh         excluded 1.33 %     2.92e-07 3.11e-07 9.93e-08 6.04e-06       3.19e-07 3.61e-07 5.96e-08
   room_chair linear      excluded 1.33 %     2.92e-07 3.11e-07 7.82e-08 2.02e-05       3.19e-07 3.61e-07 5.96e-08
   room_chair linear_bbox excluded 0.69 %     2.88e-07 3.11e-07 7.17e-08 1.11e-05       3.19e-07 3.61e-07 5.96e-08
   room_wall  bvh         excluded 0.29 %     1.24e-06 1.24e-06 8.23e-15 1.61e-06       (no such pixel)
   room_wall  linear      excluded 0.29 %     1.24e-06 1.24e-06 5.96e-08 9.26e-07       (no such pixel)
   room_wall  linear_bbox excluded 0.00 %     (no such pixel)                           1.93e-07 2.56e-07 5.96e-08

D below holds these rounded up, and never less than 6e-8 = 2^-24: one rounding of a number of magnitude
1 (room_wall's normals are the axis (0, 0, 1) exactly, where this evaluation happens to round nothing).
(linear D_uv is larger because meshIntersectionTest's uv, w*uv0 + uv1 + uv2, is a sum of magnitude 2-3.)

What "linear" means with more than one mesh (mesh_ref.py's header): meshIntersectionTest indexes the
triangle array the BVH build has reordered by POSITION, so a geom tests and lends its material to
triangles of other meshes, and with the box cull the triangles in the range of a geom whose box the ray
misses are not seen at all (room_wall: the whole wall).  The kernels and the oracle do the same; the
float64 reference follows that text, not the id ranges.
"""
import sys
from pathlib import Path

import numpy as np
import pytest

import cuda_pathtracer_amd as P
from oracle import binding as O

sys.path.insert(0, str(Path(__file__).resolve().parent))
import mesh_ref as M  # noqa: E402

pytestmark = pytest.mark.gpu

# (scene, mesh path) -> kind -> (D_t, D_p, D_n, D_uv)
D = {
    ("smooth", "bvh"): {"tri": (6.8e-07, 6.7e-07, 6.9e-06, 2.1e-06), "prim": (1.2e-05, 1.2e-05, 1.8e-04, 0.0)},
    ("smooth", "linear"): {"tri": (6.8e-07, 6.7e-07, 3.4e-06, 4.8e-05), "prim": (1.2e-05, 1.2e-05, 1.8e-04, 0.0)},
    ("smooth", "linear_bbox"): {"tri": (4.3e-07, 4.6e-07, 2.1e-07, 1.4e-06), "prim": (1.2e-05, 1.2e-05, 1.8e-04, 0.0)},
    ("room_chair", "bvh"): {"tri": (3.0e-07, 3.2e-07, 1.0e-07, 6.1e-06), "prim": (3.2e-07, 3.7e-07, 6e-08, 0.0)},
    ("room_chair", "linear"): {"tri": (3.0e-07, 3.2e-07, 7.9e-08, 2.1e-05), "prim": (3.2e-07, 3.7e-07, 6e-08, 0.0)},
    ("room_chair", "linear_bbox"): {"tri": (2.9e-07, 3.2e-07, 7.2e-08, 1.2e-05), "prim": (3.2e-07, 3.7e-07, 6e-08, 0.0)},
    ("room_wall", "bvh"): {"tri": (1.3e-06, 1.3e-06, 6e-08, 1.7e-06), "prim": (0.0, 0.0, 0.0, 0.0)},
    ("room_wall", "linear"): {"tri": (1.3e-06, 1.3e-06, 6e-08, 9.3e-07), "prim": (0.0, 0.0, 0.0, 0.0)},
    ("room_wall", "linear_bbox"): {"tri": (0.0, 0.0, 0.0, 0.0), "prim": (2.0e-07, 2.6e-07, 6e-08, 0.0)},
}
# mesh path -> (mesh_ref mode, use_bbox)
PATHS = {"bvh": ("bvh", False), "linear": ("linear", False), "linear_bbox": ("linear", True)}
# flag set -> (GuiDataContainer attributes, the mesh path they select)
FLAGS = {
    "default": (dict(), "bvh"),                                        # the pair walk
    "cull": (dict(bvhCull=True), "bvh"),                               # the node-at-a-time walk with the cull
    "linear_bbox": (dict(useBVHtree=False), "linear_bbox"),
    "linear": (dict(useBVHtree=False, useBBox=False), "linear"),
}


def _gui(**kw):
    g = P.GuiDataContainer()
    for k, v in kw.items():
        assert hasattr(g, k), k
        setattr(g, k, v)
    return g


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    """(scene name, mesh path) -> (scene, float64 reference), each computed once and left unchanged."""
    tmp = tmp_path_factory.mktemp("mesh_first_hit")
    scenes, cache = {}, {}

    def get(name, path):
        if name not in scenes:
            sc = P.Scene(M.mesh_scene(tmp, name))
            scenes[name] = (sc, M.triangle_table(sc))
        if (name, path) not in cache:
            sc, tris = scenes[name]
            mode, bbox = PATHS[path]
            cache[name, path] = M.mesh_first_hit_ref(tris, sc.geoms(), sc.camera(), np.float64, mode, use_bbox=bbox)
        return scenes[name][0], cache[name, path]
    return get


# ---- the G-buffer against float64 ------------------------------------------------------------------------
@pytest.mark.parametrize("flags", list(FLAGS))
@pytest.mark.parametrize("name", M.MESH_SCENES)
def test_gbuffer_of_mesh_scenes_within_8x_of_float32s_own_error(gpu_device, refs, name, flags):
    kw, path = FLAGS[flags]
    scene, ref = refs(name, path)
    keep = ref["keep"]
    assert 1.0 - keep.mean() <= 0.05                      # (float64 side alone)
    pt = P.PathTracer(scene, _gui(**kw))
    g = pt.gbuffer()
    pt.free()
    bad = keep & (g["mat"] != ref["mat"])
    assert not bad.any(), (name, flags, int(bad.sum()), np.argwhere(bad)[:4].tolist(), g["mat"][bad][:4], ref["mat"][bad][:4])
    e = M.errors(ref, g["t"], g["position"], g["normal"], g["uv"])
    for kind in ("tri", "prim"):
        print(f"{name} {flags} {kind}: GPU e_t={e[kind][0]:.3e} e_p={e[kind][1]:.3e} e_n={e[kind][2]:.3e} "
              f"e_uv={e[kind][3]:.3e}")
    for kind in ("tri", "prim"):
        for what, got, d in zip(("t", "P", "n", "uv"), e[kind], D[name, path][kind]):
            assert got <= 8 * d, (name, flags, kind, what, got, d)


# ---- the render path's walks pick the same geom ----------------------------------------------------------------
@pytest.fixture(scope="module")
def emissive(tmp_path_factory):
    """The smooth scene with every geom emitting its own colour, and its float64 reference."""
    sc = P.Scene(M.smooth_scene(tmp_path_factory.mktemp("mesh_emissive"), emissive=True))
    ref = M.mesh_first_hit_ref(M.triangle_table(sc), sc.geoms(), sc.camera(), np.float64, "bvh")
    return sc, ref


@pytest.mark.parametrize("walk", ["quad", "pairs", "sorted"])
def test_render_path_picks_the_float64_geom(gpu_device, emissive, monkeypatch, walk):
    """One iteration at depth 1 without jitter or lens: a pixel's colour is its geom's (mesh_ref.smooth_colour).
    quad: the 4-wide walk ahead of the bounce kernel; pairs: PT_AMD_TRAV=pairs; sorted: sortbyMaterial."""
    scene, ref = emissive
    if walk == "pairs":
        monkeypatch.setenv("PT_AMD_TRAV", "pairs")
    assert scene.state().traceDepth == 1
    pt = P.PathTracer(scene, _gui(SSAA=False, DoF=False, sortbyMaterial=walk == "sorted"))
    assert pt.walk_info()["quad_walk"] == (walk != "pairs")
    pt.render_pass(1)
    img = pt.image()
    pt.free()
    geom = np.full(img.shape[:2], -2, np.int32)
    geom[(img == 0).all(axis=-1)] = -1
    for i in range(len(M.SMOOTH_OBJECTS)):
        geom[(img == np.array(M.smooth_colour(i), np.float32)).all(axis=-1)] = i
    assert (geom >= -1).all(), "a pixel shows no geom's colour"
    keep = ref["keep"]
    bad = keep & (geom != ref["geom"])
    assert not bad.any(), (walk, int(bad.sum()), np.argwhere(bad)[:4].tolist(), geom[bad][:4], ref["geom"][bad][:4])
    assert len(np.unique(geom[keep])) == len(M.SMOOTH_OBJECTS) + 1      # every geom and the background


# ---- smooth normals steer the bounces: bit for bit like the oracle -----------------------------------------------
@pytest.mark.parametrize("kw,spp", [
    (dict(), 1),
    (dict(useBVHtree=False), 1),
    (dict(useBVHtree=False, useBBox=False), 1),
    (dict(sortbyMaterial=True), 1),
    (dict(bvhCull=True), 1),
    (dict(), 3),
], ids=["default", "linear_bbox", "linear", "sorted", "cull", "spp3"])
def test_smooth_scene_renders_bitexact(gpu_device, tmp_path, kw, spp):
    path = M.smooth_scene(tmp_path, sky=True)
    scene, oscene = P.Scene(path), O.OracleScene.from_json(path)
    gui = _gui(**kw)
    fl = O.flags(gui.russianRoulette, gui.useBVHtree, gui.useBBox, gui.sortbyMaterial, gui.useThrustPartition, gui.SSAA,
                 gui.DoF, gui.aperture, gui.focal_len, gui.singleAlbedo, gui.rngKeyPixel)
    pt = P.PathTracer(scene, gui, spp=spp)
    want = None
    for it in range(1, 3 if spp == 1 else 2):          # two iterations, or one pass of three
        pt.render_pass(it)
        want, _ = O.render_pass(oscene, fl, it, spp=spp, image=want)
    got = pt.image()
    pt.free()
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    assert same.all(), (kw, spp, int((~same).sum()), np.argwhere(~same)[:3].tolist())
    assert (want > 0).mean() > 0.5                        # (most paths reach a light, whatever they met)
