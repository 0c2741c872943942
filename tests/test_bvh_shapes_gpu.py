"""The walk kernels on degenerate BVH shapes (tests/bvh_shape_cases.py): big leaves, deep chains, a root
that is a leaf.  Which walk a context runs is decided by the tree's shape:

  a leaf over 255 triangles     no pair and no quad layout: every mesh kernel runs the node walk  (leaf256, leaf300, leaf300x2)
  any leaf code                 -(first * 256 + count) - 1, decoded c >> 8, c & 255 by three walks  (leaf255: the largest that fits)
  bvh_depth >= 32 (kLdsStack)   the inline walk leaves the LDS stack and the pairs for 64 private entries  (chain31 | chain32)
  bvh_depth + 2 > 64            k_traverse drops the pair walk for the node walk  (chain62 | chain63 under PT_AMD_TRAV=pairs)
  stack occupancy reaches 64    the reference's rule: the interior node is skipped, its subtree dropped  (chain_over)
  quad stack bound past 64      make_quads refuses; the pair walk, or past depth 62 the node walk, runs  (chain_over)
  quad bound past kTrav4LdsRows the quad walk's stack spills past its 16 LDS rows  (every chain; PT_AMD_STACK_ROWS=1: all of it)
  the root is a leaf            root_code is a leaf code, the quad table one zeroed entry  (root1, root5)
  device builder, chain > 62    k_bvh_small's 64-task stack sets error bit 2, the host builds  (chain62_pos | chain63_pos)

Every test asserts the class its case names (bvh_shape_cases.classify) and the walk that ran, from
PathTracer.walk_info() (walk / inline_walk: pt_ctx_walk_kind, the kernels' own predicates) and the
profile's traverse launches; test_bvh_shapes_cpu.py checks the same cases' stack occupancies on the CPU.

Tolerances of the G-buffer test: 8x float32's own error D, the rule of test_mesh_first_hit_gpu.py,
measured on the CPU at 32 x 24 (mesh_ref.deviations, float32 against float64 on the kept pixels;
test_bvh_shapes_cpu.py asserts that the measurement stays at or below D) with the share of pixels the
float64 side excludes (cap: 5 %).  D holds the figures rounded up, never below 6e-8 = 2^-24:

                                          tri: D_t      D_p      D_n      D_uv     prim: D_t      D_p      D_n
   leaf255    bvh         excluded 0.26 %     1.09e-06 9.08e-07 1.24e-07 5.96e-08       2.75e-06 2.60e-06 4.16e-05
   leaf255    linear      excluded 0.26 %     1.09e-06 9.08e-07 1.01e-07 4.16e-06       2.75e-06 2.60e-06 4.16e-05
   leaf255    linear_bbox excluded 0.26 %     1.09e-06 9.08e-07 1.01e-07 4.16e-06       2.75e-06 2.60e-06 4.16e-05
   leaf256    bvh         excluded 0.13 %     2.82e-07 3.29e-07 1.24e-07 5.96e-08       2.75e-06 2.60e-06 4.16e-05
   leaf256    linear      excluded 0.13 %     2.82e-07 3.29e-07 1.30e-07 2.79e-06       2.75e-06 2.60e-06 4.16e-05
   leaf256    linear_bbox excluded 0.13 %     2.82e-07 3.29e-07 1.30e-07 2.79e-06       2.75e-06 2.60e-06 4.16e-05
   leaf300    bvh         excluded 0.13 %     2.58e-07 2.57e-07 1.24e-07 5.96e-08       2.75e-06 2.60e-06 4.16e-05
   leaf300    linear      excluded 0.13 %     2.58e-07 2.57e-07 1.11e-07 9.66e-07       2.75e-06 2.60e-06 4.16e-05
   leaf300    linear_bbox excluded 0.13 %     2.58e-07 2.57e-07 1.11e-07 9.66e-07       2.75e-06 2.60e-06 4.16e-05
   leaf300x2  bvh         excluded 0.39 %     2.82e-07 2.96e-07 1.01e-07 1.19e-07       3.20e-06 3.00e-06 2.30e-05
   leaf300x2  linear      excluded 0.39 %     2.82e-07 2.96e-07 9.66e-08 3.78e-06       3.20e-06 3.00e-06 2.30e-05
   leaf300x2  linear_bbox excluded 0.39 %     2.82e-07 2.96e-07 9.66e-08 3.78e-06       3.20e-06 3.00e-06 2.30e-05
   root1      bvh         excluded 0.00 %     1.58e-07 2.19e-07 8.38e-08 3.73e-09       6.42e-06 6.30e-06 2.06e-04
   root1      linear      excluded 0.00 %     1.58e-07 2.19e-07 1.43e-07 6.99e-09       6.42e-06 6.30e-06 2.06e-04
   root1      linear_bbox excluded 0.00 %     1.58e-07 2.19e-07 1.43e-07 6.99e-09       6.42e-06 6.30e-06 2.06e-04
   root5      bvh         excluded 0.13 %     1.83e-07 2.44e-07 1.24e-07 5.96e-08       6.42e-06 6.30e-06 2.06e-04
   root5      linear      excluded 0.13 %     1.83e-07 2.44e-07 9.66e-08 1.51e-07       6.42e-06 6.30e-06 2.06e-04
   root5      linear_bbox excluded 0.26 %     1.83e-07 2.44e-07 9.66e-08 1.51e-07       6.42e-06 6.30e-06 2.06e-04
   chain30    bvh         excluded 0.26 %     6.12e-08 9.44e-08 4.92e-08 2.98e-08       9.56e-07 9.17e-07 9.75e-06
   chain30    linear      excluded 0.26 %     6.12e-08 9.44e-08 7.00e-08 2.73e-07       9.56e-07 9.17e-07 9.75e-06
   chain30    linear_bbox excluded 0.26 %     6.12e-08 9.44e-08 7.00e-08 2.73e-07       9.56e-07 9.17e-07 9.75e-06
   chain31    bvh         excluded 0.26 %     6.12e-08 9.44e-08 4.92e-08 2.98e-08       9.56e-07 9.17e-07 9.75e-06
   chain31    linear      excluded 0.26 %     6.12e-08 9.44e-08 7.00e-08 2.73e-07       9.56e-07 9.17e-07 9.75e-06
   chain31    linear_bbox excluded 0.26 %     6.12e-08 9.44e-08 7.00e-08 2.73e-07       9.56e-07 9.17e-07 9.75e-06
   chain32    bvh         excluded 0.26 %     6.12e-08 9.44e-08 4.92e-08 2.98e-08       9.56e-07 9.17e-07 9.75e-06
   chain32    linear      excluded 0.26 %     6.12e-08 9.44e-08 7.00e-08 2.73e-07       9.56e-07 9.17e-07 9.75e-06
   chain32    linear_bbox excluded 0.26 %     6.12e-08 9.44e-08 7.00e-08 2.73e-07       9.56e-07 9.17e-07 9.75e-06
   chain61    bvh         excluded 0.26 %     6.12e-08 9.44e-08 4.92e-08 2.98e-08       9.56e-07 9.17e-07 9.75e-06
   chain61    linear      excluded 0.26 %     6.12e-08 9.44e-08 7.00e-08 2.73e-07       9.56e-07 9.17e-07 9.75e-06
   chain61    linear_bbox excluded 0.26 %     6.12e-08 9.44e-08 7.00e-08 2.73e-07       9.56e-07 9.17e-07 9.75e-06
   chain62    bvh         excluded 0.26 %     6.12e-08 9.44e-08 4.92e-08 2.98e-08       9.56e-07 9.17e-07 9.75e-06
   chain62    linear      excluded 0.26 %     6.12e-08 9.44e-08 7.00e-08 2.73e-07       9.56e-07 9.17e-07 9.75e-06
   chain62    linear_bbox excluded 0.26 %     6.12e-08 9.44e-08 7.00e-08 2.73e-07       9.56e-07 9.17e-07 9.75e-06
   chain63    bvh         excluded 0.26 %     6.12e-08 9.44e-08 4.92e-08 2.98e-08       9.56e-07 9.17e-07 9.75e-06
   chain63    linear      excluded 0.26 %     6.12e-08 9.44e-08 7.00e-08 2.73e-07       9.56e-07 9.17e-07 9.75e-06
   chain63    linear_bbox excluded 0.26 %     6.12e-08 9.44e-08 7.00e-08 2.73e-07       9.56e-07 9.17e-07 9.75e-06
"""
import sys
from pathlib import Path

import numpy as np
import pytest

import cuda_pathtracer_amd as P
from oracle import binding as O

sys.path.insert(0, str(Path(__file__).resolve().parent))
import bvh_shape_cases as B  # noqa: E402
import mesh_ref as M  # noqa: E402
from test_bvh_device_gpu import _tables  # noqa: E402

pytestmark = pytest.mark.gpu

EXCLUDED_CAP = 0.05
# mesh path -> (mesh_ref mode, use_bbox)
PATHS = {"bvh": ("bvh", False), "linear": ("linear", False), "linear_bbox": ("linear", True)}
# flag set -> (GuiDataContainer attributes, the mesh path they select)
FLAGS = {
    "default": (dict(), "bvh"),
    "cull": (dict(bvhCull=True), "bvh"),
    "linear_bbox": (dict(useBVHtree=False), "linear_bbox"),
    "linear": (dict(useBVHtree=False, useBBox=False), "linear"),
}
# (case, mesh path) -> kind -> (D_t, D_p, D_n, D_uv)
D = {
    ("leaf255", "bvh"): {"tri": (1.1e-06, 9.1e-07, 1.3e-07, 6.0e-08), "prim": (2.8e-06, 2.7e-06, 4.2e-05, 0.0)},
    ("leaf255", "linear"): {"tri": (1.1e-06, 9.1e-07, 1.1e-07, 4.2e-06), "prim": (2.8e-06, 2.7e-06, 4.2e-05, 0.0)},
    ("leaf255", "linear_bbox"): {"tri": (1.1e-06, 9.1e-07, 1.1e-07, 4.2e-06), "prim": (2.8e-06, 2.7e-06, 4.2e-05, 0.0)},
    ("leaf256", "bvh"): {"tri": (2.9e-07, 3.3e-07, 1.3e-07, 6.0e-08), "prim": (2.8e-06, 2.7e-06, 4.2e-05, 0.0)},
    ("leaf256", "linear"): {"tri": (2.9e-07, 3.3e-07, 1.4e-07, 2.8e-06), "prim": (2.8e-06, 2.7e-06, 4.2e-05, 0.0)},
    ("leaf256", "linear_bbox"): {"tri": (2.9e-07, 3.3e-07, 1.4e-07, 2.8e-06), "prim": (2.8e-06, 2.7e-06, 4.2e-05, 0.0)},
    ("leaf300", "bvh"): {"tri": (2.6e-07, 2.6e-07, 1.3e-07, 6.0e-08), "prim": (2.8e-06, 2.7e-06, 4.2e-05, 0.0)},
    ("leaf300", "linear"): {"tri": (2.6e-07, 2.6e-07, 1.2e-07, 9.7e-07), "prim": (2.8e-06, 2.7e-06, 4.2e-05, 0.0)},
    ("leaf300", "linear_bbox"): {"tri": (2.6e-07, 2.6e-07, 1.2e-07, 9.7e-07), "prim": (2.8e-06, 2.7e-06, 4.2e-05, 0.0)},
    ("leaf300x2", "bvh"): {"tri": (2.9e-07, 3.0e-07, 1.1e-07, 1.2e-07), "prim": (3.3e-06, 3.1e-06, 2.3e-05, 0.0)},
    ("leaf300x2", "linear"): {"tri": (2.9e-07, 3.0e-07, 9.7e-08, 3.8e-06), "prim": (3.3e-06, 3.1e-06, 2.3e-05, 0.0)},
    ("leaf300x2", "linear_bbox"): {"tri": (2.9e-07, 3.0e-07, 9.7e-08, 3.8e-06), "prim": (3.3e-06, 3.1e-06, 2.3e-05, 0.0)},
    ("root1", "bvh"): {"tri": (1.6e-07, 2.2e-07, 8.4e-08, 6.0e-08), "prim": (6.5e-06, 6.4e-06, 2.1e-04, 0.0)},
    ("root1", "linear"): {"tri": (1.6e-07, 2.2e-07, 1.5e-07, 6.0e-08), "prim": (6.5e-06, 6.4e-06, 2.1e-04, 0.0)},
    ("root1", "linear_bbox"): {"tri": (1.6e-07, 2.2e-07, 1.5e-07, 6.0e-08), "prim": (6.5e-06, 6.4e-06, 2.1e-04, 0.0)},
    ("root5", "bvh"): {"tri": (1.9e-07, 2.5e-07, 1.3e-07, 6.0e-08), "prim": (6.5e-06, 6.4e-06, 2.1e-04, 0.0)},
    ("root5", "linear"): {"tri": (1.9e-07, 2.5e-07, 9.7e-08, 1.6e-07), "prim": (6.5e-06, 6.4e-06, 2.1e-04, 0.0)},
    ("root5", "linear_bbox"): {"tri": (1.9e-07, 2.5e-07, 9.7e-08, 1.6e-07), "prim": (6.5e-06, 6.4e-06, 2.1e-04, 0.0)},
    ("chain30", "bvh"): {"tri": (6.2e-08, 9.5e-08, 6.0e-08, 6.0e-08), "prim": (9.6e-07, 9.2e-07, 9.8e-06, 0.0)},
    ("chain30", "linear"): {"tri": (6.2e-08, 9.5e-08, 7.0e-08, 2.8e-07), "prim": (9.6e-07, 9.2e-07, 9.8e-06, 0.0)},
    ("chain30", "linear_bbox"): {"tri": (6.2e-08, 9.5e-08, 7.0e-08, 2.8e-07), "prim": (9.6e-07, 9.2e-07, 9.8e-06, 0.0)},
    ("chain31", "bvh"): {"tri": (6.2e-08, 9.5e-08, 6.0e-08, 6.0e-08), "prim": (9.6e-07, 9.2e-07, 9.8e-06, 0.0)},
    ("chain31", "linear"): {"tri": (6.2e-08, 9.5e-08, 7.0e-08, 2.8e-07), "prim": (9.6e-07, 9.2e-07, 9.8e-06, 0.0)},
    ("chain31", "linear_bbox"): {"tri": (6.2e-08, 9.5e-08, 7.0e-08, 2.8e-07), "prim": (9.6e-07, 9.2e-07, 9.8e-06, 0.0)},
    ("chain32", "bvh"): {"tri": (6.2e-08, 9.5e-08, 6.0e-08, 6.0e-08), "prim": (9.6e-07, 9.2e-07, 9.8e-06, 0.0)},
    ("chain32", "linear"): {"tri": (6.2e-08, 9.5e-08, 7.0e-08, 2.8e-07), "prim": (9.6e-07, 9.2e-07, 9.8e-06, 0.0)},
    ("chain32", "linear_bbox"): {"tri": (6.2e-08, 9.5e-08, 7.0e-08, 2.8e-07), "prim": (9.6e-07, 9.2e-07, 9.8e-06, 0.0)},
    ("chain61", "bvh"): {"tri": (6.2e-08, 9.5e-08, 6.0e-08, 6.0e-08), "prim": (9.6e-07, 9.2e-07, 9.8e-06, 0.0)},
    ("chain61", "linear"): {"tri": (6.2e-08, 9.5e-08, 7.0e-08, 2.8e-07), "prim": (9.6e-07, 9.2e-07, 9.8e-06, 0.0)},
    ("chain61", "linear_bbox"): {"tri": (6.2e-08, 9.5e-08, 7.0e-08, 2.8e-07), "prim": (9.6e-07, 9.2e-07, 9.8e-06, 0.0)},
    ("chain62", "bvh"): {"tri": (6.2e-08, 9.5e-08, 6.0e-08, 6.0e-08), "prim": (9.6e-07, 9.2e-07, 9.8e-06, 0.0)},
    ("chain62", "linear"): {"tri": (6.2e-08, 9.5e-08, 7.0e-08, 2.8e-07), "prim": (9.6e-07, 9.2e-07, 9.8e-06, 0.0)},
    ("chain62", "linear_bbox"): {"tri": (6.2e-08, 9.5e-08, 7.0e-08, 2.8e-07), "prim": (9.6e-07, 9.2e-07, 9.8e-06, 0.0)},
    ("chain63", "bvh"): {"tri": (6.2e-08, 9.5e-08, 6.0e-08, 6.0e-08), "prim": (9.6e-07, 9.2e-07, 9.8e-06, 0.0)},
    ("chain63", "linear"): {"tri": (6.2e-08, 9.5e-08, 7.0e-08, 2.8e-07), "prim": (9.6e-07, 9.2e-07, 9.8e-06, 0.0)},
    ("chain63", "linear_bbox"): {"tri": (6.2e-08, 9.5e-08, 7.0e-08, 2.8e-07), "prim": (9.6e-07, 9.2e-07, 9.8e-06, 0.0)},
}
ALL = list(B.CASES)
NOT_OVER = [n for n in ALL if n != "chain_over"]


def _gui(**kw):
    g = P.GuiDataContainer()
    for k, v in kw.items():
        assert hasattr(g, k), k
        setattr(g, k, v)
    return g


def expected_walks(cls, nq):
    """(the walk ahead of the bounce kernel, the walk inside it) for a tree of this class, by the rows of
    the table above."""
    fits = cls["big_leaves"] == 0
    pre = "quads" if nq else "pairs" if fits and cls["depth"] + 2 <= 64 else "nodes"
    inline = "nodes_private" if cls["depth"] >= 32 else "pairs" if fits else "nodes"
    return pre, inline


@pytest.fixture(scope="module")
def shapes(tmp_path_factory):
    """name -> dict(path, emissive path, scene, class, quad entries); float64 references per mesh path.
    Each is computed once and left unchanged."""
    tmp = tmp_path_factory.mktemp("bvh_shapes")
    made = {}

    def get(name):
        if name not in made:
            path = B.scene_file(tmp, name)
            sc = B.load(path, name)
            cls = B.classify(sc)
            want = B.CASES[name][2]
            assert {k: cls[k] for k in want} == want, (name, cls)
            nq = B.quads_of(sc)[0]
            assert (nq > 0) == B.CASES[name][3]
            made[name] = dict(path=path, epath=B.scene_file(tmp, name, emissive=True), scene=sc, cls=cls, nq=nq,
                              refs={}, tris=M.triangle_table(sc))
        return made[name]

    def ref(name, path):
        s = get(name)
        if path not in s["refs"]:
            mode, bbox = PATHS[path]
            s["refs"][path] = M.mesh_first_hit_ref(s["tris"], s["scene"].geoms(), s["scene"].camera(), np.float64, mode,
                                                   use_bbox=bbox)
        return s["refs"][path]
    get.ref = ref
    return get


# ---- the G-buffer against float64 ------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", list(FLAGS))
@pytest.mark.parametrize("name", NOT_OVER)
def test_gbuffer_of_shape_scenes_within_8x_of_float32s_own_error(gpu_device, shapes, name, flags):
    kw, path = FLAGS[flags]
    s, ref = shapes(name), shapes.ref(name, path)
    keep = ref["keep"]
    assert 1.0 - keep.mean() <= EXCLUDED_CAP                      # (float64 side alone)
    pt = P.PathTracer(s["scene"], _gui(**kw))
    info = pt.walk_info()
    g = pt.gbuffer()
    pt.free()
    _, inline = expected_walks(s["cls"], s["nq"])
    if flags == "cull" and inline == "pairs":
        inline = "nodes"                                            # the cull runs on the node walk only
    assert info["inline_walk"] == (inline if path == "bvh" else "none"), info
    assert info["bvh_depth"] == s["cls"]["depth"]
    bad = keep & (g["mat"] != ref["mat"])
    assert not bad.any(), (name, flags, int(bad.sum()), np.argwhere(bad)[:4].tolist(), g["mat"][bad][:4], ref["mat"][bad][:4])
    e = M.errors(ref, g["t"], g["position"], g["normal"], g["uv"])
    for kind in ("tri", "prim"):
        print(f"{name} {flags} {kind}: GPU e_t={e[kind][0]:.3e} e_p={e[kind][1]:.3e} e_n={e[kind][2]:.3e} "
              f"e_uv={e[kind][3]:.3e}")
    for kind in ("tri", "prim"):
        for what, got, d in zip(("t", "P", "n", "uv"), e[kind], D[name, path][kind]):
            assert got <= 8 * d, (name, flags, kind, what, got, d)
    if path == "bvh":   # the uv names the triangle (Triangle::intersect's weights sum to 1): the float64 side's
        tri = keep & (ref["tri"] >= 0)
        want = np.array([B.uv_of(i) for i in range(len(s["tris"]))])[np.maximum(ref["tri"], 0)]
        assert tri.any() and np.abs(g["uv"][tri] - want[tri]).max() < 2.0 ** -11


# ---- the render path's walks: one depth-1 emissive iteration, every variant the same bits as the oracle --------
# variant -> (environment, GuiDataContainer attributes, where the walk runs: "pre" | "inline")
VARIANTS = {
    "default": ({}, {}, "pre"),
    "pairs": ({"PT_AMD_TRAV": "pairs"}, {}, "pre"),
    "inline": ({"PT_AMD_MESH_INLINE": "1"}, {}, "inline"),
    "sorted": ({}, dict(sortbyMaterial=True), "inline"),
    "split": ({"PT_PIPELINE": "split"}, {}, "inline"),
    "cull": ({}, dict(bvhCull=True), "pre"),
    "tasks1": ({"PT_AMD_WALK_TASKS": "1"}, {}, "pre"),
    "tasks2": ({"PT_AMD_WALK_TASKS": "2"}, {}, "pre"),
    "tcull": ({"PT_AMD_TCULL": "1"}, {}, "pre"),
    "rows1": ({"PT_AMD_STACK_ROWS": "1"}, {}, "pre"),
}


@pytest.fixture(scope="module")
def emissive_oracle(shapes):
    """name -> (the emissive scene, the oracle's image of iteration 1 at depth 1 without jitter or lens)."""
    made = {}

    def get(name):
        if name not in made:
            s = shapes(name)
            osc = B.load_oracle(s["epath"], name)
            assert osc.depth == 1
            img, _ = O.render_pass(osc, O.flags(ssaa=False, dof=False), 1)
            made[name] = (B.load(s["epath"], name), img)
        return made[name]
    return get


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", ALL)
def test_render_path_walks_give_the_oracles_bits(gpu_device, shapes, emissive_oracle, monkeypatch, name, variant):
    env, kw, where = VARIANTS[variant]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    s = shapes(name)
    scene, want = emissive_oracle(name)
    pre, inline = expected_walks(s["cls"], s["nq"])
    if variant == "pairs" and pre == "quads":
        pre = "pairs" if s["cls"]["depth"] + 2 <= 64 else "nodes"
    if variant == "cull":
        pre, inline = "nodes", ("nodes" if inline == "pairs" else inline)
    pt = P.PathTracer(scene, _gui(SSAA=False, DoF=False, **kw))
    try:
        info = pt.walk_info()
        assert info["walk"] == (pre if where == "pre" else "none"), (name, variant, info)
        assert info["inline_walk"] == inline, (name, variant, info)
        assert info["quad_walk"] == (s["nq"] > 0 and variant != "pairs")      # (the layout is in use, cull aside)
        if name in B.BIG or name == "chain_over":
            assert not info["quad_walk"]
        if name == "chain62":
            assert info["quad_walk"] == (variant != "pairs") and info["stack_bound"] > 16
        if variant == "tcull":
            assert info["tcull"] == (s["nq"] > 0)
        pt.profile(True)
        pt.render_pass(1)
        got = pt.image()
        kinds = pt.profile_read()
        walks = kinds["traverse"][1] + kinds["first_traverse"][1]
        assert kinds["first_bounce"][1] == 1 and (walks > 0) == (where == "pre"), kinds
    finally:
        pt.free()
    same = got == want
    assert same.all(), (name, variant, int((~same).sum()), np.argwhere(~same)[:4].tolist())
    assert len(np.unique(want.reshape(-1, 3), axis=0)) == 3            # background, mesh, sphere (the light is behind the camera)


# ---- whole paths: bit for bit like the oracle ----------------------------------------------------------------
@pytest.mark.parametrize("kw,spp", [(dict(), 1), (dict(sortbyMaterial=True), 1), (dict(), 3), (dict(sortbyMaterial=True), 3)],
                         ids=["default", "sorted", "spp3", "sorted_spp3"])
@pytest.mark.parametrize("name", ALL)
def test_shape_scene_renders_bitexact(gpu_device, shapes, name, kw, spp):
    s = shapes(name)
    scene, oscene = s["scene"], B.load_oracle(s["path"], name)
    assert scene.state().traceDepth == 4
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
    assert same.all(), (name, kw, spp, int((~same).sum()), np.argwhere(~same)[:3].tolist())
    assert (want > 0).mean() > 0.03                       # (not a comparison of black images)


# ---- the device builder ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL + list(B.BUILDER_CASES))
def test_device_builder_gives_the_host_tree_or_falls_back(gpu_device, tmp_path, name):
    """The device-built tree is the host's, bytes and triangle order.  The build runs on the device
    except where one thread's subtree (a range of at most 128 primitives) needs more than k_bvh_small's
    64 task entries: a chain of more than 63 splits that each leave their right range pending
    (chain63_pos; chain62_pos needs exactly 64).  There error bit 2 is set and the host builds
    (pt_scene.cpp scene_finalize).  The chains the walks see peel a LEFT leaf on their mirrored x
    levels, which leaves nothing pending: even chain_over needs only 2/3 of its depth."""
    path = B.scene_file(tmp_path, name)
    host = B.load(path, name)
    cls = B.classify(host)
    want = B.case_of(name)[2]
    assert {k: cls[k] for k in want} == want, (name, cls)
    need = B.builder_stack(host)
    assert need == {"chain62_pos": 64, "chain63_pos": 65}.get(name, need) and (need <= 64 or host.counts()[2] <= 128)
    dev = B.load(path, name, device_bvh=True)
    assert not host.bvh_build_info()[0]
    assert dev.bvh_build_info()[0] == (need <= 64), (name, cls, need, dev.bvh_build_info())
    assert _tables(dev) == _tables(host)
