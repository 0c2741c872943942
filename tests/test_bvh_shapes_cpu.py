"""Degenerate BVH shapes (tests/bvh_shape_cases.py) judged on the CPU, before any kernel walks them: that
each generator lands in its class, that the stacks the kernels index stay within their bounds, that
pt_scene_bvh_quads hands out a table exactly where the context walks one, and that the oracle's first
hit stands against two yardsticks it does not share code with.

The reference walk is test_bvh_quads_cpu._walk_binary with the reference's own overflow rule
(intersections.cu:202-205: an interior node met with 64 entries on the stack is skipped, its subtree
dropped) in place of that file's assertion that the rule never applies; here it does (chain_over).

Teeth, on the Python side only (measured here, 32 x 24 camera rays):
  * a leaf code that wraps at 256 triangles, (first * 256 + count) >> 8 and & 255 — what the pair and
    quad walks would decode had the layouts been built — picks another triangle than the reference
    walk on 11.1 % (leaf256) and 11.1 % (leaf300) of the pixels (another material on 11.1 % / 10.9 %);
  * a walk without the overflow rule picks another triangle on 10.8 % of chain_over's pixels (another
    material on 9.9 %): the overflow changes FIRST HITS there, not only the stack count (81.9 % of its
    camera rays reach 64 entries; without the rule the stack would reach 70).
"""
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import binding as O

sys.path.insert(0, str(Path(__file__).resolve().parent))
import bvh_shape_cases as B  # noqa: E402
import denoise_ref as R  # noqa: E402
import mesh_ref as M  # noqa: E402
from test_bvh_quads_cpu import _check_structure, _tables, _walk_binary, _walk_quads  # noqa: E402
from test_bvh_shapes_gpu import D, EXCLUDED_CAP, PATHS  # noqa: E402

f32 = np.float32
STRIDE = 3          # the leaf-sequence comparison walks every third camera ray (256 of 768)


def tri_tests(v, o, d, dt=f32):
    """glm::intersectRayTriangle (gtx/intersect.inl:37-74) of every ray (o, d[r]) against every triangle
    v[k], every step in dt, as mesh_ref.mesh_hit_ref writes it: (hit (r, T), t (r, T))."""
    with np.errstate(all="ignore"):
        v = v.astype(dt)
        v0, e1, e2 = v[:, 0], v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
        e1c = tuple(e1[:, k][None, :] for k in range(3))
        e2c = tuple(e2[:, k][None, :] for k in range(3))
        dc = tuple(d[:, k][:, None].astype(dt) for k in range(3))
        sc = tuple(dt(o[k]) - v0[:, k][None, :] for k in range(3))
        q = M._cross(sc, e1c)
        p = M._cross(dc, e2c)
        a = M._dot3(e1c, p)
        f = dt(1) / a
        bx = f * M._dot3(sc, p)
        by = f * M._dot3(dc, q)
        bz = f * M._dot3(e2c, q)
        hit = ~(a < dt(M.FLT_EPSILON)) & ~(bx < 0) & ~(bx > 1) & ~(by < 0) & ~(by + bx > 1) & (bz >= 0)
    return hit, bz


def closest_of(leaves, hit, t):
    """BVHIntersectionTest's update over the leaves in order: the closest triangle's array position,
    the first found on ties (-1: none), and its t."""
    best, bt = -1, f32(0)
    for first, count in leaves:
        for k in range(first, first + count):
            if hit[k] and (best < 0 or t[k] < bt):
                best, bt = k, t[k]
    return best, bt


def wrapped(leaves):
    """The leaves as a code -(first * 256 + count) - 1 decodes them: c >> 8, c & 255."""
    return [((f * 256 + c) >> 8, (f * 256 + c) & 255) for f, c in leaves]


class Case:
    def __init__(self, tmp, name):
        self.name = name
        self.path = B.scene_file(tmp, name)
        self.scene = B.load(self.path, name)
        self.cls = B.classify(self.scene)
        self.pn = B.nodes_of(self.scene)
        self.tris = M.triangle_table(self.scene)
        self.nq, self.root, self.bound = B.quads_of(self.scene)
        cam = self.scene.camera()
        self.o = np.asarray(list(cam.position), f32)
        self.d = R.camera_rays(cam, f32).reshape(-1, 3)
        self.hit, self.t = tri_tests(self.tris["v"], self.o, self.d)
        self._walks, self._refs, self._oracle = {}, {}, None

    def walk(self, overflow, stride=1):
        """(per ray: array position of the closest triangle or -1; the leaves' lists; stats)."""
        key = (overflow, stride)
        if key not in self._walks:
            stats, best, seqs = {"full": 0}, [], []
            for i in range(0, len(self.d), stride):
                st = {}
                leaves = _walk_binary(self.pn, self.o, self.d[i], overflow, st)
                stats["deepest"] = max(stats.get("deepest", 0), st["deepest"])
                stats["full"] += st["deepest"] == 64
                stats["skipped"] = stats.get("skipped", 0) + st["skipped"]
                seqs.append(leaves)
                best.append(closest_of(leaves, self.hit[i], self.t[i])[0])
            self._walks[key] = (np.array(best), seqs, stats)
        return self._walks[key]

    def ref(self, path, dt=np.float64):
        if (path, dt) not in self._refs:
            mode, bbox = PATHS[path]
            self._refs[path, dt] = M.mesh_first_hit_ref(self.tris, self.scene.geoms(), self.scene.camera(), dt, mode,
                                                        use_bbox=bbox)
        return self._refs[path, dt]

    def oracle(self):
        """(material key (H, W), hit mask (H, W)) of the oracle's first hit: test_denoise_gpu.py's route."""
        if self._oracle is None:
            fl = O.flags(ssaa=False, dof=False)
            keys, _ = O.bounce_records(B.load_oracle(self.path, self.name), fl, 1, 0)
            white = B.load_oracle(self.path, self.name)
            for m in white.materials:
                m.color[:] = [1.0, 1.0, 1.0]
                m.emittance = 1.0
            img, _ = O.render_pass(white, fl, 1, depth=1)
            assert set(np.unique(img).tolist()) <= {0.0, 1.0}
            self._oracle = (keys.reshape(B.RES[1], B.RES[0]), img[..., 0] == 1.0)
        return self._oracle

    def mats_of_walk(self, best):
        """The material of every pixel when the mesh's closest triangle is `best` (array positions, -1:
        none): computeIntersections' loop over the geoms in float32 (mesh, cube, sphere)."""
        geoms = self.scene.geoms()
        rr = np.arange(len(best))
        bt = np.full(len(best), np.inf, f32)
        mat = np.full(len(best), -1, np.int32)
        ob = np.broadcast_to(self.o, self.d.shape)
        for g in geoms:
            if g.type == 2:
                tw = np.where(best >= 0, self.t[rr, np.maximum(best, 0)], f32(np.inf))
            else:
                tw = R.geom_hit(g, ob, self.d, f32, 1e-3)[0]
            closer = (tw > 0) & (tw < bt)
            bt = np.where(closer, tw, bt)
            mat = np.where(closer, g.material_id, mat)
        return mat.reshape(B.RES[1], B.RES[0])


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("bvh_shapes_cpu")
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(tmp, name)
        return made[name]
    return get


ALL = list(B.CASES)


@pytest.mark.parametrize("name", ALL)
def test_generator_lands_in_its_class(cases, name):
    c = cases(name)
    want = B.CASES[name][2]
    print(name, c.cls, "quads", (c.nq, c.bound))
    assert {k: c.cls[k] for k in want} == want, c.cls
    assert c.cls["height"] == (0 if c.cls["root_leaf"] else c.cls["depth"] + 1)
    if name.startswith("leaf"):
        # leaves before and after the big one in triangle order: a wrapped code lands in their triangles
        assert c.cls["big_first"] > 0 and c.cls["leaves_after"] >= 8
    if name == "chain_over":
        assert c.cls["depth"] >= 66
    # the oracle's tree is this tree, and every triangle arrived (their ids are a permutation)
    osc = B.load_oracle(c.path, name)
    assert osc.nodes.tobytes() == c.pn.tobytes() and osc.tris.tobytes() == c.tris.tobytes()
    assert sorted(c.tris["id"].tolist()) == list(range(len(B.CASES[name][0]())))
    assert np.isfinite(c.pn["bmin"]).all() and np.isfinite(c.pn["bmax"]).all()


@pytest.mark.parametrize("name,need", [("chain62", None), ("chain63", None), ("chain_over", None), ("chain62_pos", 64),
                                       ("chain63_pos", 65)])
def test_builder_cases_need_the_task_stack_they_name(cases, name, need):
    """k_bvh_small's 64 task entries: the chains the walks see stay far below (their mirrored x levels
    peel a left leaf and leave nothing pending); the +x chains sit at the limit and one past it."""
    c = cases(name)
    want = B.case_of(name)[2]
    assert {k: c.cls[k] for k in want} == want, c.cls
    print(name, "builder stack", B.builder_stack(c.scene))
    got = B.builder_stack(c.scene)
    assert (got == need if need else got <= 2 * (c.cls["depth"] + 1) // 3 + 3 <= 64) and len(c.tris) <= 128


@pytest.mark.parametrize("name", ALL)
def test_accessor_hands_out_quads_exactly_where_the_context_walks_them(cases, name):
    """pt_create builds the pair and quad layouts only when every leaf fits the leaf code (<= 255
    triangles, first < 2^23), and the quad layout only within the stack's capacity; make_quads refuses
    the same trees, so pt_scene_bvh_quads returns 0 for them (it used to return a table whose big leaf's
    code had wrapped)."""
    c = cases(name)
    assert (c.nq > 0) == B.CASES[name][3], (name, c.nq)
    assert (c.nq > 0) == (c.cls["big_leaves"] == 0 and c.cls["depth"] + 1 <= 64)
    if c.cls["root_leaf"]:
        assert c.nq == 1 and c.root == -(c.pn[0]["first_area_idx"] * 256 + c.pn[0]["sub_areas"]) - 1 and c.bound == 0


@pytest.mark.parametrize("name", ALL)
def test_stacks_stay_within_what_the_kernels_index(cases, name):
    """The deepest occupancy of the reference walk is at most 64 (the private arrays), at most depth + 1
    (LdsStack's 32 rows below depth 32), and the quad walk's at most its bound (_walk_quads asserts it);
    both walks reach the same leaves in the same order, and the table passes _check_structure."""
    c = cases(name)
    _, seqs, stats = c.walk("reference", STRIDE)
    print(f"{name}: deepest stack {stats['deepest']} (depth {c.cls['depth']}), rays at 64 entries {stats['full']}, "
          f"skipped nodes {stats['skipped']}, quad bound {c.bound if c.nq else None}")
    assert stats["deepest"] <= 64
    if name != "chain_over":
        assert stats["deepest"] <= c.cls["depth"] + 1 and stats["skipped"] == 0
    if name.startswith("chain"):    # the camera does fill the stack: one entry per level, down to the boxes of
        assert stats["deepest"] >= min(c.cls["depth"] - 2, 64)   # the few smallest triangles, which few rays meet
    if name == "chain_over":
        assert stats["full"] > 0 and stats["skipped"] > 0
    if not c.nq:
        return
    if c.cls["root_leaf"]:
        for leaves in seqs:
            assert leaves in ([], [(int(c.pn[0]["first_area_idx"]), int(c.pn[0]["sub_areas"]))])
        return
    pn, Q, root, bound = _tables(c.scene)
    _check_structure(pn, Q, root, bound)
    deepest = 0
    for k, i in enumerate(range(0, len(c.d), STRIDE)):
        got, dq = _walk_quads(pn, Q, root, c.o, c.d[i], bound)
        deepest = max(deepest, dq)
        assert got == seqs[k], f"ray {i}: leaf sequences differ"
    print(f"{name}: deepest quad stack {deepest} of bound {bound}")


@pytest.mark.parametrize("name", ALL)
def test_oracle_first_hit_against_independent_yardsticks(cases, name):
    """Every case but chain_over: the float64 brute force over all triangles, on its kept pixels.
    chain_over: the Python walk with the overflow rule in float32 (the brute force sees the triangles
    the overflow drops); pixels the float64 side calls risky are left out there too."""
    c = cases(name)
    keys, hit = c.oracle()
    ref = c.ref("bvh")
    keep = ref["keep"]
    if name == "chain_over":
        best, _, _ = c.walk("reference")
        want = c.mats_of_walk(best)
    else:
        want = ref["mat"]
    assert np.array_equal(hit[keep], (want >= 0)[keep])
    k = keep & hit
    assert np.array_equal(keys[k], want[k])
    assert len(np.unique(want[keep])) == 3      # background, mesh and sphere are in view (the light is behind the camera)


@pytest.mark.parametrize("name", ALL)
def test_python_walk_picks_the_float64_triangle(cases, name):
    """The yardstick of the teeth below is itself right: on the kept pixels the float32 walk picks the
    brute force's triangle (chain_over: where the overflow drops nothing, and only there)."""
    c = cases(name)
    ref = c.ref("bvh")
    stride = 1 if name in ("leaf256", "leaf300", "chain_over") else STRIDE
    best, _, _ = c.walk("reference", stride)
    ids = np.where(best >= 0, c.tris["id"][np.maximum(best, 0)], -1)
    keep = ref["keep"].reshape(-1)[::stride]
    want = ref["tri"].reshape(-1)[::stride]
    prim = (ref["tri"] < 0).reshape(-1)[::stride] & (ref["mat"] >= 0).reshape(-1)[::stride]   # a cube or sphere is nearer
    differ = keep & ~prim & (ids != want)
    if name == "chain_over":
        free = c.walk("none")[0]
        assert np.array_equal(differ, keep & ~prim & (free != best)) and differ.any()
    else:
        assert not differ.any(), (name, int(differ.sum()))


@pytest.mark.parametrize("name", ["leaf256", "leaf300"])
def test_teeth_a_wrapped_leaf_code_picks_other_triangles(cases, name):
    c = cases(name)
    best, seqs, _ = c.walk("reference")
    other = np.array([closest_of(wrapped(seqs[i]), c.hit[i], c.t[i])[0] for i in range(len(seqs))])
    share = (other != best).mean()
    print(f"{name}: a wrapped leaf code picks another triangle on {100 * share:.1f} % of the pixels")
    assert (other != best).sum() > 0
    lost = c.mats_of_walk(other) != c.mats_of_walk(best)
    print(f"{name}: and another material on {100 * lost.mean():.1f} %")


def test_teeth_a_walk_without_the_overflow_rule_picks_other_triangles(cases):
    c = cases("chain_over")
    best, _, stats = c.walk("reference")
    free, _, fstats = c.walk("none")
    share = (free != best).mean()
    print(f"chain_over: {100 * stats['full'] / len(best):.1f} % of the rays reach 64 entries; without the rule the stack "
          f"reaches {fstats['deepest']} and {100 * share:.1f} % of the pixels show another triangle")
    assert stats["full"] > 0 and (free != best).sum() > 0 and fstats["deepest"] > 64
    assert ((free >= 0) & (best < 0)).sum() > 0        # the rule hides triangles: the deepest, smallest ones
    mats = c.mats_of_walk(free) != c.mats_of_walk(best)
    print(f"chain_over: and another material on {100 * mats.mean():.1f} %")


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", [n for n in ALL if n != "chain_over"])
def test_excluded_share_and_float32s_own_error(cases, name, path):
    """The float64 side alone excludes at most 5 % of a case's pixels, and float32's own error (the same
    evaluation in float32, mesh_ref.deviations) stays at or below test_bvh_shapes_gpu.py's table D."""
    c = cases(name)
    ref = c.ref(path)
    excluded = 1.0 - ref["keep"].mean()
    dev = M.deviations(ref, c.ref(path, np.float32))
    print(f"{name} {path}: excluded {100 * excluded:.2f} %  " + "  ".join(
        f"{kind}: D_t={dev[kind][0]:.2e} D_p={dev[kind][1]:.2e} D_n={dev[kind][2]:.2e} D_uv={dev[kind][3]:.2e}"
        for kind in ("tri", "prim")))
    assert excluded <= EXCLUDED_CAP
    for kind in ("tri", "prim"):
        for what, got, d in zip(("t", "P", "n", "uv"), dev[kind], D[name, path][kind]):
            assert got <= d, (name, path, kind, what, got, d)
    mesh = ref["keep"] & (ref["tri"] >= 0)
    assert mesh.mean() >= 0.04 and len(np.unique(ref["tri"][mesh])) >= min(5, len(c.tris))
