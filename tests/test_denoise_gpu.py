"""First-hit G-buffer (pt_gbuffer) and the edge-avoiding a-trous denoiser (pt_denoise.hip) on the GPU.

The filter is compared bit for bit with the numpy float32 restatement of DESIGN.md §10
(tests/denoise_ref.py); the G-buffer's material ids, hit mask and albedo exactly with the oracle and the
scene's tables; its normals, distances and positions with a float64 restatement of the reference's
sphere and cube tests, within 8x the error the same restatement shows when evaluated in float32.

Measured on the CPU (float32 restatement against float64, kept pixels; tests/denoise_ref.py deviations):
    sphere.json, 40x30, camera moved in:   D_n = 2.76e-5   D_t = 4.40e-6   D_p = 3.98e-6
    three_body_scene, 40x30:               D_n = 3.99e-5   D_t = 4.45e-6   D_p = 4.40e-6
    inside_scene (sphere shell), 40x30:    D_n = 3.53e-5   D_t = 4.93e-6   D_p = 4.59e-6
    inside_scene (cube shell), 40x30:      D_n = 3.53e-5   D_t = 4.93e-6   D_p = 4.59e-6
(the 1e-4 back-off of getPointOnRay is subtracted from an object-space parameter of order 10, and the
normal of a stretched sphere comes from that point: a few ulp of 10 through the inverse-transpose.)
The constants below are those, rounded up; the GPU may deviate by 8x them.
"""
import ctypes as C
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import cuda_pathtracer_amd as P
from cuda_pathtracer_amd import _native as N
from oracle import binding as O

sys.path.insert(0, str(Path(__file__).resolve().parent))
import denoise_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
SCENES = ROOT / "tests" / "scenes"
F = np.float32
PT_ERR_ARG = 1

D_N = {"sphere": 2.8e-5, "three": 4.0e-5, "inside_sphere": 3.6e-5, "inside_cube": 3.6e-5}
D_T = {"sphere": 4.5e-6, "three": 4.5e-6, "inside_sphere": 5.0e-6, "inside_cube": 5.0e-6}
D_P = {"sphere": 4.0e-6, "three": 4.5e-6, "inside_sphere": 4.6e-6, "inside_cube": 4.6e-6}


# ---- the filter, bit for bit ------------------------------------------------------------------------
def _synthetic(w, h, seed):
    """Guides on 4 planes (noisy unit normals, positions on the planes), ~10% misses, colours in [0, 4)
    with exact zeros, subnormals and one 1e30 firefly, albedo components on both sides of 2^-10."""
    rng = np.random.default_rng(seed)
    planes_n = np.array([[0, 0, 1], [0, 1, 0], [0.6, 0, 0.8], [-0.48, 0.6, 0.64]], np.float64)
    pid = rng.integers(0, 4, (h, w))
    if w * h > 64:   # blocks of one plane, so that the filter has neighbours to mix
        yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        pid = ((xx // 9) + 2 * (yy // 7)) % 4
    n = planes_n[pid] + rng.normal(0, 0.02, (h, w, 3))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    pos = np.stack([xx * 0.1, yy * 0.1, np.zeros_like(xx)], -1)
    pn = planes_n[pid]
    pos -= pn * (np.sum(pos * pn, -1, keepdims=True) - pid[..., None])   # onto the plane n.x = pid
    mat = rng.integers(0, 5, (h, w)).astype(np.int32)
    mat[rng.random((h, w)) < 0.1] = -1
    gA = np.zeros((h, w, 4), F)
    gA[..., :3] = n
    gA[..., 3] = mat.view(F)
    gB = np.zeros((h, w, 4), F)
    gB[..., :3] = pos
    gB[..., 3] = np.where(mat < 0, -1, 5).astype(F)
    rgb = (rng.random((h, w, 3)) * 4).astype(F)
    flat = rgb.reshape(-1)
    k = flat.size
    flat[rng.integers(0, k, max(1, k // 20))] = 0.0
    flat[rng.integers(0, k, max(1, k // 50))] = F(1e-41)          # subnormal
    flat[rng.integers(0, k, 1)] = F(3e-39)
    if k > 3:
        flat[rng.integers(0, k)] = F(1e30)                        # firefly
    alb = np.zeros((h, w, 4), F)
    alb[..., :3] = (rng.random((h, w, 3)) * 0.9 + 0.05).astype(F)
    af = alb[..., :3].reshape(-1).copy()
    af[rng.integers(0, k, max(1, k // 10))] = F(2.0 ** -11)       # below 2^-10: left alone
    af[rng.integers(0, k, max(1, k // 10))] = 0.0
    af[rng.integers(0, k, max(1, k // 10))] = F(2.0 ** -10)       # exactly the threshold: modulated
    alb[..., :3] = af.reshape(h, w, 3)
    return rgb, gA, gB, alb


def _prm(levels, demodulate, sc=0.5, sn=0.1, sp=0.05):
    p = N.DenoiseParams.default()
    p.levels, p.demodulate, p.sigma_c, p.sigma_n, p.sigma_p = levels, demodulate, sc, sn, sp
    return p


def _host(rgb, samples, gA, gB, alb, prm):
    h, w = rgb.shape[:2]
    out = np.empty((h, w, 3), F)
    rc = P.lib().pt_denoise_host(w, h, rgb.ctypes.data, samples, gA.ctypes.data, gB.ctypes.data, alb.ctypes.data,
                                 C.byref(prm), out.ctypes.data)
    assert rc == 0, P.lib().pt_last_error()
    return out


SHAPES = [(1, 1), (1, 70), (70, 1), (37, 29), (64, 64), (130, 67)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_filter_equals_the_restatement_bitwise(gpu_device, shape):
    w, h = shape
    rgb, gA, gB, alb = _synthetic(w, h, 1000 + 7 * w + h)
    samples = 3.0
    for levels in (0, 1, 3, 5):
        for demod in (0, 1):
            got = _host(rgb, samples, gA, gB, alb, _prm(levels, demod))
            want = R.atrous_ref(rgb, samples, gA, gB, alb, levels, 0.5, 0.1, 0.05, bool(demod))
            bad = got.view(np.uint32) != want.view(np.uint32)
            assert not bad.any(), (shape, levels, demod, int(bad.sum()), np.argwhere(bad)[:4].tolist(),
                                   got[bad][:4], want[bad][:4])


def test_denoiser_run_on_device_buffers_matches_host_and_repeats(gpu_device):
    import torch
    w, h = 130, 67
    rgb, gA, gB, alb = _synthetic(w, h, 77)
    prm = _prm(5, 1)
    want = _host(rgb, 2.0, gA, gB, alb, prm)
    t = [torch.from_numpy(a).to(gpu_device) for a in (rgb, gA, gB, alb)]
    outs = [torch.empty((h, w, 3), dtype=torch.float32, device=gpu_device) for _ in range(2)]
    L = P.lib()
    dn = C.c_void_p()
    assert L.pt_denoiser_create(w, h, C.byref(dn)) == 0
    try:
        st = torch.cuda.current_stream().cuda_stream
        for o in outs:
            rc = L.pt_denoiser_run(dn, t[0].data_ptr(), 2.0, t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(),
                                   C.byref(prm), o.data_ptr(), st)
            assert rc == 0, L.pt_last_error()
        assert L.pt_denoiser_run(dn, t[0].data_ptr(), 2.0, t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(),
                                 C.byref(prm), t[0].data_ptr(), st) == PT_ERR_ARG      # aliased output
        torch.cuda.synchronize()
        a, b = (o.cpu().numpy() for o in outs)
    finally:
        L.pt_denoiser_destroy(dn)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(a.view(np.uint32), want.view(np.uint32))


# ---- G-buffer: ids, hit mask, albedo (exact) -----------------------------------------------------------
def _scene_file(tmp, name, **camera):
    spec = json.loads((SCENES / f"{name}.json").read_text())
    spec["Camera"].update(camera)
    d = tmp / name
    d.mkdir()
    (d / "Textures").symlink_to(SCENES / "Textures")
    (d / "Models").symlink_to(SCENES / "Models")
    path = d / f"{name}.json"
    path.write_text(json.dumps(spec))
    return str(path)


@pytest.fixture(scope="module")
def gbuffers(tmp_path_factory, gpu_device):
    """name -> (scene, gbuffer dict, oracle material keys (H, W), oracle hit mask (H, W)); computed once."""
    tmp = tmp_path_factory.mktemp("gbuf")
    out = {}
    for name, res in (("cornell", [64, 48]), ("sphere", [48, 48]), ("room", [48, 48])):
        path = _scene_file(tmp, name, RES=res)
        scene = P.Scene(path)
        pt = P.PathTracer(scene)
        g = pt.gbuffer()
        pt.free()
        fl = O.flags(ssaa=False, dof=False)
        sc = O.OracleScene.from_json(path)
        keys, _ = O.bounce_records(sc, fl, 1, 0)
        white = O.OracleScene.from_json(path)
        for m in white.materials:
            m.color[:] = [1.0, 1.0, 1.0]
            m.emittance = 1.0
        img, _ = O.render_pass(white, fl, 1, depth=1)
        assert set(np.unique(img).tolist()) <= {0.0, 1.0}
        out[name] = (scene, g, keys.reshape(res[1], res[0]), img[..., 0] == 1.0, path)
    return out


@pytest.mark.parametrize("name", ["cornell", "sphere", "room"])
def test_gbuffer_ids_and_hit_mask_equal_the_oracle(gbuffers, name):
    scene, g, keys, hit, _ = gbuffers[name]
    assert g["mat"].dtype == np.int32 and g["mat"].shape == hit.shape
    assert np.array_equal(g["mat"] >= 0, hit)
    assert np.array_equal(g["t"] > 0, hit)
    assert np.array_equal(g["mat"][hit], keys[hit])
    if name == "sphere":   # (the other two are closed rooms)
        assert (~hit).any()
    miss = ~hit
    assert (g["mat"][miss] == -1).all() and (g["t"][miss] == -1).all()
    for k in ("normal", "position", "uv"):
        assert not g[k][miss].any(), k
    assert (g["albedo"][miss] == 1).all()
    nn = np.linalg.norm(g["normal"][hit].astype(np.float64), axis=-1)
    assert np.abs(nn - 1).max() < 1e-5


def test_gbuffer_tiles_of_two_ranks_interleave_bitwise(gbuffers):
    scene, g, _, _, _ = gbuffers["cornell"]
    for rank in (0, 1):
        pt = P.PathTracer(scene, rank=rank, world=2, spp=2)
        t = pt.gbuffer()
        pt.free()
        for k, v in g.items():
            assert t[k].tobytes() == np.ascontiguousarray(v[rank::2]).tobytes(), (rank, k)


def _expected_albedo(scene, g, single):
    mats = scene.materials()
    want = np.ones(g["mat"].shape + (3,), F)
    for mid, m in enumerate(mats):
        sel = g["mat"] == mid
        if not sel.any() or m.emittance > 0:
            continue
        col = np.array(m.color[:], F)
        if m.texture_id != -1:
            w, h, comps, data = O.load_texture(scene.texture_path(m.texture_id))
            assert comps == 3
            toc = R.tex_color_ref(data.reshape(h, w, 3), g["uv"][sel][:, 0], g["uv"][sel][:, 1])
        else:
            toc = np.broadcast_to(col, (int(sel.sum()), 3))
        want[sel] = toc if single else (toc * col).astype(F)
    return want


@pytest.mark.parametrize("name", ["cornell", "sphere", "room"])
def test_gbuffer_albedo_is_exact(gbuffers, name):
    scene, g, _, _, _ = gbuffers[name]
    want = _expected_albedo(scene, g, single=False)
    assert np.array_equal(g["albedo"].view(np.uint32), want.view(np.uint32))
    if name == "room":
        tex = [i for i, m in enumerate(scene.materials()) if m.texture_id != -1]
        assert tex and all((g["mat"] == i).any() for i in tex)      # both textured materials are in view
    gui = P.GuiDataContainer()
    gui.singleAlbedo = True
    pt = P.PathTracer(scene, gui)
    g1 = pt.gbuffer()
    pt.free()
    assert np.array_equal(g1["mat"], g["mat"]) and g1["uv"].tobytes() == g["uv"].tobytes()
    want1 = _expected_albedo(scene, g1, single=True)
    assert np.array_equal(g1["albedo"].view(np.uint32), want1.view(np.uint32))


# ---- G-buffer: normals, t, P against float64 ---------------------------------------------------------------
def _geometry_scene(tmp_path, which):
    if which == "sphere":   # the bundled scene, its camera moved in so that the sphere fills a fifth of the frame
        return P.Scene(_scene_file(tmp_path, "sphere", RES=[40, 30], FOVY=14.0, EYE=[1.0, 4.0, 10.5],
                                   LOOKAT=[0.3, 0.4, 0.0]))
    if which.startswith("inside"):   # the camera within the shell: the outside = false branches of both tests
        return R.inside_scene(P, P.SPHERE if which == "inside_sphere" else P.CUBE)
    return R.three_body_scene(P)


@pytest.mark.parametrize("which", ["sphere", "three", "inside_sphere", "inside_cube"])
def test_gbuffer_geometry_within_8x_of_float32s_own_error(tmp_path, gpu_device, which):
    scene = _geometry_scene(tmp_path, which)
    ref = R.first_hit_ref(scene.geoms(), scene.camera(), np.float64)
    ref32 = R.first_hit_ref(scene.geoms(), scene.camera(), np.float32)
    keep = ref["keep"]
    assert 1.0 - keep.mean() <= 0.05                      # (float64 side alone)
    if which.startswith("inside"):                        # closed: the shell (material 1) behind everything
        assert (ref["mat"] >= 0).all() and (ref["mat"] == 1).mean() > 0.5 and len(np.unique(ref["mat"])) == 3
    else:
        assert (ref["mat"] >= 0).mean() > 0.1 and (ref["mat"] < 0).any()
    d_n, d_t, d_p = R.deviations(ref, ref32)
    print(f"{which}: D_n={d_n:.3e} D_t={d_t:.3e} D_p={d_p:.3e} excluded={1 - keep.mean():.4f}")
    assert d_n <= D_N[which] and d_t <= D_T[which] and d_p <= D_P[which]
    pt = P.PathTracer(scene)
    g = pt.gbuffer()
    pt.free()
    assert np.array_equal(g["mat"][keep], ref["mat"][keep])
    k = keep & (ref["mat"] >= 0)
    scale = np.maximum(1.0, ref["t"][k])
    e_n = np.abs(g["normal"][k].astype(np.float64) - ref["n"][k]).max()
    e_t = (np.abs(g["t"][k].astype(np.float64) - ref["t"][k]) / scale).max()
    e_p = (np.abs(g["position"][k].astype(np.float64) - ref["P"][k]) / scale[:, None]).max()
    print(f"{which}: GPU e_n={e_n:.3e} e_t={e_t:.3e} e_p={e_p:.3e}")
    assert e_n <= 8 * D_N[which] and e_t <= 8 * D_T[which] and e_p <= 8 * D_P[which]


# ---- pt_denoise_image ------------------------------------------------------------------------------------
def test_denoise_image_is_host_filter_of_image_and_gbuffer(tmp_path, gpu_device):
    scene = P.Scene(_scene_file(tmp_path, "cornell", RES=[64, 64]))
    pt = P.PathTracer(scene)
    for it in range(1, 5):
        pt.render_pass(it)
    before = pt.image()
    got = pt.denoised(4.0)
    assert got.shape == (64, 64, 3) and got.dtype == np.float32
    assert pt.image().tobytes() == before.tobytes()       # the accumulator is untouched
    want = P.denoise(before, 4.0, pt.gbuffer())
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert not np.array_equal(got, before / F(4.0))
    pt.free()
    pt2 = P.PathTracer(scene, rank=0, world=2)
    prm = N.DenoiseParams.default()
    out = np.empty((32, 64, 3), F)
    assert P.lib().pt_denoise_image(pt2._h, 1.0, C.byref(prm), out.ctypes.data) == PT_ERR_ARG
    with pytest.raises(P.PtError):
        pt2.denoised(1.0)
    pt2.free()


# ---- quality -------------------------------------------------------------------------------------------
def test_denoised_16spp_is_closer_to_1024spp_than_raw_16spp(tmp_path, gpu_device):
    scene = P.Scene(_scene_file(tmp_path, "cornell", RES=[200, 200]))
    pt = P.PathTracer(scene)
    for it in range(1, 17):
        pt.render_pass(it)
    raw16 = pt.image() / F(16)
    dn16 = pt.denoised(16.0)
    for it in range(17, 1025):
        pt.render_pass(it)
    ref = pt.image() / F(1024)
    pt.free()

    def rmse(a):
        return float(np.sqrt(np.mean((np.clip(a, 0, 1).astype(np.float64) - np.clip(ref, 0, 1)) ** 2)))

    r_raw, r_dn = rmse(raw16), rmse(dn16)
    print(f"RMSE raw16={r_raw:.5f} denoised16={r_dn:.5f} ratio={r_dn / r_raw:.3f}")
    assert r_dn < r_raw


# ---- CLI -------------------------------------------------------------------------------------------------
def test_cli_denoise_and_aov(tmp_path):
    exe = ROOT / "cuda_pathtracer_amd" / "pathtracer_amd"
    scene = str(SCENES / "sphere.json")
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir()
    b.mkdir()
    base = [str(exe), scene, "--iterations", "2", "--out"]
    r0 = subprocess.run(["timeout", "-k", "10", "120", *base, str(a)], capture_output=True, text=True)
    assert r0.returncode == 0, r0.stdout + r0.stderr
    r1 = subprocess.run(["timeout", "-k", "10", "120", *base, str(b), "--denoise", "--aov", str(b)],
                        capture_output=True, text=True)
    assert r1.returncode == 0, r1.stdout + r1.stderr
    raw_a = [p for p in a.glob("sphere.*.2samp.png")]
    raw_b = [p for p in b.glob("sphere.*.2samp.png") if not p.name.endswith(".denoised.png")]
    assert len(raw_a) == 1 and len(raw_b) == 1
    assert raw_a[0].read_bytes() == raw_b[0].read_bytes()
    dn = list(b.glob("sphere.*.2samp.denoised.png"))
    assert len(dn) == 1 and dn[0].stat().st_size > 0
    from PIL import Image
    assert Image.open(dn[0]).size == Image.open(raw_b[0]).size
    side = json.loads((b / "sphere.aov.json").read_text())
    assert side["dtype"] == "<f4" and sorted(side["planes"]) == ["albedo", "gA", "gB", "uv"]
    files = sorted(b.glob("*.f32"))
    assert len(files) == 4
    for name, pl in side["planes"].items():
        f = b / pl["file"]
        assert f.stat().st_size == 4 * int(np.prod(pl["shape"])), name
    gA = np.fromfile(b / side["planes"]["gA"]["file"], "<f4").reshape(side["planes"]["gA"]["shape"])
    mat = gA[..., 3].copy().view(np.int32)
    assert (mat == -1).any() and (mat == 0).any()
