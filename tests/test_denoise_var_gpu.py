"""Per-pixel luminance moments (pt_moments), the variance-guided a-trous filter (pt_denoiser_run_var) and
the context's variance tracking on the GPU.  Everything is compared bit for bit with the numpy float32
restatement of DESIGN.md §11 (tests/denoise_var_ref.py); the quality test only asserts that the filter
at 16 spp is closer to 1024 spp than the raw image, and prints the rest."""
import ctypes as C
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import cuda_pathtracer_amd as P
from cuda_pathtracer_amd import _native as N

sys.path.insert(0, str(Path(__file__).resolve().parent))
import denoise_var_ref as RV  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
SCENES = ROOT / "tests" / "scenes"
F = np.float32
PT_ERR_ARG = 1
SHAPES = [(1, 1), (1, 70), (70, 1), (37, 29), (64, 64), (130, 67)]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(got, want, what):
    bad = _bits(got) != _bits(want)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4], want[bad][:4])


# ---- moments ----------------------------------------------------------------------------------------
def _albedo(h, w, rng):
    """Components on both sides of 2^-10 (and exactly on it)."""
    alb = np.zeros((h, w, 4), F)
    a = (rng.random(h * w * 3) * 0.9 + 0.05).astype(F)
    k = a.size
    a[rng.integers(0, k, max(1, k // 10))] = F(2.0 ** -11)
    a[rng.integers(0, k, max(1, k // 10))] = 0.0
    a[rng.integers(0, k, max(1, k // 10))] = F(2.0 ** -10)
    alb[..., :3] = a.reshape(h, w, 3)
    return alb


def _accumulators(h, w, rng, n, bs):
    """n + 1 accumulator snapshots: growing sums with pixels that gain exactly nothing in a batch, that
    gain a subnormal, and one 1e15 firefly (l * l stays finite)."""
    acc = [(rng.random((h, w, 3)) * 2).astype(F)]
    for b in range(n):
        gain = (rng.random((h, w, 3)) * bs).astype(F)
        flat = gain.reshape(-1)
        k = flat.size
        flat[rng.integers(0, k, max(1, k // 8))] = 0.0
        nxt = (acc[-1] + gain).astype(F)
        nf = nxt.reshape(-1)
        nf[rng.integers(0, k, max(1, k // 16))] = F(1e-41)       # (a subnormal accumulator value)
        if b == 2:
            nf[rng.integers(0, k)] = F(1e15)
        acc.append(nxt)
    return acc


class _Mom:
    def __init__(self, w, h):
        self.L, self.w, self.h = P.lib(), w, h
        self.m = C.c_void_p()
        N.check_pt(self.L.pt_moments_create(w, h, C.byref(self.m)))

    def close(self):
        self.L.pt_moments_destroy(self.m)

    def get(self):
        m1, m2 = np.empty((self.h, self.w), F), np.empty((self.h, self.w), F)
        prev = np.empty((self.h, self.w, 3), F)
        N.check_pt(self.L.pt_moments_get(self.m, m1.ctypes.data, m2.ctypes.data, prev.ctypes.data))
        return m1, m2, prev


@pytest.mark.parametrize("use_alb", [False, True], ids=["plain", "albedo"])
@pytest.mark.parametrize("bs", [1.0, 4.0])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_moments_equal_the_restatement_bitwise(gpu_device, shape, bs, use_alb):
    import torch
    w, h = shape
    rng = np.random.default_rng(500 + 7 * w + h + int(bs))
    acc = _accumulators(h, w, rng, 5, bs)
    alb = _albedo(h, w, rng) if use_alb else None
    d_alb = torch.from_numpy(alb).to(gpu_device) if use_alb else None
    d_acc = [torch.from_numpy(a).to(gpu_device) for a in acc]
    st = torch.cuda.current_stream().cuda_stream
    mom = _Mom(w, h)
    try:
        for with_base in (True, False):
            N.check_pt(mom.L.pt_moments_reset(mom.m, d_acc[0].data_ptr() if with_base else None, st))
            ref = RV.Moments(h, w, acc[0] if with_base else None)
            m1, m2, prev = mom.get()
            assert not m1.any() and not m2.any()
            _same(prev, ref.prev, ("reset", with_base))
            for b in range(1, 6):
                N.check_pt(mom.L.pt_moments_update(mom.m, d_acc[b].data_ptr(), bs,
                                                   d_alb.data_ptr() if use_alb else None, st))
                ref.update(acc[b], bs, alb)
            n, got_bs = C.c_int32(), C.c_float()
            N.check_pt(mom.L.pt_moments_info(mom.m, C.byref(n), C.byref(got_bs)))
            assert (n.value, got_bs.value) == (5, bs)
            m1, m2, prev = mom.get()
            _same(m1, ref.m1, ("m1", with_base))
            _same(m2, ref.m2, ("m2", with_base))
            _same(prev, ref.prev, ("prev", with_base))
            assert np.isfinite(m2).all()
            d_var = torch.empty((h, w), dtype=torch.float32, device=gpu_device)
            N.check_pt(mom.L.pt_moments_variance(mom.m, 5 * bs, d_var.data_ptr(), st))
            torch.cuda.synchronize()
            _same(d_var.cpu().numpy(), ref.variance(5 * bs), ("variance", with_base))
            # a changed batch size is refused, and the object goes on as it was
            assert mom.L.pt_moments_update(mom.m, d_acc[5].data_ptr(), bs + 1.0, None, st) == PT_ERR_ARG
            N.check_pt(mom.L.pt_moments_info(mom.m, C.byref(n), None))
            assert n.value == 5
    finally:
        mom.close()


def test_moments_unaligned_accumulator_takes_the_one_pixel_path_with_the_same_bits(gpu_device):
    import torch
    w, h = 37, 29
    rng = np.random.default_rng(9)
    acc = _accumulators(h, w, rng, 2, 1.0)
    alb = _albedo(h, w, rng)
    d_alb = torch.from_numpy(alb).to(gpu_device)
    st = torch.cuda.current_stream().cuda_stream
    mom = _Mom(w, h)
    try:
        ref = RV.Moments(h, w)
        for b in (1, 2):
            buf = torch.zeros(h * w * 3 + 1, dtype=torch.float32, device=gpu_device)
            buf[1:] = torch.from_numpy(acc[b].reshape(-1)).to(gpu_device)
            assert buf[1:].data_ptr() % 16 == 4
            N.check_pt(mom.L.pt_moments_update(mom.m, buf[1:].data_ptr(), 1.0, d_alb.data_ptr(), st))
            ref.update(acc[b], 1.0, alb)
        m1, m2, prev = mom.get()
        _same(m1, ref.m1, "m1")
        _same(m2, ref.m2, "m2")
        _same(prev, ref.prev, "prev")
    finally:
        mom.close()


# ---- the filter, bit for bit ----------------------------------------------------------------------------
def _synthetic(w, h, seed):
    """tests/test_denoise_gpu.py's planes (guides on 4 planes, ~10% misses, colours in [0, 4) with zeros and
    subnormals, albedo on both sides of 2^-10) without its 1e30 colour, plus a variance plane of zeros,
    subnormals, ordinary values and 1e30."""
    rng = np.random.default_rng(seed)
    planes_n = np.array([[0, 0, 1], [0, 1, 0], [0.6, 0, 0.8], [-0.48, 0.6, 0.64]], np.float64)
    pid = rng.integers(0, 4, (h, w))
    if w * h > 64:
        yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        pid = ((xx // 9) + 2 * (yy // 7)) % 4
    n = planes_n[pid] + rng.normal(0, 0.02, (h, w, 3))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    pos = np.stack([xx * 0.1, yy * 0.1, np.zeros_like(xx)], -1)
    pn = planes_n[pid]
    pos -= pn * (np.sum(pos * pn, -1, keepdims=True) - pid[..., None])
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
    flat[rng.integers(0, k, max(1, k // 50))] = F(1e-41)
    alb = _albedo(h, w, rng)
    var = (rng.random((h, w)) ** 4 * 0.5).astype(F)
    vf = var.reshape(-1)
    kv = vf.size
    vf[rng.integers(0, kv, max(1, kv // 6))] = 0.0
    vf[rng.integers(0, kv, max(1, kv // 20))] = F(1e-41)
    vf[rng.integers(0, kv, max(1, kv // 20))] = F(1e30)
    return rgb, var, gA, gB, alb


def _prm(levels, demodulate, sl=1.5, sn=0.1, sp=0.05):
    p = N.DenoiseVarParams.default()
    p.levels, p.demodulate, p.sigma_l, p.sigma_n, p.sigma_p = levels, demodulate, sl, sn, sp
    return p


def _host(rgb, samples, var, gA, gB, alb, prm, want_var=True):
    h, w = rgb.shape[:2]
    out, ov = np.empty((h, w, 3), F), np.empty((h, w), F)
    rc = P.lib().pt_denoise_var_host(w, h, rgb.ctypes.data, samples, var.ctypes.data, gA.ctypes.data, gB.ctypes.data,
                                     alb.ctypes.data, C.byref(prm), out.ctypes.data, ov.ctypes.data if want_var else None)
    assert rc == 0, P.lib().pt_last_error()
    return out, ov


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_filter_equals_the_restatement_bitwise(gpu_device, shape):
    w, h = shape
    rgb, var, gA, gB, alb = _synthetic(w, h, 2000 + 7 * w + h)
    assert np.isfinite(var).all() and np.isfinite(rgb).all()
    samples = 3.0
    for levels in (0, 1, 3, 5):
        for demod in (0, 1):
            got, got_v = _host(rgb, samples, var, gA, gB, alb, _prm(levels, demod))
            want, want_v = RV.atrous_var_ref(rgb, samples, var, gA, gB, alb, levels, 1.5, 0.1, 0.05, bool(demod))
            assert np.isfinite(want).all() and np.isfinite(want_v).all()     # (no NaN is made)
            _same(got, want, (shape, levels, demod, "colour"))
            _same(got_v, want_v, (shape, levels, demod, "variance"))


def test_denoiser_run_var_on_device_buffers_matches_host_and_repeats(gpu_device):
    import torch
    w, h = 130, 67
    rgb, var, gA, gB, alb = _synthetic(w, h, 78)
    prm = _prm(5, 1)
    want, want_v = _host(rgb, 2.0, var, gA, gB, alb, prm)
    no_var, _ = _host(rgb, 2.0, var, gA, gB, alb, prm, want_var=False)          # out_var = NULL
    _same(no_var, want, "without out_var")
    t = [torch.from_numpy(a).to(gpu_device) for a in (rgb, var, gA, gB, alb)]
    outs = [torch.empty((h, w, 3), dtype=torch.float32, device=gpu_device) for _ in range(2)]
    ovs = [torch.empty((h, w), dtype=torch.float32, device=gpu_device) for _ in range(2)]
    L = P.lib()
    dn = C.c_void_p()
    assert L.pt_denoiser_create(w, h, C.byref(dn)) == 0
    try:
        st = torch.cuda.current_stream().cuda_stream
        args = [x.data_ptr() for x in t]
        for o, ov in zip(outs, ovs):
            rc = L.pt_denoiser_run_var(dn, args[0], 2.0, args[1], args[2], args[3], args[4], C.byref(prm), o.data_ptr(),
                                       ov.data_ptr(), st)
            assert rc == 0, L.pt_last_error()
        assert L.pt_denoiser_run_var(dn, args[0], 2.0, args[1], args[2], args[3], args[4], C.byref(prm), args[0],
                                     None, st) == PT_ERR_ARG                     # aliased colour output
        assert L.pt_denoiser_run_var(dn, args[0], 2.0, args[1], args[2], args[3], args[4], C.byref(prm),
                                     outs[0].data_ptr(), args[1], st) == PT_ERR_ARG   # aliased variance output
        torch.cuda.synchronize()
        a, b = (o.cpu().numpy() for o in outs)
        av, bv = (o.cpu().numpy() for o in ovs)
    finally:
        L.pt_denoiser_destroy(dn)
    _same(a, b, "repeat colour")
    _same(av, bv, "repeat variance")
    _same(a, want, "device colour")
    _same(av, want_v, "device variance")


@pytest.mark.parametrize("shape", [(37, 29), (130, 67)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_huge_variance_equals_the_plain_kernel_without_a_colour_term_bitwise(gpu_device, shape):
    """tests/test_denoise_var_cpu.py's huge-variance limit, kernel against kernel: albedo in [0.5, 1] keeps
    the demodulated colours below 8, where both colour terms round 1 + x to exactly 1."""
    w, h = shape
    rgb, _, gA, gB, alb = _synthetic(w, h, 31 + w)
    rng = np.random.default_rng(w)
    alb[..., :3] = (rng.random((h, w, 3)) * 0.5 + 0.5).astype(F)
    var = np.full((h, w), 1e30, F)
    for levels in (1, 3, 5):
        for demod in (0, 1):
            got, _ = _host(rgb, 1.0, var, gA, gB, alb, _prm(levels, demod, sl=1.0, sn=0.3, sp=0.2))
            p = N.DenoiseParams.default()
            p.levels, p.demodulate, p.sigma_c, p.sigma_n, p.sigma_p = levels, demod, 1e6, 0.3, 0.2
            want = np.empty((h, w, 3), F)
            N.check_pt(P.lib().pt_denoise_host(w, h, rgb.ctypes.data, 1.0, gA.ctypes.data, gB.ctypes.data,
                                               alb.ctypes.data, C.byref(p), want.ctypes.data))
            _same(got, want, (shape, levels, demod))


# ---- context ------------------------------------------------------------------------------------------
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


def _alb4(g):
    a = np.zeros(g["albedo"].shape[:2] + (4,), F)
    a[..., :3] = g["albedo"]
    return a


def test_tracking_context_renders_the_same_and_its_variance_is_the_restatements(tmp_path, gpu_device):
    scene = P.Scene(_scene_file(tmp_path, "cornell", RES=[64, 64]))
    plain, pt = P.PathTracer(scene), P.PathTracer(scene)
    assert pt.variance_info() == {"on": False, "batches": 0, "batch_samples": 0.0}
    with pytest.raises(P.PtError):                      # tracking off
        pt.variance_update()
    with pytest.raises(P.PtError):
        pt.variance(1.0)
    with pytest.raises(P.PtError):
        pt.denoised_variance(1.0)
    pt.track_variance(True)
    pt.track_variance(True)                             # (already on: nothing changes)
    snaps = []
    for it in range(1, 7):
        plain.render_pass(it)
        pt.render_pass(it)
        pt.variance_update()
        snaps.append(pt.image())
        assert snaps[-1].tobytes() == plain.image().tobytes(), it
        if it == 1:
            with pytest.raises(P.PtError):              # fewer than 2 batches
                pt.variance(1.0)
            prm = N.DenoiseVarParams.default()
            out = np.empty((64, 64, 3), F)
            assert P.lib().pt_denoise_image_var(pt._h, 1.0, C.byref(prm), out.ctypes.data) == PT_ERR_ARG
    plain.free()
    assert pt.variance_info() == {"on": True, "batches": 6, "batch_samples": 1.0}
    g = pt.gbuffer()
    ref = RV.Moments(64, 64)
    for s in snaps:
        ref.update(s, 1.0, _alb4(g))
    var = pt.variance(6.0)
    assert var.shape == (64, 64) and var.dtype == np.float32
    _same(var, ref.variance(6.0), "variance(6)")
    assert (var > 0).any()
    before = pt.image()
    got = pt.denoised_variance(6.0)
    assert pt.image().tobytes() == before.tobytes()     # the accumulator is untouched
    want = P.denoise_variance(before, 6.0, var, g)
    _same(got, want, "denoised_variance")
    assert not np.array_equal(got, before / F(6.0))
    _same(pt.variance(6.0), var, "variance after the filter")
    # reset_image rebases: the count goes to zero and the next batch is measured from the new accumulator
    pt.reset_image()
    assert pt.variance_info()["batches"] == 0
    ref = RV.Moments(64, 64)
    for it in (1, 2):
        pt.render_pass(it)
        pt.variance_update()
        ref.update(pt.image(), 1.0, _alb4(g))
    _same(pt.variance(2.0), ref.variance(2.0), "variance after reset_image")
    # set_image rebases too: prev becomes the loaded accumulator
    pt.set_image(snaps[3])
    assert pt.variance_info()["batches"] == 0
    ref = RV.Moments(64, 64, snaps[3])
    for it in (5, 6):
        pt.render_pass(it)
        pt.variance_update()
        ref.update(pt.image(), 1.0, _alb4(g))
    assert pt.image().tobytes() == snaps[5].tobytes()
    _same(pt.variance(6.0), ref.variance(6.0), "variance after set_image")
    pt.track_variance(False)
    assert pt.variance_info()["on"] is False
    with pytest.raises(P.PtError):
        pt.variance(6.0)
    pt.free()


def test_batched_context_gives_batches_of_its_spp_and_world_2_is_refused(tmp_path, gpu_device):
    scene = P.Scene(_scene_file(tmp_path, "cornell", RES=[64, 64]))
    pt = P.PathTracer(scene, spp=4)
    pt.track_variance(True)
    snaps = []
    for it in (1, 5, 9):
        pt.render_pass(it)
        pt.variance_update()
        snaps.append(pt.image())
    assert pt.variance_info() == {"on": True, "batches": 3, "batch_samples": 4.0}
    with pytest.raises(P.PtError):                      # another batch size than the first update's
        pt.variance_update(1.0)
    g = pt.gbuffer()
    ref = RV.Moments(64, 64)
    for s in snaps:
        ref.update(s, 4.0, _alb4(g))
    _same(pt.variance(12.0), ref.variance(12.0), "variance(12)")
    ref_plain = RV.Moments(64, 64)                      # demodulate = False: no albedo
    pt.reset_image()
    for it in (1, 5):
        pt.render_pass(it)
        pt.variance_update(demodulate=False)
        ref_plain.update(pt.image(), 4.0)
    _same(pt.variance(8.0), ref_plain.variance(8.0), "variance(8), not demodulated")
    pt.free()
    pt2 = P.PathTracer(scene, rank=0, world=2)
    assert P.lib().pt_track_variance(pt2._h, 1) == PT_ERR_ARG
    with pytest.raises(P.PtError):
        pt2.track_variance(True)
    prm = N.DenoiseVarParams.default()
    out = np.empty((32, 64, 3), F)
    assert P.lib().pt_denoise_image_var(pt2._h, 1.0, C.byref(prm), out.ctypes.data) == PT_ERR_ARG
    pt2.free()


def test_render_denoise_variance_saves_beside_the_same_raw_image(tmp_path, gpu_device):
    from PIL import Image
    path = _scene_file(tmp_path, "cornell", RES=[48, 40])
    outs = {}
    for mode in (False, "variance"):
        d = tmp_path / f"out_{mode}"
        d.mkdir()
        img, png = P.render(path, 3, out_dir=str(d), denoise=mode)
        outs[mode] = (img, png, d)
    assert outs[False][0].tobytes() == outs["variance"][0].tobytes()
    assert Path(outs[False][1]).read_bytes() == Path(outs["variance"][1]).read_bytes()
    assert not list(outs[False][2].glob("*denoised*"))
    dn = list(outs["variance"][2].glob("cornell.*.3samp.denoised-var.png"))
    assert len(dn) == 1 and Image.open(dn[0]).size == (48, 40)
    assert Image.open(dn[0]).tobytes() != Image.open(outs["variance"][1]).tobytes()
    # one batch gives no variance: the plain filter's image under the same name
    d1 = tmp_path / "one"
    d1.mkdir()
    _, png1 = P.render(path, 1, out_dir=str(d1), denoise="variance")
    dn1 = list(d1.glob("cornell.*.1samp.denoised-var.png"))
    assert len(dn1) == 1 and dn1[0].stat().st_size > 0
    with pytest.raises(ValueError):
        P.render(path, 1, denoise="nonsense")


def test_denoise_variance_returns_the_filtered_variance_on_request(gpu_device):
    w, h = 37, 29
    rgb, var, gA, gB, alb = _synthetic(w, h, 5)
    g = {"normal": gA[..., :3], "mat": gA[..., 3].copy().view(np.int32), "position": gB[..., :3], "t": gB[..., 3],
         "albedo": alb[..., :3]}
    prm = _prm(3, 1)
    want, want_v = _host(rgb, 2.0, var, gA, gB, alb, prm)
    got, got_v = P.denoise_variance(rgb, 2.0, var, g, prm, return_variance=True)
    _same(got, want, "colour")
    _same(got_v, want_v, "variance")
    _same(P.denoise_variance(rgb, 2.0, var, g, prm), want, "colour alone")


# ---- CLI -------------------------------------------------------------------------------------------------
def test_cli_denoise_variance(tmp_path):
    exe = ROOT / "cuda_pathtracer_amd" / "pathtracer_amd"
    scene = str(SCENES / "sphere.json")
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir()
    b.mkdir()
    base = [str(exe), scene, "--iterations", "4", "--out"]
    r0 = subprocess.run(["timeout", "-k", "10", "120", *base, str(a)], capture_output=True, text=True)
    assert r0.returncode == 0, r0.stdout + r0.stderr
    r1 = subprocess.run(["timeout", "-k", "10", "120", *base, str(b), "--denoise-variance"], capture_output=True, text=True)
    assert r1.returncode == 0, r1.stdout + r1.stderr
    raw_a = list(a.glob("sphere.*.4samp.png"))
    raw_b = list(b.glob("sphere.*.4samp.png"))
    assert len(raw_a) == 1 and len(raw_b) == 1
    assert raw_a[0].read_bytes() == raw_b[0].read_bytes()
    dn = list(b.glob("sphere.*.4samp.denoised-var.png"))
    assert len(dn) == 1 and dn[0].stat().st_size > 0
    from PIL import Image
    assert Image.open(dn[0]).size == Image.open(raw_b[0]).size


# ---- quality -------------------------------------------------------------------------------------------
def test_variance_guided_16spp_is_closer_to_1024spp_than_raw_16spp(tmp_path, gpu_device):
    """Cornell 200 x 200, a spp = 4 context (batches of 4), reference = 1024 spp of the same run.  Only
    RMSE(variance-guided, 16 spp) < RMSE(raw, 16 spp) is asserted; the table is printed."""
    scene = P.Scene(_scene_file(tmp_path, "cornell", RES=[200, 200]))
    pt = P.PathTracer(scene, spp=4)
    pt.track_variance(True)
    shots = {}
    for it in range(1, 1025, 4):
        pt.render_pass(it)
        n = it + 3
        if n <= 256:
            pt.variance_update()
        if n in (16, 64, 256):
            shots[n] = (pt.image() / F(n), pt.denoised(float(n)), pt.denoised_variance(float(n)))
    ref = pt.image() / F(1024)
    pt.free()

    def rmse(a):
        return float(np.sqrt(np.mean((np.clip(a, 0, 1).astype(np.float64) - np.clip(ref, 0, 1)) ** 2)))

    for n, (raw, plain, var) in shots.items():
        print(f"RMSE {n} spp: raw={rmse(raw):.5f} plain={rmse(plain):.5f} variance-guided={rmse(var):.5f}")
    raw16, _, var16 = shots[16]
    assert rmse(var16) < rmse(raw16)
