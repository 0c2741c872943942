"""Environment lighting without a GPU: the Radiance HDR reader, the lat-long -> octahedral
resampler, the gutter, and the float64 path replay with an environment judged on its own.

* The reader returns exactly the floats the RGBE bytes stand for (an independent Python decode, env_ref), for
  the project's own encoder's files and a hand-built flat one, and refuses every truncation without a crash.
* The resampler stays within 2^-22 x the largest source texel each map texel reads of a float64 numpy
  restatement: both evaluate the same float64 formulas and differ only in libm's last bits before the single
  rounding to float32, so the bound is that rounding (2^-24 relative), doubled twice.
* The gutter equals env_ref's rule with ==, and in the float64 restatement L is continuous across the fold, the
  axis planes and the texel edges.
* The replay (env_path_ref.replay_env, the open lantern of test_env_gpu.py): the conditions on the scene, asserted
  on the float64 side alone; float32 takes the same routes and stays at the constants test_env_gpu.py allows 8x of.
"""
import sys
from pathlib import Path

import numpy as np
import pytest

import cuda_pathtracer_amd as P

sys.path.insert(0, str(Path(__file__).resolve().parent))
import env_path_ref as EP  # noqa: E402
import env_ref as E  # noqa: E402
import path_ref as R  # noqa: E402
from env_path_ref import D, GOLDEN_HDR, REPLAYS, TEETH, Replays, replay_requests  # noqa: E402

REQUESTS = replay_requests()


def _id(req):
    key, iters, rank, world = req
    return f"{key}-it{iters[0]}..{iters[-1]}x{len(iters)}-r{rank}of{world}"


@pytest.fixture(scope="module")
def replays(tmp_path_factory):
    return Replays(tmp_path_factory.mktemp("env_replay_cpu"))


# ---- the HDR reader -----------------------------------------------------------------------------------------
def _pixels(h, w, seed):
    """Zeros, denormal-small values, values >= 2^100, runs and noise."""
    rng = np.random.default_rng(seed)
    img = (rng.random((h, w, 3), dtype=np.float32) * np.float32(3.0)).astype(np.float32)
    flat = img.reshape(-1, 3)
    flat[0] = 0.0
    if len(flat) > 3:
        flat[1] = (1e-39, 3e-40, 0.0)
        flat[2] = (2.0 ** 100, 2.0 ** 101, 1.5 * 2.0 ** 120)
        flat[3] = (1e-30, 5e-31, 2e-30)
    if w >= 8:
        img[h - 1, 2:w - 2] = (0.25, 0.5, 0.75)                 # a run in every channel
        img[0, w // 2:] = img[0, w // 2]
    return img


@pytest.mark.parametrize("h,w", [(1, 1), (3, 7), (2, 8), (5, 40)])
def test_reader_returns_the_floats_the_encoder_s_bytes_stand_for(h, w):
    data = P.encode_hdr(_pixels(h, w, h * w), 1.0)
    rle = b"\x02\x02" + bytes([w >> 8, w & 255]) in data
    assert rle == (w >= 8)
    got, want = P.decode_hdr(data), E.decode_hdr(data)
    assert got.dtype == np.float32 and got.shape == (h, w, 3)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    if w >= 8:
        assert (want >= 2.0 ** 100).any() and (want == 0).all(-1).any()


def test_reader_decodes_a_hand_built_flat_file():
    rgbe = np.random.default_rng(3).integers(0, 256, (4, 9, 4), dtype=np.uint8)
    rgbe[0, 0] = (255, 1, 0, 255)
    rgbe[0, 1] = (1, 2, 3, 1)                                   # 2^-135: denormal
    rgbe[0, 2] = (9, 9, 9, 0)                                   # exponent 0: black whatever the mantissas
    rgbe[:, :, 0] = np.where(rgbe[:, :, 0] == 2, 3, rgbe[:, :, 0])   # (no scanline may look like an RLE header)
    got = P.decode_hdr(E.flat_hdr(rgbe))
    want = E.decode_rgbe(rgbe)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and not got[0, 2].any() and got[0, 1, 0] == 2.0 ** -135


def test_reader_refuses_every_truncation_and_malformed_input():
    data = P.encode_hdr(_pixels(2, 8, 16), 1.0)
    assert P.decode_hdr(data).shape == (2, 8, 3)
    ok = 0
    for k in range(len(data)):
        try:
            assert P.decode_hdr(data[:k]).shape == (2, 8, 3)
            ok += 1
        except P.PtError as e:
            assert e.code == 5 and "hdr" in str(e)              # PT_ERR_PARSE
    assert ok == 0                                              # (the last byte is needed too)
    head = b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n"
    for bad in (b"", b"\n", b"RADIANCE\n\n-Y 1 +X 1\n\0\0\0\0", b"#?RADIANCE\n\n-Y 1 +X 1\n\0\0\0\0",
                b"#?RADIANCE\nFORMAT=32-bit_rle_xyze\n\n-Y 1 +X 1\n\0\0\0\0", head + b"+Y 1 +X 1\n\0\0\0\0",
                head + b"-Y 0 +X 1\n", head + b"-Y 1 +X 99999999999\n", head + b"-Y 1 +X 8\n\2\2\0\x08\x89\1",
                head + b"-Y 1 +X 8\n\2\2\0\x08\0", head + b"-Y 1 +X 8\n\2\2\0\x08\x09" + b"\1" * 9):
        with pytest.raises(P.PtError):
            P.decode_hdr(bad)


def test_a_header_that_promises_more_than_the_file_holds_is_refused_before_anything_is_sized(tmp_path):
    """A few bytes of header with a huge resolution, through every entry point that reads a file: an error code and
    a message, no allocation sized by the header (the process would abort on std::bad_alloc otherwise)."""
    head = b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n"
    scene = P.Scene()
    for k, dims in enumerate((b"-Y 999999 +X 999999\n", b"-Y 16384 +X 16384\n", b"-Y 20000 +X 10000\n" + b"\0" * 4096,
                              b"-Y 3 +X 40\n" + b"\2\2\0\x28" * 2, b"-Y 2 +X 7\n" + b"\1" * 55)):
        data = head + dims
        with pytest.raises(P.PtError) as e:
            P.decode_hdr(data)
        assert e.value.code == 5 and "hdr" in str(e.value)
        f = tmp_path / f"bad{k}.hdr"
        f.write_bytes(data)
        with pytest.raises(P.PtError) as e:
            scene.set_environment(f)
        assert e.value.code == 5 and scene.environment() is None
    with pytest.raises(P.PtError) as e:
        scene.set_environment(tmp_path / "missing.hdr")
    assert e.value.code == 4                                    # PT_ERR_IO
    # a scene file's ENVIRONMENT goes the same way, and its SIZE is checked as the number it is
    import json
    (tmp_path / "Textures").mkdir()
    (tmp_path / "Textures" / "huge.hdr").write_bytes(head + b"-Y 999999 +X 999999\n")
    (tmp_path / "Textures" / "sky.hdr").write_bytes(GOLDEN_HDR.read_bytes())
    spec = json.loads((Path(__file__).resolve().parent / "scenes" / "cornell.json").read_text())
    for envspec, code in (({"FILE": "huge.hdr"}, 5), ({"FILE": "sky.hdr", "SIZE": 1e300}, 5), ({"FILE": "sky.hdr", "SIZE": -3}, 5),
                          ({"FILE": "sky.hdr", "SIZE": 7}, 0)):
        spec["Extensions"] = {"ENVIRONMENT": envspec}
        (tmp_path / "scene.json").write_text(json.dumps(spec))
        if code:
            with pytest.raises(P.PtError) as e:
                P.Scene(str(tmp_path / "scene.json"))
            assert e.value.code == code
        else:
            assert P.Scene(str(tmp_path / "scene.json")).environment()["n"] == 7


def test_the_preview_refuses_the_material_sort_of_a_scene_with_an_environment():
    """The panel's box must not reach pt_set_flags, whose refusal inside the render loop would end the session."""
    from cuda_pathtracer_amd import preview as V
    scene = P.Scene(str(Path(__file__).resolve().parent / "scenes" / "cornell.json"))
    session = V.PreviewSession(scene)
    session.set_setting("sortbyMaterial", True)
    session.set_setting("sortbyMaterial", False)
    scene.set_environment_octa(np.ones((2, 2, 3), np.float32))
    with pytest.raises(ValueError, match="environment"):
        session.set_setting("sortbyMaterial", True)
    assert session.gui.sortbyMaterial is False
    session.set_setting("useThrustPartition", True)             # (no effect on the fused pipeline: allowed)


# ---- the resampler ----------------------------------------------------------------------------------------------
def _sources():
    rng = np.random.default_rng(8)
    y, x = np.meshgrid(np.linspace(0, 1, 32), np.linspace(0, 1, 64), indexing="ij")
    smooth = np.stack([1 + np.sin(6.283 * x) * y, 0.5 + y * y, 2 + np.cos(12.566 * x)], -1).astype(np.float32)
    return {"random16x8": (rng.random((8, 16, 3), dtype=np.float32) * np.float32(5)).astype(np.float32), "smooth64x32": smooth,
            "constant1x1": np.array([[[0.3, 1.7, 250.0]]], np.float32),
            # other aspects than 2:1: a wide strip and a tall one (the box filter has a factor per direction)
            "strip96x4": (rng.random((4, 96, 3), dtype=np.float32) * np.float32(5)).astype(np.float32),
            "tall6x40": (rng.random((40, 6, 3), dtype=np.float32) * np.float32(5)).astype(np.float32)}


@pytest.mark.parametrize("n", [1, 2, 5, 16])
@pytest.mark.parametrize("name", ["random16x8", "smooth64x32", "constant1x1", "strip96x4", "tall6x40"])
def test_resampler_equals_the_float64_restatement_within_one_rounding(name, n):
    src = _sources()[name]
    scene = P.Scene()
    scene.set_environment(src, size=n)
    got = scene.environment()
    assert got["n"] == n
    want, reads = E.resample(src, n)
    err = np.abs(got["map"][1:-1, 1:-1, :3].astype(np.float64) - want).max(-1)
    print(f"{name} -> {n}: largest error {(err / reads).max():.3e} of the largest texel read (allowed {2.0 ** -22:.3e})")
    assert (err <= 2.0 ** -22 * reads).all()
    assert np.array_equal(got["map"], E.pad(got["map"][1:-1, 1:-1, :3]))
    if name == "constant1x1":
        assert (got["map"][..., :3] == src[0, 0]).all()
    if name == "strip96x4" and n == 2:
        # no source column is skipped: 96 columns over the 8 texels round the horizon are blocks of 12, and the mean of
        # the map (every source texel weighted alike by the block means and the taps' partition of unity in x) moves when
        # any one source texel does
        bumped = src.copy()
        for col in range(0, 96, 5):
            bumped[:] = src
            bumped[:, col] += np.float32(100.0)
            scene.set_environment(bumped, size=n)
            assert np.abs(scene.environment()["map"][1:-1, 1:-1, :3] - got["map"][1:-1, 1:-1, :3]).max() > 0.5, col


def test_default_size_follows_the_source_height():
    scene = P.Scene()
    for h, w in ((1, 1), (8, 16), (9, 5), (30, 60)):
        scene.set_environment(np.ones((h, w, 3), np.float32))
        assert scene.environment()["n"] == E.default_size(h) == max(1, h // 2)
    assert E.default_size(4096) == 2048 and E.default_size(10000) == 2048
    for bad in (-1, 4097):
        with pytest.raises(P.PtError):
            scene.set_environment(np.ones((2, 4, 3), np.float32), size=bad)
    with pytest.raises(P.PtError):
        scene.set_environment(np.ones((2, 4, 3), np.float32), scale=float("nan"))
    scene.clear_environment()
    assert scene.environment() is None


def test_the_committed_sky_is_the_encoder_s_own_file():
    """tests/golden/env_sky.hdr: a generated 32x16 lat-long sky (a gradient, a bright patch, a darker lower half)
    written by encode_hdr: run-length coded scanlines under the encoder's own header."""
    data = GOLDEN_HDR.read_bytes()
    assert data.startswith(b"#?RADIANCE\n# Written by stb_image_write.h\nFORMAT=32-bit_rle_rgbe\n") and b"\x02\x02\x00\x20" in data
    img = P.decode_hdr(data)
    assert len(data) < 10 * 1024 and img.shape == (16, 32, 3) and img.min() >= 0 and img.max() > 4
    assert np.array_equal(img.view(np.uint32), E.decode_hdr(data).view(np.uint32))


# ---- the gutter ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 5, 8])
def test_gutter_equals_the_edge_rule(n):
    texels = np.random.default_rng(n).random((n, n, 3), dtype=np.float32)
    scene = P.Scene()
    scene.set_environment_octa(texels, scale=2.0, rotate=(1.0, 2.0, 3.0))
    got = scene.environment()
    assert (got["n"], got["scale"], got["rotate"]) == (n, 2.0, (1.0, 2.0, 3.0))
    assert np.array_equal(got["map"].view(np.uint32), E.pad(texels).view(np.uint32))


@pytest.mark.parametrize("n", [2, 5, 8])
def test_lookup_is_continuous_across_the_fold_the_axis_planes_and_the_texel_edges(n):
    """A property of the DEFINITION (env_ref.pad and env_ref.lookup in float64): it runs no product code and passes
    without it.  It bears on the product only through test_gutter_equals_the_edge_rule (the product's gutter == pad's)
    and test_env_gpu.py's bit-equal env_eval (the product's lookup == lookup's in float32)."""
    rng = np.random.default_rng(100 + n)
    texels = rng.random((n, n, 3))
    padded = E.pad(texels.astype(np.float32))
    spread = float(np.ptp(padded[..., :3]))                      # the map's largest texel difference
    rot = E.rotation((0.0, 0.0, 0.0))
    eps = 1e-6
    base, step = [], []
    m = 400
    for axis in range(3):                                       # straddle r.y = 0 (axis 1: the fold) and the planes x = 0, z = 0
        p = rng.normal(size=(m, 3))
        p /= np.abs(p).sum(-1, keepdims=True)
        p[:, axis] = 0
        e = np.zeros(3)
        e[axis] = eps / 2
        base.append(p - e)
        step.append(np.broadcast_to(2 * e, p.shape))
    for k in range(1, n):                                       # straddle the texel boundaries of either axis, both halves
        for ax in (0, 2):
            for sy in (1.0, -1.0):
                bnd = 2.0 * k / n - 1.0                         # the boundary's coordinate in the square
                if sy < 0 and bnd == 0:
                    continue                                    # (the plane x = 0 or z = 0 of the lower half: above)
                # a point of the square on the boundary: inside the diamond |u| + |v| <= 1 for the upper half,
                # outside it for the lower one, where the fold (its own inverse) gives the projected direction
                other = rng.uniform(-1, 1, size=m) * (1.0 - abs(bnd))
                if sy < 0:
                    other = np.where(other >= 0, 1.0, -1.0) * rng.uniform(1.0 - abs(bnd), 1.0, size=m)
                u, v = (np.full(m, bnd), other) if ax == 0 else (other, np.full(m, bnd))
                if sy < 0:
                    u, v = (1.0 - np.abs(v)) * np.where(u >= 0, 1.0, -1.0), (1.0 - np.abs(u)) * np.where(v >= 0, 1.0, -1.0)
                p = np.stack([u, (1.0 - np.abs(u) - np.abs(v)) * sy, v], -1)
                e = np.zeros(3)
                e[ax] = eps / 2
                base.append(p - e)
                step.append(np.broadcast_to(2 * e, p.shape))
    a, s = np.concatenate(base), np.concatenate(step)
    La = E.lookup(padded, 1.0, rot, a, np.float64)
    Lb = E.lookup(padded, 1.0, rot, a + s, np.float64)
    # the pair's distance in texel units: the square's coordinates move by at most |delta|_1 / |d|_1 (x 2 for the
    # fold's mirrored axis), and one unit of the square is n / 2 texels
    dist = (np.abs(s).sum(-1) / np.abs(a).sum(-1)) * 2.0 * (n / 2.0)
    jump = np.abs(La - Lb).max(-1)
    print(f"n = {n}: largest jump {jump.max():.3e}, allowed {(spread * dist * 2).min():.3e} .. {(spread * dist * 2).max():.3e}")
    assert (jump <= spread * dist * 2).all()
    assert jump.max() > 0


# ---- the replay on its own ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("req", REQUESTS, ids=_id)
def test_the_open_lantern_meets_its_conditions(replays, req):
    ref = replays(*req)
    keep = ref["keep"]
    excluded = 1.0 - keep.mean()
    ends, via = EP.env_shares(ref)
    nan = ((ref["route"] & R.REFRACT_NAN) != 0) & keep[None, None]
    print(f"{_id(req)}: excluded {100 * excluded:.2f} %, ends in the environment {100 * ends:.1f} %, only after a mirror "
          f"or glass bounce {100 * via:.1f} %, k < 0 refractions {int(nan.sum())}")
    assert excluded <= 0.10
    if req[0] == "glass_d2":                                     # the NaN tooth's view: nearly every camera path refracts with k < 0
        first = ((ref["route"][:, 0] & R.REFRACT_NAN) != 0).any(0)
        assert (ref["geom"][:, 0] == R.GLASS_15).all() and first[keep].mean() >= 0.9
    else:
        assert ends >= 0.50 and via >= 0.05
    # a k < 0 refraction is present, its NaN ray misses everything and contributes 0
    assert nan.any()
    it, b, r, c = np.argwhere(nan[:, :-1])[0]
    assert ref["route"][it, b + 1, r, c] == (R.MISS | R.NAN_RAY) and not ref["env"][it, b + 1, r, c]
    one = replays(req[0], (req[1][it],), req[2], req[3])
    assert not one["image"][r, c].any()


@pytest.mark.parametrize("req", REQUESTS, ids=_id)
def test_float32_takes_the_same_route_and_stays_at_the_recorded_constants(replays, req):
    r64, r32 = replays(*req), replays(*req, dt=np.float32)
    assert r32["image"].dtype == np.float32
    keep = r64["keep"]
    assert np.array_equal(r64["route"][:, :, keep], r32["route"][:, :, keep])
    assert np.array_equal(r64["geom"][:, :, keep], r32["geom"][:, :, keep])
    assert np.array_equal(r64["env"][:, :, keep], r32["env"][:, :, keep])
    d = R.deviation(r32["image"], r64["image"])[keep].max()
    print(f"{_id(req)}: D_c = {d:.3e}")
    assert 2.0 ** -24 <= D[req[0]] and d <= D[req[0]], (req, d)


def test_without_an_environment_the_replay_is_path_ref_s(replays):
    scene, textures, _, _ = replays.scene("open_d8")
    fl = R.default_flags(**REPLAYS["open_d8"][3])
    a = EP.replay_env(scene, textures, None, (1, 7), 8, fl)
    b = R.replay(scene, textures, (1, 7), 8, fl)
    for k in ("image", "keep", "route", "geom", "hit_risky"):
        assert np.array_equal(a[k], b[k]), k
    assert not a["env"].any()


@pytest.mark.parametrize("variant", list(TEETH))
def test_each_deliberate_error_changes_the_replay(replays, variant):
    key = TEETH[variant]
    right, wrong = replays(key, (1, 7)), replays(key, (1, 7), variant=variant)
    keep = right["keep"] & wrong["keep"]
    share = float((R.deviation(right["image"], wrong["image"])[keep] > 8 * D[key]).mean())
    print(f"{variant} on {key}: {100 * share:.1f} % of the kept pixels differ beyond 8 x D_c")
    assert share >= 0.20
    if variant == "env_nan_L":                                  # (the share on the open lantern's own view, for the record)
        a, b = replays("open_d2", (1, 7)), replays("open_d2", (1, 7), variant=variant)
        k2 = a["keep"] & b["keep"]
        print(f"  on open_d2: {100 * float((R.deviation(a['image'], b['image'])[k2] > 8 * D['open_d2']).mean()):.1f} %")
