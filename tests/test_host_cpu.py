"""Host-side product code on the CPU (no GPU): the C ABI loads and exports every declared symbol,
the scene loader matches the oracle's independent parse bit for bit, tonemap/PNG output matches
saveImage, errors are reported as status codes, and the device entry points fail loudly when no
GPU is present (there is no CPU fallback).

Reference: scene.cpp:33-219 (loader), utilities.cpp:84-92 (transforms), main.cpp:88-136 (camera
recompute, saveImage), image.cpp:22-42 (PNG), pathtrace.h:6-9 / efficient.h:9-11 (API surface).
"""
from __future__ import annotations

import json
import re
from pathlib import Path

import numpy as np
import pytest

import cuda_pathtracer_amd as P
from cuda_pathtracer_amd import _native as N
from oracle import binding as O

ROOT = Path(__file__).resolve().parent.parent
SCENES = ROOT / "tests" / "scenes"


def _declared_functions() -> set[str]:
    names = set()
    for h in (ROOT / "include").glob("*.h"):
        text = re.sub(r"/\*.*?\*/", "", h.read_text(), flags=re.S)
        for m in re.finditer(r"^[A-Za-z_][\w\s\*]*?\b((?:pt|sc)_\w+)\s*\(", text, flags=re.M):
            names.add(m.group(1))
    return names


def test_abi_exports_every_declared_symbol():
    declared = _declared_functions()
    assert len(declared) >= 40
    L = N.lib()
    missing = [n for n in sorted(declared) if not hasattr(L, n)]
    assert not missing, f"declared in include/*.h but not exported: {missing}"
    assert declared == set(N.SIGNATURES), (declared ^ set(N.SIGNATURES))


def test_abi_struct_sizes_match_header():
    text = (ROOT / "include" / "pt_amd.h").read_text()
    for struct, size in (("pt_material", 48), ("pt_geom", 272), ("pt_triangle", 124), ("pt_bvh_node", 40)):
        assert struct in text
    import ctypes as C
    assert C.sizeof(N.Material) == 48 and C.sizeof(N.Geom) == 272
    assert C.sizeof(N.Triangle) == 124 and C.sizeof(N.BvhNode) == 40
    assert C.sizeof(N.Camera) == 4 * (2 + 3 * 5 + 4)
    # the rows of pt_scene_bound_info and the report of pt_selftest_bounds, sized in the header's comments
    for struct, size, cls in (("pt_bound_info", 88, N.BoundInfo), ("pt_bounds_report", 264, N.BoundsReport)):
        assert re.search(r"\}\s*%s;\s*/\*\s*%d bytes" % (struct, size), text)
        assert C.sizeof(cls) == size


def _f(a):
    return np.array(list(a), np.float32)


@pytest.mark.parametrize("scene", ["cornell.json", "sphere.json"])
def test_scene_loader_matches_oracle(scene):
    path = SCENES / scene
    ps = P.Scene(path)
    osc = O.OracleScene.from_json(path)
    ng, nm, ntri, nnode, ntex = ps.counts()
    assert (ng, nm, ntri, nnode, ntex) == (len(osc.geoms), len(osc.materials), 0, 0, 0)
    for g, og in zip(ps.geoms(), osc.geoms):
        assert g.type == og.type and g.material_id == og.materialid
        for a, b in (("translation", "translation"), ("rotation", "rotation"), ("scale", "scale"),
                     ("transform", "transform"), ("inverse_transform", "inverse_transform"),
                     ("inv_transpose", "inv_transpose")):
            np.testing.assert_array_equal(_f(getattr(g, a)), _f(getattr(og, b)), err_msg=f"{scene} {a}")
    for m, om in zip(ps.materials(), osc.materials):
        for k in ("color", "spec_color"):
            np.testing.assert_array_equal(_f(getattr(m, k)), _f(getattr(om, k)))
        for k in ("spec_exponent", "has_reflective", "has_refractive", "ior", "emittance"):
            assert np.float32(getattr(m, k)) == np.float32(getattr(om, k)), k
    c, oc = ps.camera(), osc.cam
    assert tuple(c.res) == tuple(oc.res)
    for k in ("position", "look_at", "view", "up", "right", "fov", "pixel_length"):
        np.testing.assert_array_equal(_f(getattr(c, k)), _f(getattr(oc, k)), err_msg=k)
    st = ps.state()
    assert st.traceDepth == osc.depth and st.iterations == osc.iterations and st.imageName == osc.file


def test_materials_are_alphabetical():
    """nlohmann::json objects iterate in std::map order, so material ids are alphabetical
    (scene.cpp:40-85); objects refer to them by name."""
    data = json.loads((SCENES / "cornell.json").read_text())
    names = sorted(data["Materials"])
    mats = P.Scene(SCENES / "cornell.json").materials()
    for i, name in enumerate(names):
        rgb = data["Materials"][name].get("RGB", [0, 0, 0])
        np.testing.assert_array_equal(_f(mats[i].color), np.array(rgb, np.float32))


def test_programmatic_scene_matches_json(tmp_path):
    data = json.loads((SCENES / "cornell.json").read_text())
    js = P.Scene(SCENES / "cornell.json")
    sc = P.Scene()
    ids = {}
    for name in sorted(data["Materials"]):
        p = data["Materials"][name]
        rgb = p.get("RGB", [0.0, 0.0, 0.0])
        ids[name] = sc.add_material(rgb=rgb, specrgb=p.get("SPECRGB", rgb), specex=p.get("SPECEX", 1.0),
                                    reflective=p.get("REFLECTIVE", 0.0), emittance=p.get("EMITTANCE", 0.0))
    for o in data["Objects"]:
        sc.add_geom({"sphere": P.SPHERE, "cube": P.CUBE}[o["TYPE"]], ids[o["MATERIAL"]], o["TRANS"], o["ROTAT"],
                    o["SCALE"])
    c = data["Camera"]
    sc.set_camera(c["RES"], c["FOVY"], c["EYE"], c["LOOKAT"], c["UP"])
    sc.set_render(c["ITERATIONS"], c["DEPTH"], c["FILE"])
    sc.finalize()
    for a, b in zip(sc.geoms(), js.geoms()):
        np.testing.assert_array_equal(_f(a.inverse_transform), _f(b.inverse_transform))
    for k in ("position", "view", "right", "pixel_length"):
        np.testing.assert_array_equal(_f(getattr(sc.camera(), k)), _f(getattr(js.camera(), k)))


def test_scene_errors_are_status_codes(tmp_path):
    with pytest.raises(N.PtError, match="open|read|exist|No such"):
        P.Scene(tmp_path / "missing.json")
    bad = tmp_path / "bad.json"
    bad.write_text("{ not json")
    with pytest.raises(N.PtError):
        P.Scene(bad)
    data = json.loads((SCENES / "cornell.json").read_text())
    data["Camera"]["DEPTH"] = 65                          # device arrays hold <= 64 bounces
    deep = tmp_path / "deep.json"
    deep.write_text(json.dumps(data))
    with pytest.raises(N.PtError, match="[Dd]epth|DEPTH"):
        P.Scene(deep)
    sc = P.Scene()
    sc.add_geom(P.CUBE, 3, (0, 0, 0), (0, 0, 0), (1, 1, 1))   # materials may be added later ...
    sc.set_camera((8, 8), 45.0, (0, 0, 5), (0, 0, 0))
    with pytest.raises(N.PtError, match="material"):
        sc.finalize()                                          # ... but must exist at finalize
    with pytest.raises(N.PtError, match="camera"):
        P.Scene().finalize()


def test_tonemap_matches_oracle_and_png_roundtrip(tmp_path):
    rng = np.random.default_rng(5)
    img = rng.uniform(0, 3.0, size=(37, 53, 3)).astype(np.float32)
    img[0, 0] = [np.inf, -1.0, 0.0]
    out = P.tonemap(img, 2.0)
    np.testing.assert_array_equal(out[1:], O.tonemap(img, 2.0)[1:])
    np.testing.assert_array_equal(out[0, :-1], O.tonemap(img, 2.0)[0, :-1])
    path = tmp_path / "x.png"
    P.save_image(str(path), img, 2.0)
    from PIL import Image
    png = np.asarray(Image.open(path).convert("RGB"))
    assert png.shape == (37, 53, 3)
    np.testing.assert_array_equal(png, out)


def test_device_entry_points_fail_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    sc = P.Scene(SCENES / "cornell.json")
    with pytest.raises(N.PtError):
        P.PathTracer(sc)
    a = np.array([1, 5, 0, 1, 2, 0, 3], np.int32)
    with pytest.raises(N.PtError):
        P.Efficient.scan(7, np.zeros(7, np.int32), a)


def test_product_does_not_import_oracle():
    """The oracle is test infrastructure: the product package never imports, loads or links it
    (build.py only compiles it, as build() must)."""
    pat = re.compile(r"(import\s+oracle|from\s+oracle|liboracle|oracle_[a-z]+\s*\(|pt_oracle|sc_oracle)")
    for f in (ROOT / "cuda_pathtracer_amd").rglob("*"):
        if f.suffix in (".py", ".cpp", ".hip", ".h") and f.name != "build.py":
            assert not pat.search(f.read_text()), f


@pytest.mark.parametrize("shape", [(5, 6), (7, 40), (3, 9)])
def test_hdr_matches_stb_restatement_and_decodes(shape):
    """Image::saveHDR bytes (RGBE + stb's per-channel RLE) == the oracle's line-by-line restatement
    of the vendored stb_image_write writer; decoding them gives the pixels within RGBE precision.
    Runs and flat areas exercise both RLE packet kinds; width < 8 the raw path."""
    from cuda_pathtracer_amd import encode_hdr
    from oracle import hdr_oracle
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    H, W = shape
    img = rng.uniform(0, 8, (H, W, 3)).astype(np.float32)
    img[:, W // 3: W // 3 + 5] = 2.5          # runs
    img[0, 0] = 0.0                           # the zero pixel
    img[-1, -1] = [1e-3, 50.0, 0.2]
    got = encode_hdr(img, 4.0)
    assert got == hdr_oracle.encode_hdr(img, 4.0)
    dec = hdr_oracle.decode_hdr(got)
    ref = (img / np.float32(4.0))[:, ::-1]
    # RGBE shares one exponent per pixel: error <= 2^-7 of the pixel's largest component
    assert (np.abs(dec - ref) <= ref.max(axis=2, keepdims=True) * 2 ** -7 + 1e-30).all()


def _cornell_with_refraction_keys(tmp_path, opt_in=None):
    """cornell.json with REFRACTIVE / IOR added to two materials (keys the reference ignores)."""
    scene = json.loads((SCENES / "cornell.json").read_text())
    scene["Materials"]["specular_white"]["REFRACTIVE"] = 1.0
    scene["Materials"]["specular_white"]["IOR"] = 1.5
    scene["Materials"]["diffuse_red"]["IOR"] = 2.4
    if opt_in is not None:
        scene["Extensions"] = opt_in
    path = tmp_path / "cornell_refr.json"
    path.write_text(json.dumps(scene))
    return path


def _mat_table(s):
    return [(tuple(m.color), m.has_reflective, m.has_refractive, m.ior, m.emittance) for m in s.materials()]


def test_refraction_keys_ignored_by_default(tmp_path):
    """scene.cpp:46-56 never reads REFRACTIVE or IOR: by default the
    product's and the oracle's loaders ignore them too, so a reference scene that carries the keys
    loads exactly like the bundled file (the GPU render equality is test_render_gpu.py's
    test_refraction_keys_render_like_bundled_scene).  The extension is on with PT_LOAD_REFRACTION
    (refraction=True) or the file's own "Extensions": {"REFRACTION": true}."""
    path = _cornell_with_refraction_keys(tmp_path)
    bundled = _mat_table(P.Scene(SCENES / "cornell.json"))
    assert _mat_table(P.Scene(path)) == bundled
    assert all(m[2] == 0.0 and m[3] == 0.0 for m in bundled)
    on = _mat_table(P.Scene(path, refraction=True))
    assert on != bundled and any(m[2] == 1.0 and m[3] == np.float32(1.5) for m in on)
    for opt_in in ({"REFRACTION": True}, ["REFRACTION"]):
        assert _mat_table(P.Scene(_cornell_with_refraction_keys(tmp_path, opt_in))) == on
    assert _mat_table(P.Scene(_cornell_with_refraction_keys(tmp_path, {"REFRACTION": False}))) == bundled
    # the oracle follows the same rule
    o_off = [(m.has_refractive, m.ior) for m in O.OracleScene.from_json(path).materials]
    o_on = [(m.has_refractive, m.ior) for m in O.OracleScene.from_json(path, refraction=True).materials]
    assert o_off == [(m[2], m[3]) for m in bundled] and o_on == [(m[2], m[3]) for m in on]
    with pytest.raises(N.PtError):
        import ctypes as C
        h = C.c_void_p()
        N.check_pt(N.lib().pt_scene_load_json_ex(str(path).encode(), 0x80, C.byref(h)))


@pytest.mark.parametrize("ext", ["REFRACTION", {"REFRACTION": "yes"}, 1, ["refraction"], [True]])
def test_refraction_opt_in_forms_agree(tmp_path, ext):
    """Only `"Extensions": {"REFRACTION": true}` or `["REFRACTION"]` opt a file in; any other form
    (a bare string, a non-boolean value, other array items) loads with the extension off in both
    the product's loader (pt_scene.cpp file_wants_refraction) and the oracle's."""
    path = _cornell_with_refraction_keys(tmp_path, ext)
    bundled = _mat_table(P.Scene(SCENES / "cornell.json"))
    assert _mat_table(P.Scene(path)) == bundled
    o = [(m.has_refractive, m.ior) for m in O.OracleScene.from_json(path).materials]
    assert o == [(m[2], m[3]) for m in bundled]


def test_non_jpeg_texture_modes_follow_stb(tmp_path):
    """Non-JPEG textures are decoded on the host (pathtrace.py _stb_texels) with stbi_load's mode
    mapping: 16-bit grey keeps the high byte, a tRNS chunk adds an alpha channel to grey and RGB,
    palette images expand, 1-bit grey becomes 0/255, and an unmapped mode raises."""
    from PIL import Image
    from cuda_pathtracer_amd.pathtrace import _stb_texels
    g16 = np.array([[0, 255, 256, 65535], [1000, 40000, 512, 300]], np.uint16)
    im = Image.fromarray(g16.astype(np.int32), mode="I")
    assert np.array_equal(_stb_texels(im, "g16"), (g16 >> 8).astype(np.uint8))
    p = tmp_path / "g16.png"
    Image.fromarray(g16).save(p)
    with Image.open(p) as im2:
        assert np.array_equal(_stb_texels(im2, p), (g16 >> 8).astype(np.uint8))
    g8 = np.array([[0, 7, 255], [7, 9, 7]], np.uint8)
    p = tmp_path / "gt.png"
    Image.fromarray(g8).save(p, transparency=7)
    with Image.open(p) as im3:
        la = _stb_texels(im3, p)
    assert la.shape == (2, 3, 2) and np.array_equal(la[..., 0], g8)
    assert np.array_equal(la[..., 1], np.where(g8 == 7, 0, 255))
    rgb = np.arange(2 * 2 * 3, dtype=np.uint8).reshape(2, 2, 3)
    p = tmp_path / "rt.png"
    Image.fromarray(rgb).save(p, transparency=(0, 1, 2))
    with Image.open(p) as im4:
        ra = _stb_texels(im4, p)
    assert ra.shape == (2, 2, 4) and np.array_equal(ra[..., :3], rgb) and ra[0, 0, 3] == 0 and ra[1, 1, 3] == 255
    bw = Image.fromarray(np.array([[0, 255], [255, 0]], np.uint8)).convert("1")
    assert np.array_equal(_stb_texels(bw, "bw"), np.array([[0, 255], [255, 0]], np.uint8))
    with pytest.raises(ValueError):
        _stb_texels(Image.new("CMYK", (2, 2)), "cmyk")
