"""Python mirror of the reference's render boundary, backed by libpt_amd.so.

Reference interfaces (path_tracer/src):
  Scene::Scene(filename) / loadFromJSON           scene.h:17-35, scene.cpp:16-219   -> Scene(path)
  GuiDataContainer (runtime flags)                utilities.h:17-34                 -> GuiDataContainer
  InitDataContainer / pathtraceInit / pathtraceFree / pathtrace   pathtrace.h:6-9   -> same names
  runCuda's iteration loop + saveImage            main.cpp:88-168                   -> render(), save_image()
The reference keeps one implicit global render (file-static device buffers); the module-level
functions below reproduce that, while PathTracer objects allow any number of independent
contexts (one per GPU / pixel tile).
"""
from __future__ import annotations

import ctypes as C
import os
import time
from dataclasses import dataclass
from pathlib import Path

import numpy as np

from . import _native as N
from ._native import (AdaptiveParams, BloomParams, DenoiseParams, DenoiseVarParams, DisplayParams, EnvParams, ExrChannel, ExrParams, HdrParams,  # noqa: F401
                      JpegParams, PngParams, TemporalParams, check_pt, lib)

SPHERE, CUBE, MESH = 0, 1, 2


class GuiDataContainer:
    """Runtime flags with the reference defaults (utilities.h:17-34)."""

    def __init__(self):
        self.TracedDepth = 0
        self.russianRoulette = True
        self.useBVHtree = True
        self.useBBox = True
        self.sortbyMaterial = False
        self.useThrustPartition = False
        self.SSAA = True
        self.DoF = True
        self.aperture = 0.1
        self.focal_len = 10.0
        # extension, off = the reference: albedo applied once instead of twice (include/pt_amd.h)
        self.singleAlbedo = False
        # extension, off = the reference: cull BVH nodes beyond the closest hit so far
        self.bvhCull = False
        # tile schedule of the look-back kernels: False = static grid (fastest), True = claimed
        # tiles (other kernels / processes share the GPU); default from PT_AMD_SCHEDULE=claim
        self.sharedGPU = os.environ.get("PT_AMD_SCHEDULE", "") == "claim"
        # extension, off = the reference: shading RNG keyed by the global pixel, so the image does
        # not depend on the shard layout or the material sort (bitwise equal across GPU counts)
        self.rngKeyPixel = False

    def to_c(self) -> N.Flags:
        f = N.Flags()
        f.russian_roulette = int(bool(self.russianRoulette))
        f.use_bvh = int(bool(self.useBVHtree))
        f.use_bbox = int(bool(self.useBBox))
        f.sort_by_material = int(bool(self.sortbyMaterial))
        f.use_thrust_partition = int(bool(self.useThrustPartition))
        f.ssaa = int(bool(self.SSAA))
        f.dof = int(bool(self.DoF))
        f.aperture = float(self.aperture)
        f.focal_dist = float(self.focal_len)
        f.single_albedo = int(bool(self.singleAlbedo))
        f.bvh_cull = int(bool(self.bvhCull))
        f.shared_gpu = int(bool(self.sharedGPU))
        f.rng_key_pixel = int(bool(self.rngKeyPixel))
        return f


@dataclass
class RenderState:
    iterations: int
    traceDepth: int
    imageName: str


def decode_jpeg(data: bytes) -> np.ndarray:
    """Texture::load's stbi_load(file, &w, &h, &comp, 0) (sceneStructs.h:171-175) for JPEG bytes,
    by the native decoder (pt_decode_jpeg): an (h, w, components) uint8 array."""
    L = lib()
    w, h, c = C.c_int32(), C.c_int32(), C.c_int32()
    check_pt(L.pt_decode_jpeg(data, len(data), C.byref(w), C.byref(h), C.byref(c), None, 0))
    out = np.empty((h.value, w.value, c.value), np.uint8)
    check_pt(L.pt_decode_jpeg(data, len(data), C.byref(w), C.byref(h), C.byref(c),
                              out.ctypes.data_as(C.c_void_p), out.size))
    return out


def decode_hdr(data: bytes) -> np.ndarray:
    """A Radiance .hdr file's pixels, (h, w, 3) float32 in file order, by the native reader (pt_decode_hdr)."""
    L = lib()
    w, h = C.c_int32(), C.c_int32()
    check_pt(L.pt_decode_hdr(data, len(data), C.byref(w), C.byref(h), None, 0))
    out = np.empty((h.value, w.value, 3), np.float32)
    check_pt(L.pt_decode_hdr(data, len(data), C.byref(w), C.byref(h), out.ctypes.data_as(C.c_void_p), out.size))
    return out


def env_eval(scene: "Scene", dirs) -> np.ndarray:
    """L(d) of the scene's environment for an (n, 3) array of directions, evaluated on the device by the
    lookup the bounce kernels call (pt_env_eval): (n, 3) float32."""
    d = np.ascontiguousarray(dirs, np.float32)
    if d.ndim != 2 or d.shape[1] != 3:
        raise ValueError("env_eval: expected an (n, 3) array")
    out = np.empty_like(d)
    check_pt(lib().pt_env_eval_host(scene.handle, d.shape[0], d.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
    return out


class Scene:
    """Scene description; `Scene(path)` loads a reference JSON scene file (textures decoded
    natively, pt_decode_jpeg).  refraction=True reads the REFRACTIVE / IOR material keys the
    reference loader ignores (PT_LOAD_REFRACTION; a file may also opt in with
    "Extensions": {"REFRACTION": true}); by default they are ignored, like scene.cpp:46-56."""

    def __init__(self, filename: str | os.PathLike | None = None, refraction: bool = False,
                 device_bvh: bool = False):
        """device_bvh=True builds the BVH on the current HIP device (pt_scene_set_bvh_builder: the
        same tree as the host build, byte for byte)."""
        self._h = C.c_void_p()
        L = lib()
        if filename is None:
            check_pt(L.pt_scene_create(C.byref(self._h)))
            if device_bvh:
                check_pt(L.pt_scene_set_bvh_builder(self._h, 1))
            return
        opts = (1 if refraction else 0) | (2 if device_bvh else 0)
        check_pt(L.pt_scene_load_json_ex(str(filename).encode(), opts, C.byref(self._h)))
        self._fill_non_jpeg_textures()

    def set_bvh_builder(self, device: bool) -> None:
        check_pt(lib().pt_scene_set_bvh_builder(self._h, 1 if device else 0))

    def bvh_build_info(self) -> tuple[bool, float]:
        """(the last BVH build ran on the device, its wall time in ms)."""
        d, ms = C.c_int32(), C.c_double()
        check_pt(lib().pt_scene_bvh_build_info(self._h, C.byref(d), C.byref(ms)))
        return bool(d.value), float(ms.value)

    def texture_path(self, tid: int) -> str:
        buf = C.create_string_buffer(4096)
        check_pt(lib().pt_scene_texture_path(self._h, int(tid), buf, 4096))
        return buf.value.decode()

    def _fill_non_jpeg_textures(self) -> None:
        """Texture files that are not JPEG (PNG, BMP, TGA: stbi_load reads them too) are left
        undecoded by the native loader (include/pt_amd.h); decode them here.  These formats are
        lossless, so a decoder yields stbi_load(path, &w, &h, &comp, 0)'s texels once the modes are
        mapped as stb maps them: palette images expand to RGB, or RGBA with a tRNS chunk; a tRNS chunk
        adds an alpha channel to grey and RGB images too; 16-bit samples keep their high byte; 1-bit
        grey expands to 0/255.  A mode stb would not produce raises instead of converting silently
        (non-JPEG texels are parity-unpinned: no reference fixture covers them)."""
        ntex = self.counts()[4]
        for tid in range(ntex):
            path = self.texture_path(tid)
            with open(path, "rb") as f:
                head = f.read(2)
            if head == b"\xff\xd8":
                continue
            from PIL import Image   # (host-side file IO only; not on the render path)
            with Image.open(path) as im:
                px = _stb_texels(im, path)
            h, w = px.shape[:2]
            comps = 1 if px.ndim == 2 else px.shape[2]
            check_pt(lib().pt_scene_set_texture_pixels(self._h, tid, w, h, comps, px.ctypes.data_as(C.c_void_p)))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                lib().pt_scene_free(h)
            except Exception:
                pass
            self._h = None

    @property
    def handle(self) -> C.c_void_p:
        return self._h

    # -- programmatic construction --
    def add_material(self, rgb=(0, 0, 0), specrgb=None, specex=1.0, reflective=0.0, refractive=0.0, ior=0.0,
                     emittance=0.0, texture_id=-1) -> int:
        m = N.Material()
        m.color[:] = [float(v) for v in rgb]
        m.spec_color[:] = [float(v) for v in (specrgb if specrgb is not None else rgb)]
        m.spec_exponent = specex
        m.has_reflective = reflective
        m.has_refractive = refractive
        m.ior = ior
        m.emittance = emittance
        m.texture_id = texture_id
        out = C.c_int32()
        check_pt(lib().pt_scene_add_material(self._h, C.byref(m), C.byref(out)))
        return out.value

    def add_geom(self, type_: int, material: int, trans, rotat, scale) -> int:
        out = C.c_int32()
        check_pt(lib().pt_scene_add_geom(self._h, type_, material, N.f3(trans), N.f3(rotat), N.f3(scale),
                                         C.byref(out)))
        return out.value

    def set_camera(self, res, fovy, eye, lookat, up=(0, 1, 0)) -> None:
        check_pt(lib().pt_scene_set_camera(self._h, int(res[0]), int(res[1]), float(fovy), N.f3(eye), N.f3(lookat),
                                           N.f3(up)))

    def set_render(self, iterations: int, depth: int, file: str = "render") -> None:
        check_pt(lib().pt_scene_set_render(self._h, iterations, depth, file.encode()))

    def finalize(self) -> None:
        check_pt(lib().pt_scene_finalize(self._h))

    # -- inspection --
    def counts(self):
        v = [C.c_int32() for _ in range(5)]
        check_pt(lib().pt_scene_counts(self._h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def camera(self) -> N.Camera:
        cam = N.Camera()
        check_pt(lib().pt_scene_get_camera(self._h, C.byref(cam)))
        return cam

    def orbit(self) -> tuple[float, float, float]:
        """(phi, theta, zoom) of the loaded camera, as main.cpp:59-73 derives them."""
        p, t, z = C.c_float(), C.c_float(), C.c_float()
        check_pt(lib().pt_scene_get_orbit(self._h, C.byref(p), C.byref(t), C.byref(z)))
        return p.value, t.value, z.value

    def set_orbit(self, phi: float, theta: float, zoom: float, look_at) -> None:
        """runCuda's camera recompute (main.cpp:117-136) for an orbit about look_at; contexts created
        afterwards render it."""
        check_pt(lib().pt_scene_set_orbit(self._h, float(phi), float(theta), float(zoom), N.f3(look_at)))

    def state(self) -> RenderState:
        it, d = C.c_int32(), C.c_int32()
        buf = C.create_string_buffer(1024)
        check_pt(lib().pt_scene_get_render(self._h, C.byref(it), C.byref(d), buf, 1024))
        return RenderState(it.value, d.value, buf.value.decode())

    def geoms(self):
        ng = self.counts()[0]
        arr = (N.Geom * max(ng, 1))()
        lib().pt_scene_get_geoms(self._h, arr, ng)
        return list(arr)[:ng]

    def triangles(self):
        """The world-space mesh triangles in BVH leaf order, each with its load-order id
        (pt_scene_get_triangles)."""
        nt = self.counts()[2]
        arr = (N.Triangle * max(nt, 1))()
        if lib().pt_scene_get_triangles(self._h, arr, nt) != nt:
            raise RuntimeError("pt_scene_get_triangles: triangle count changed")
        return list(arr)[:nt]

    def room_info(self, gui: GuiDataContainer | None = None) -> dict:
        """The room a PathTracer of this scene with these flags would bound as one group
        (pt_scene_room_info: the host's scene preparation alone, no device), as PathTracer.room_info."""
        if not hasattr(lib(), "pt_scene_room_info"):
            raise N.NativeLibraryError("the loaded library (PT_AMD_LIB) predates pt_scene_room_info")
        flags = (gui or GuiDataContainer()).to_c()
        n, faces = C.c_int32(), (C.c_int32 * 6)()
        lo, hi = (C.c_float * 3)(), (C.c_float * 3)()
        check_pt(lib().pt_scene_room_info(self._h, C.byref(flags), C.byref(n), faces, lo, hi))
        return {"walls": int(n.value), "faces": [int(v) for v in faces], "lo": [float(v) for v in lo],
                "hi": [float(v) for v in hi]}

    def bound_info(self, gui: GuiDataContainer | None = None) -> dict:
        """The widened bounds a PathTracer of this scene with these flags would use (pt_scene_bound_info:
        the host's scene preparation alone, no device): R, r_limit, bounded, abs_slack, wb_tslack and one
        dict per geom (bkind, slo, shi, wlo, whi, tight, tslack, back, wback)."""
        if not hasattr(lib(), "pt_scene_bound_info"):
            raise N.NativeLibraryError("the loaded library (PT_AMD_LIB) predates pt_scene_bound_info")
        flags = (gui or GuiDataContainer()).to_c()
        ng = self.counts()[0]
        rows = (N.BoundInfo * max(ng, 1))()
        R, lim, bounded = C.c_double(), C.c_double(), C.c_int32()
        slack, wbts = C.c_float(), C.c_float()
        check_pt(lib().pt_scene_bound_info(self._h, C.byref(flags), rows, ng, C.byref(R), C.byref(lim),
                                           C.byref(bounded), C.byref(slack), C.byref(wbts)))
        geoms = [{"bkind": int(r.bkind), "slo": list(r.slo), "shi": list(r.shi), "wlo": list(r.wlo),
                  "whi": list(r.whi), "tight": list(r.tight), "tslack": float(r.tslack), "back": float(r.back),
                  "wback": float(r.wback)} for r in list(rows)[:ng]]
        return {"R": float(R.value), "r_limit": float(lim.value), "bounded": bool(bounded.value),
                "abs_slack": float(slack.value), "wb_tslack": float(wbts.value), "geoms": geoms}

    def selftest_bounds(self, gui: GuiDataContainer | None = None, n: int = 1 << 16, seed: int = 1) -> dict:
        """The device's per-pair check of every bound form of this scene against the exact test
        (pt_selftest_bounds): pair and violation counts per kind (bkind 1, 2, 3, 4, room), rays per class,
        and the first violating record, if any."""
        if not hasattr(lib(), "pt_selftest_bounds"):
            raise N.NativeLibraryError("the loaded library (PT_AMD_LIB) predates pt_selftest_bounds")
        flags = (gui or GuiDataContainer()).to_c()
        r = N.BoundsReport()
        check_pt(lib().pt_selftest_bounds(self._h, C.byref(flags), int(n), int(seed), C.byref(r)))
        kinds = ("1", "2", "3", "4", "room")
        first = None
        if r.has_first:
            first = {"geom": int(r.first_geom), "form": int(r.first_form),
                     "origin_bits": [hex(v) for v in r.first_origin], "dir_bits": [hex(v) for v in r.first_dir],
                     "bound_bits": hex(r.first_bound), "t_bits": hex(r.first_t)}
        return {"pairs": dict(zip(kinds, map(int, r.pairs))), "bad_tagged": dict(zip(kinds, map(int, r.bad_tagged))),
                "bad_float": dict(zip(kinds, map(int, r.bad_float))), "rays": [int(v) for v in r.rays],
                "skipped": [int(v) for v in r.skipped], "first": first}

    # -- environment lighting --
    @staticmethod
    def _env_params(scale, rotate, size) -> "N.EnvParams":
        p = N.EnvParams.default()
        p.scale = float(scale)
        p.rotate_deg[:] = [float(v) for v in rotate]
        p.size = 0 if size is None else int(size)
        return p

    def set_environment(self, source, scale: float = 1.0, rotate=(0, 0, 0), size: int | None = None) -> None:
        """The scene's environment from a lat-long image: an (h, w, 3) float array (row 0 up), or the path of
        a Radiance .hdr file.  rotate: degrees about x, y, z; size: the octahedral map's n (default: from the
        source height, at most 2048).  PathTracers created afterwards shade their misses with it."""
        p = self._env_params(scale, rotate, size)
        if isinstance(source, (str, os.PathLike)):
            check_pt(lib().pt_scene_load_environment(self._h, os.fspath(source).encode(), C.byref(p)))
            return
        a = np.ascontiguousarray(source, np.float32)
        if a.ndim != 3 or a.shape[2] != 3:
            raise ValueError("environment: expected an (h, w, 3) array")
        check_pt(lib().pt_scene_set_environment(self._h, a.shape[1], a.shape[0], a.ctypes.data_as(C.c_void_p), C.byref(p)))

    def set_environment_octa(self, texels, scale: float = 1.0, rotate=(0, 0, 0)) -> None:
        """The environment from the octahedral map itself: an (n, n, 3) float array, row j along z, column i
        along x, +y at the centre (no gutter)."""
        a = np.ascontiguousarray(texels, np.float32)
        if a.ndim != 3 or a.shape[0] != a.shape[1] or a.shape[2] != 3:
            raise ValueError("environment: expected an (n, n, 3) array")
        p = self._env_params(scale, rotate, None)
        check_pt(lib().pt_scene_set_environment_octa(self._h, a.shape[0], a.ctypes.data_as(C.c_void_p), C.byref(p)))

    def clear_environment(self) -> None:
        check_pt(lib().pt_scene_clear_environment(self._h))

    def environment(self) -> dict | None:
        """None, or dict(n, scale, rotate, map): map is the padded (n + 2, n + 2, 4) float32 array the device reads."""
        n, p = C.c_int32(), N.EnvParams()
        check_pt(lib().pt_scene_get_environment(self._h, C.byref(n), C.byref(p), None, 0))
        if n.value <= 0:
            return None
        m = np.empty((n.value + 2, n.value + 2, 4), np.float32)
        check_pt(lib().pt_scene_get_environment(self._h, C.byref(n), C.byref(p), m.ctypes.data_as(C.c_void_p), m.size))
        return {"n": int(n.value), "scale": float(p.scale), "rotate": tuple(float(v) for v in p.rotate_deg), "map": m}

    def materials(self):
        nm = self.counts()[1]
        arr = (N.Material * max(nm, 1))()
        lib().pt_scene_get_materials(self._h, arr, nm)
        return list(arr)[:nm]


def _stream_ptr(stream):
    if stream is None:
        return None
    return int(getattr(stream, "cuda_stream", stream))


def _stb_texels(im, path) -> np.ndarray:
    """PIL image -> the (h, w[, c]) uint8 texels stbi_load(..., 0) returns for the same file."""
    trans = "transparency" in im.info
    mode = im.mode
    if mode == "P":
        return np.ascontiguousarray(np.asarray(im.convert("RGBA" if trans else "RGB"), dtype=np.uint8))
    if mode == "1":
        im, mode = im.convert("L"), "L"
    if mode in ("I;16", "I;16B", "I;16L", "I"):   # 16-bit grey: stb keeps the high byte
        g = (np.asarray(im).astype(np.uint32) >> 8).astype(np.uint8)
        if trans:   # tRNS on grey: stb adds an alpha channel (opaque except the keyed value)
            key = int(im.info["transparency"])
            a = np.where(np.asarray(im).astype(np.uint32) == key, 0, 255).astype(np.uint8)
            return np.ascontiguousarray(np.stack([g, a], axis=-1))
        return np.ascontiguousarray(g)
    if mode == "L" and trans:
        return np.ascontiguousarray(np.asarray(im.convert("LA"), dtype=np.uint8))
    if mode == "RGB" and trans:
        return np.ascontiguousarray(np.asarray(im.convert("RGBA"), dtype=np.uint8))
    if mode in ("L", "LA", "RGB", "RGBA"):
        return np.ascontiguousarray(np.asarray(im, dtype=np.uint8))
    raise ValueError(f"texture {path}: image mode {mode!r} has no stbi_load equivalent here")


class PathTracer:
    """One render context (pathtraceInit ... pathtraceFree) for a pixel tile of the image.

    rank/world select the rows y % world == rank; spp iterations are traced per pass.
    """

    def __init__(self, scene: Scene, gui: GuiDataContainer | None = None, rank: int = 0, world: int = 1,
                 spp: int = 1):
        self.scene = scene
        self.gui = gui or GuiDataContainer()
        self._h = C.c_void_p()
        flags = self.gui.to_c()
        shard = N.Shard(rank, world, spp, 0)
        check_pt(lib().pt_create(scene.handle, C.byref(flags), C.byref(shard), C.byref(self._h)))
        w, rows, npix, npaths = (C.c_int32() for _ in range(4))
        check_pt(lib().pt_tile_info(self._h, C.byref(w), C.byref(rows), C.byref(npix), C.byref(npaths)))
        self.width, self.rows, self.npix, self.npaths = w.value, rows.value, npix.value, npaths.value
        self.rank, self.world, self.spp = rank, world, spp

    def free(self) -> None:
        if self._h is not None and self._h.value:
            check_pt(lib().pt_destroy(self._h))
        self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def set_flags(self, gui: GuiDataContainer) -> None:
        self.gui = gui
        check_pt(lib().pt_set_flags(self._h, C.byref(gui.to_c())))

    def counters(self) -> dict:
        """Host-side counters (pt_ctx_counters): camera-mask builds and device-synchronising
        pt_set_flags calls."""
        b, y = C.c_uint64(), C.c_uint64()
        check_pt(lib().pt_ctx_counters(self._h, C.byref(b), C.byref(y)))
        return {"mask_builds": int(b.value), "flag_syncs": int(y.value)}

    def stream_info(self) -> dict:
        """Stream budget (pt_ctx_stream_info): the context's lanes and busy streams, the busy streams
        of every live context of the process, the hardware queues per priority, and whether pt_create
        capped the lanes to stay within them."""
        v = [C.c_int32() for _ in range(5)]
        check_pt(lib().pt_ctx_stream_info(self._h, *[C.byref(x) for x in v]))
        k = ("lanes", "busy_streams", "process_busy", "hw_queues", "lanes_capped")
        return {a: int(x.value) for a, x in zip(k, v)}

    def cmask_info(self) -> dict:
        """First-bounce camera masks (pt_ctx_cmask_info): built, share of empty 64-pixel blocks, and
        whether the fused first bounce skips those waves in its own instantiation."""
        on, sk, fr = C.c_int32(), C.c_int32(), C.c_double()
        check_pt(lib().pt_ctx_cmask_info(self._h, C.byref(on), C.byref(fr), C.byref(sk)))
        return {"on": bool(on.value), "empty_frac": float(fr.value), "skip_fused": bool(sk.value)}

    def room_info(self) -> dict:
        """The room whose walls the later bounces bound as one group (pt_ctx_room_info): wall count,
        the geom index per face (-x, +x, -y, +y, -z, +z; -1: none) and the box between the walls."""
        if not hasattr(lib(), "pt_ctx_room_info"):
            raise N.NativeLibraryError("the loaded library (PT_AMD_LIB) predates pt_ctx_room_info")
        n, faces = C.c_int32(), (C.c_int32 * 6)()
        lo, hi = (C.c_float * 3)(), (C.c_float * 3)()
        check_pt(lib().pt_ctx_room_info(self._h, C.byref(n), faces, lo, hi))
        return {"walls": int(n.value), "faces": [int(v) for v in faces], "lo": [float(v) for v in lo],
                "hi": [float(v) for v in hi]}

    def depart_counts(self) -> dict:
        """PT_AMD_VERIFY_BOUNDS=1 only (pt_ctx_depart_counts): later-bounce rays whose wall behind the
        room's tight plane alone called a miss, and the per-cube loop's zero-bound candidates (all, and
        those the same claim could remove)."""
        if not hasattr(lib(), "pt_ctx_depart_counts"):
            raise N.NativeLibraryError("the loaded library (PT_AMD_LIB) predates pt_ctx_depart_counts")
        v = [C.c_uint64() for _ in range(3)]
        check_pt(lib().pt_ctx_depart_counts(self._h, *[C.byref(x) for x in v]))
        return {"room": int(v[0].value), "loop_zero": int(v[1].value), "loop_depart": int(v[2].value)}

    def exact_counts(self) -> dict:
        """PT_AMD_VERIFY_BOUNDS=1 only (pt_ctx_exact_counts): exact tests the bounded closest hit ran,
        and those whose range gate tripped (the literal path recomputed them)."""
        if not hasattr(lib(), "pt_ctx_exact_counts"):
            raise N.NativeLibraryError("the loaded library (PT_AMD_LIB) predates pt_ctx_exact_counts")
        v = [C.c_uint64() for _ in range(2)]
        check_pt(lib().pt_ctx_exact_counts(self._h, *[C.byref(x) for x in v]))
        return {"tests": int(v[0].value), "tripped": int(v[1].value)}

    def walk_info(self) -> dict:
        """Mesh scenes: 4-wide walk on/off, its exact t-cull on/off and the share of slots whose
        cull margin can pay (pt_ctx_walk_info)."""
        qw, on, fr = C.c_int32(), C.c_int32(), C.c_double()
        check_pt(lib().pt_ctx_walk_info(self._h, C.byref(qw), C.byref(on), C.byref(fr)))
        info = {"quad_walk": bool(qw.value), "tcull": bool(on.value), "tcull_frac": float(fr.value)}
        if hasattr(lib(), "pt_ctx_walk_kind"):
            # walk: the kernel ahead of the bounce kernel ("quads", "pairs", "nodes"; "none": inside it);
            # inline_walk: the walk inside the bounce kernel and of the G-buffer ("pairs", "nodes",
            # "nodes_private": the reference's 64 private entries; "none": no tree, or the BVH flag off)
            names = ("none", "quads", "pairs", "nodes", "nodes_private")
            w, iw, dp, sb = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
            check_pt(lib().pt_ctx_walk_kind(self._h, C.byref(w), C.byref(iw), C.byref(dp), C.byref(sb)))
            info.update(walk=names[w.value], inline_walk=names[iw.value], bvh_depth=int(dp.value),
                        stack_bound=int(sb.value))
        return info

    def render_pass(self, iter_first: int, stream=None) -> None:
        """pathtrace(): iterations [iter_first, iter_first + spp) for this tile, asynchronous."""
        check_pt(lib().pt_render_pass(self._h, int(iter_first), _stream_ptr(stream)))

    def render_ahead(self, iteration: int, stream=None) -> None:
        """One-iteration contexts: queue iteration `iteration`'s bounces now (pt_render_ahead); the
        render_pass(iteration) that follows with the same flags only adds their colours."""
        check_pt(lib().pt_render_ahead(self._h, int(iteration), _stream_ptr(stream)))

    def image(self) -> np.ndarray:
        """Tile accumulator (sum of radiance over iterations), shape (rows, width, 3) float32."""
        out = np.empty((self.rows, self.width, 3), dtype=np.float32)
        check_pt(lib().pt_get_image(self._h, out.ctypes.data))
        return out

    def set_image(self, image: np.ndarray) -> None:
        """Resume: load a tile accumulator saved from image() (pt_set_accum)."""
        img = np.ascontiguousarray(image, dtype=np.float32)
        if img.shape != (self.rows, self.width, 3):
            raise ValueError(f"accumulator shape {img.shape} != {(self.rows, self.width, 3)}")
        check_pt(lib().pt_set_accum(self._h, img.ctypes.data))

    def save_state(self, path: str, iterations_done: int) -> str:
        """Checkpoint the accumulator and the next iteration index (extension: resume a render)."""
        np.savez(path, image=self.image(), iterations_done=np.int64(iterations_done),
                 rank=np.int32(self.rank), world=np.int32(self.world))
        return str(path)

    def load_state(self, path: str) -> int:
        """Load a checkpoint written by save_state for the same tile; returns iterations_done."""
        with np.load(path, allow_pickle=False) as z:
            if int(z["rank"]) != self.rank or int(z["world"]) != self.world:
                raise ValueError("checkpoint is for another tile")
            self.set_image(z["image"])
            return int(z["iterations_done"])

    def copy_image_to(self, dst_ptr: int, stream=None) -> None:
        check_pt(lib().pt_copy_image(self._h, C.c_void_p(dst_ptr), _stream_ptr(stream)))

    def reset_image(self, stream=None) -> None:
        check_pt(lib().pt_reset_image(self._h, _stream_ptr(stream)))

    def preview_rgba(self, iteration: int, dst_ptr: int, stream=None) -> None:
        check_pt(lib().pt_preview_rgba(self._h, int(iteration), C.c_void_p(dst_ptr), _stream_ptr(stream)))

    def _preview_file(self, entry, iteration: int, encoder: "_Encoder", stream) -> bytes:
        out, size = encoder._buffers()
        check_pt(entry(self._h, int(iteration), encoder._h, out.data_ptr(), encoder.cap, size.data_ptr(), _stream_ptr(stream)))
        return encoder._read(stream)

    def preview_bloom(self, iteration: int, bloom: "Bloom", dst_ptr: "int | None" = None, stream=None):
        """The accumulated image of `iteration` iterations through `bloom` (pt_preview_bloom), still an
        accumulator of that many samples: as floats at the device pointer dst_ptr, asynchronous; or without one into
        the device buffer `bloom` keeps and returned as a (rows, width, 3) float32 array."""
        ptr = bloom._buffer().data_ptr() if dst_ptr is None else int(dst_ptr)
        check_pt(lib().pt_preview_bloom(self._h, int(iteration), bloom._h, C.c_void_p(ptr), _stream_ptr(stream)))
        if dst_ptr is not None:
            return None
        bloom._wait(stream)
        return bloom._buffer().cpu().numpy()

    def _bloomed(self, iteration: int, bloom: "Bloom", stream, reader) -> int:
        """preview_bloom into the device buffer `bloom` keeps: the pointer of an accumulator of `iteration` samples for
        `reader` (a DisplayTransform or an encoder), which reads an image of its own size from it."""
        if (reader.width, reader.height) != (bloom.width, bloom.height):
            raise ValueError(f"bloom= is for {bloom.width} x {bloom.height} images, {type(reader).__name__} for "
                             f"{reader.width} x {reader.height}")
        ptr = bloom._buffer().data_ptr()
        self.preview_bloom(iteration, bloom, ptr, stream)
        return ptr

    def preview_display(self, iteration: int, display: "DisplayTransform", dst_ptr: int, pixel_stride: int = 4,
                        stream=None, bloom: "Bloom | None" = None) -> None:
        """The accumulated image of `iteration` iterations through `display` (pt_preview_display: metered first in
        auto mode) as RGB8 / RGBA8 bytes at the device pointer dst_ptr; asynchronous.  bloom: a Bloom the image goes
        through first, into the device buffer it keeps."""
        if bloom is not None:
            entry = lib().pt_display_frame if display.automatic else lib().pt_display_apply
            check_pt(entry(display._h, C.c_void_p(self._bloomed(iteration, bloom, stream, display)), float(iteration), C.c_void_p(dst_ptr),
                           int(pixel_stride), _stream_ptr(stream)))
            return
        check_pt(lib().pt_preview_display(self._h, int(iteration), display._h, C.c_void_p(dst_ptr), int(pixel_stride),
                                          _stream_ptr(stream)))

    def _preview_displayed(self, iteration: int, encoder: "_Encoder", display: "DisplayTransform", stream, bloom=None) -> bytes:
        """preview_display into the device pixels `encoder` keeps, then its pixels entry: only the file crosses."""
        pix = encoder._pixel_buffer()
        self.preview_display(iteration, display, pix.data_ptr(), 4, stream, bloom=bloom)
        return encoder.encode(pix.data_ptr(), pixel_stride=4, stream=stream)

    def preview_jpeg(self, iteration: int, encoder: "JpegEncoder", stream=None, display: "DisplayTransform | None" = None,
                     bloom: "Bloom | None" = None) -> bytes:
        """The accumulated image of `iteration` iterations as preview_rgba converts it, as a JPEG file
        encoded on the device by `encoder` (pt_preview_jpeg): only the file crosses to the host.  display: a
        DisplayTransform that converts it instead, still on the device.  bloom: a Bloom the image goes
        through first, into the device buffer it keeps; the encoder's accumulator entry follows."""
        if display is not None:
            return self._preview_displayed(iteration, encoder, display, stream, bloom)
        if bloom is not None:
            return encoder.encode(self._bloomed(iteration, bloom, stream, encoder), samples=float(iteration), stream=stream)
        return self._preview_file(lib().pt_preview_jpeg, iteration, encoder, stream)

    def preview_png(self, iteration: int, encoder: "PngEncoder", stream=None, display: "DisplayTransform | None" = None,
                    bloom: "Bloom | None" = None) -> bytes:
        """The accumulated image of `iteration` iterations as a PNG file written on the device by `encoder`
        (pt_preview_png), converted as the encoder's params.conv says: only the file crosses to the host.  display:
        a DisplayTransform that converts it instead, still on the device.  bloom: as preview_jpeg's."""
        if display is not None:
            return self._preview_displayed(iteration, encoder, display, stream, bloom)
        if bloom is not None:
            return encoder.encode(self._bloomed(iteration, bloom, stream, encoder), samples=float(iteration), stream=stream)
        return self._preview_file(lib().pt_preview_png, iteration, encoder, stream)

    def save_png(self, path: str, iteration: int) -> str:
        """saveImage's file written on the device: save_image's pixels (pt_tonemap's conversion, x-mirrored) of the
        accumulator, without the accumulator crossing to the host."""
        prm = N.PngParams.default()
        prm.conv, prm.mirror_x = N.PNG_CONV_SAVE, 1
        enc = PngEncoder(self.width, self.rows, prm)
        try:
            data = self.preview_png(iteration, enc)
        finally:
            enc.free()
        with open(path, "wb") as f:
            f.write(data)
        return str(path)

    def preview_hdr(self, iteration: int, encoder: "HdrEncoder", stream=None, bloom: "Bloom | None" = None) -> bytes:
        """The accumulated image of `iteration` iterations as a Radiance HDR file written on the device by
        `encoder` (pt_preview_hdr): only the file crosses to the host.  bloom: a Bloom the image goes through first
        (DESIGN.md §20), into the device buffer it keeps."""
        if bloom is not None:
            return encoder.encode(self._bloomed(iteration, bloom, stream, encoder), float(iteration), stream=stream)
        return self._preview_file(lib().pt_preview_hdr, iteration, encoder, stream)

    def save_hdr(self, path: str, iteration: int, bloom: "Bloom | None" = None) -> str:
        """save_image_hdr's file (x-mirrored, accumulator / iteration) written on the device, without the
        accumulator crossing to the host.  bloom: as preview_hdr's."""
        prm = N.HdrParams.default()
        prm.mirror_x = 1
        enc = HdrEncoder(self.width, self.rows, prm)
        try:
            data = self.preview_hdr(iteration, enc, bloom=bloom)
        finally:
            enc.free()
        with open(path, "wb") as f:
            f.write(data)
        return str(path)

    def preview_exr(self, iteration: int, encoder: "ExrEncoder", layers: int = N.EXR_BEAUTY, stream=None,
                    bloom: "Bloom | None" = None) -> bytes:
        """The layers `layers` (a mask of EXR_BEAUTY .. EXR_ID) as one OpenEXR file written on the device by `encoder`
        (pt_preview_exr), whose channels must be exr_ctx_channels(layers, half)'s: the accumulated image of `iteration`
        iterations and the first-hit planes.  Only the file crosses to the host.  bloom: a Bloom the image goes through
        first, into the device buffer it keeps; the beauty layer alone (ValueError otherwise)."""
        if bloom is not None:
            if int(layers) != N.EXR_BEAUTY:
                raise ValueError("preview_exr: bloom= takes the beauty layer alone")
            ptr = self._bloomed(iteration, bloom, stream, encoder)
            return encoder.encode([ptr, ptr + 4, ptr + 8], strides=[3] * 3, divisors=[float(iteration)] * 3, stream=stream)
        out, size = encoder._buffers()
        check_pt(lib().pt_preview_exr(self._h, int(iteration), int(layers), encoder._h, out.data_ptr(), encoder.cap,
                                      size.data_ptr(), _stream_ptr(stream)))
        return encoder._read(stream)

    def save_exr(self, path: str, iteration: int, layers: int = N.EXR_BEAUTY, half: int = 0, bloom: "Bloom | None" = None) -> str:
        """The layers as a ZIP-compressed OpenEXR file, x-mirrored like every saved image, written on the device; the
        layers of `half` that may be are stored as HALF.  bloom: as preview_exr's."""
        prm = N.ExrParams.default()
        prm.mirror_x = 1
        enc = ExrEncoder(self.width, self.rows, exr_ctx_channels(layers, half), prm)
        try:
            data = self.preview_exr(iteration, enc, layers, bloom=bloom)
        finally:
            enc.free()
        with open(path, "wb") as f:
            f.write(data)
        return str(path)

    def gbuffer(self) -> dict:
        """First-hit feature planes of the tile (pt_get_gbuffer; the deterministic camera ray): normal
        (rows, W, 3), mat (rows, W) int32 with -1 on a miss, position (rows, W, 3), t (rows, W) with -1
        on a miss, albedo (rows, W, 3) and uv (rows, W, 2)."""
        r, w = self.rows, self.width
        ga, gb, al = (np.empty((r, w, 4), np.float32) for _ in range(3))
        uv = np.empty((r, w, 2), np.float32)
        check_pt(lib().pt_get_gbuffer(self._h, ga.ctypes.data, gb.ctypes.data, al.ctypes.data, uv.ctypes.data))
        return {"normal": ga[..., :3].copy(), "mat": ga[..., 3].copy().view(np.int32), "position": gb[..., :3].copy(),
                "t": gb[..., 3].copy(), "albedo": al[..., :3].copy(), "uv": uv}

    def denoised(self, samples: float, params: "N.DenoiseParams | None" = None) -> np.ndarray:
        """The accumulator of `samples` samples filtered by the edge-avoiding a-trous denoiser over this
        context's G-buffer (pt_denoise_image; world == 1 only): (H, W, 3) float32, per-sample radiance
        (tonemap(..., 1.0) writes it).  The accumulator is not modified."""
        prm = params if params is not None else N.DenoiseParams.default()
        out = np.empty((self.rows, self.width, 3), np.float32)
        check_pt(lib().pt_denoise_image(self._h, float(samples), C.byref(prm), out.ctypes.data))
        return out

    def track_variance(self, on: bool = True) -> None:
        """Start (from the accumulator as it stands) or stop tracking the per-pixel variance of the
        luminance (pt_track_variance; world == 1 only).  Passes are not changed: call variance_update
        after each."""
        check_pt(lib().pt_track_variance(self._h, int(bool(on))))

    def variance_update(self, batch_samples: float | None = None, demodulate: bool = True, stream=None) -> None:
        """One batch: what the accumulator gained since the last update, batch_samples samples (default:
        the context's spp), divided by the first-hit albedo with `demodulate` (pt_variance_update)."""
        bs = float(self.spp if batch_samples is None else batch_samples)
        check_pt(lib().pt_variance_update(self._h, bs, int(bool(demodulate)), _stream_ptr(stream)))

    def variance_info(self) -> dict:
        on, n, bs = C.c_int32(), C.c_int32(), C.c_float()
        check_pt(lib().pt_variance_info(self._h, C.byref(on), C.byref(n), C.byref(bs)))
        return {"on": bool(on.value), "batches": int(n.value), "batch_samples": float(bs.value)}

    def variance(self, samples: float) -> np.ndarray:
        """(rows, W) float32: the variance of the luminance of the accumulator's per-sample mean over
        `samples` samples, from the tracked batch means (pt_get_variance; needs 2 batches)."""
        out = np.empty((self.rows, self.width), np.float32)
        check_pt(lib().pt_get_variance(self._h, float(samples), out.ctypes.data))
        return out

    def denoised_variance(self, samples: float, params: "N.DenoiseVarParams | None" = None) -> np.ndarray:
        """denoised() with the variance-guided filter and the tracked variance (pt_denoise_image_var;
        tracking on and at least 2 batches, else PtError).  The accumulator is not modified."""
        prm = params if params is not None else N.DenoiseVarParams.default()
        out = np.empty((self.rows, self.width, 3), np.float32)
        check_pt(lib().pt_denoise_image_var(self._h, float(samples), C.byref(prm), out.ctypes.data))
        return out

    def adaptive(self, on: bool = True) -> None:
        """Start (from the accumulator as it stands, every 64-pixel block active) or stop adaptive
        sampling (pt_adaptive_enable): later passes trace the active blocks only.  Needs
        world == 1, an analytic scene with camera masks and the fused or the material-sorted pipeline."""
        check_pt(lib().pt_adaptive_enable(self._h, int(bool(on))))

    def adaptive_update(self, demodulate: bool = True, stream=None) -> None:
        """One batch (the context's spp) of the active blocks into their moments, after a pass
        (pt_adaptive_update)."""
        check_pt(lib().pt_adaptive_update(self._h, int(bool(demodulate)), _stream_ptr(stream)))

    def adaptive_select(self, params: "N.AdaptiveParams | None" = None) -> dict:
        """Choose the active blocks from the moments (pt_adaptive_select; synchronous):
        {"active_blocks", "blocks"}; a caller may stop at 0 active blocks."""
        prm = params if params is not None else N.AdaptiveParams.default()
        a, n = C.c_int32(), C.c_int32()
        check_pt(lib().pt_adaptive_select(self._h, C.byref(prm), C.byref(a), C.byref(n)))
        return {"active_blocks": int(a.value), "blocks": int(n.value)}

    def adaptive_set_mask(self, mask) -> None:
        """Region rendering: trace only the blocks whose entry is nonzero (pt_adaptive_set_mask; one
        entry per 64 consecutive pixels of image().reshape(-1, 3))."""
        m = np.ascontiguousarray(np.asarray(mask).reshape(-1) != 0, dtype=np.uint8)
        check_pt(lib().pt_adaptive_set_mask(self._h, m.ctypes.data, int(m.size)))

    def adaptive_info(self) -> dict:
        v = [C.c_int32() for _ in range(4)]
        bs = C.c_float()
        check_pt(lib().pt_adaptive_info(self._h, *[C.byref(x) for x in v], C.byref(bs)))
        return {"on": bool(v[0].value), "blocks": int(v[1].value), "active_blocks": int(v[2].value),
                "updates": int(v[3].value), "batch_samples": float(bs.value)}

    def adaptive_state(self) -> dict:
        """The adaptive state as it stands (pt_adaptive_get): m1, m2, hot (rows, W), prev (rows, W, 3),
        nb and act (blocks,) uint32."""
        r, w = self.rows, self.width
        nblk = (self.npix + 63) // 64
        m1, m2 = np.empty((r, w), np.float32), np.empty((r, w), np.float32)
        pv, hot = np.empty((r, w, 3), np.float32), np.empty((r, w), np.uint8)
        nb, act = np.empty(nblk, np.uint32), np.empty(nblk, np.uint32)
        check_pt(lib().pt_adaptive_get(self._h, m1.ctypes.data, m2.ctypes.data, pv.ctypes.data, nb.ctypes.data,
                                       act.ctypes.data, hot.ctypes.data))
        return {"m1": m1, "m2": m2, "prev": pv, "nb": nb, "act": act, "hot": hot}

    def adaptive_image(self, var_params: "N.DenoiseVarParams | None" = None, return_variance: bool = False):
        """(rows, W, 3) float32 per-sample radiance: every pixel's accumulator divided by the samples its
        block received, or with var_params the variance-guided filter's output on it (pt_adaptive_image).
        return_variance adds the (rows, W) variance of its luminance."""
        out = np.empty((self.rows, self.width, 3), np.float32)
        var = np.empty((self.rows, self.width), np.float32) if return_variance else None
        check_pt(lib().pt_adaptive_image(self._h, C.byref(var_params) if var_params is not None else None,
                                         out.ctypes.data, var.ctypes.data if return_variance else None))
        return (out, var) if return_variance else out

    def stats(self) -> dict:
        s = N.Stats()
        check_pt(lib().pt_stats(self._h, C.byref(s)))
        depth = self.scene.state().traceDepth
        return {"segments": int(s.segments), "passes": int(s.passes),
                "bounce_live": [int(s.bounce_live[k]) for k in range(depth)],
                "bounce_emit": [int(s.bounce_emit[k]) for k in range(depth)],
                "emissive_hits": int(s.emissive_hits), "bound_mismatch": int(s.bound_mismatch),
                "device_error": int(s.device_error)}

    def profile(self, on: bool = True) -> None:
        check_pt(lib().pt_profile_enable(self._h, int(on)))

    # PT_KIND_* of include/pt_amd.h, in order
    KINDS = ("first_bounce", "bounce", "compact", "sort", "traverse", "first_traverse")

    def profile_read(self) -> dict:
        """{kind: (summed ms, launches, busy ms)} since the previous read (HIP events on the launch
        streams); busy ms = the union of the kind's launch intervals (lanes overlap launches)."""
        k = len(self.KINDS)
        ms = (C.c_double * k)()
        busy = (C.c_double * k)()
        n = (C.c_uint64 * k)()
        check_pt(lib().pt_profile_read_kinds(self._h, k, ms, busy, n))
        return {name: (float(ms[i]), int(n[i]), float(busy[i])) for i, name in enumerate(self.KINDS)}


def _plane4(xyz: np.ndarray, w: np.ndarray, shape) -> np.ndarray:
    out = np.empty(shape + (4,), np.float32)
    out[..., :3] = np.asarray(xyz, np.float32).reshape(shape + (3,))
    out[..., 3] = np.asarray(w).reshape(shape)
    return out


def denoise(image: np.ndarray, samples: float, gbuffer: dict, params: "N.DenoiseParams | None" = None) -> np.ndarray:
    """pt_denoise_host: filter an accumulated (H, W, 3) image of `samples` samples with the planes of
    PathTracer.gbuffer() (normal, mat, position, t, albedo) -> (H, W, 3) float32 per-sample radiance."""
    img = np.ascontiguousarray(image, dtype=np.float32)
    shape = img.shape[:2]
    mat = np.ascontiguousarray(gbuffer["mat"], dtype=np.int32).view(np.float32)
    ga = _plane4(gbuffer["normal"], mat, shape)
    gb = _plane4(gbuffer["position"], np.asarray(gbuffer["t"], np.float32), shape)
    al = _plane4(gbuffer["albedo"], np.zeros(shape, np.float32), shape)
    prm = params if params is not None else N.DenoiseParams.default()
    out = np.empty(shape + (3,), np.float32)
    check_pt(lib().pt_denoise_host(shape[1], shape[0], img.ctypes.data, float(samples), ga.ctypes.data, gb.ctypes.data,
                                   al.ctypes.data, C.byref(prm), out.ctypes.data))
    return out


def denoise_variance(image: np.ndarray, samples: float, variance: np.ndarray, gbuffer: dict,
                     params: "N.DenoiseVarParams | None" = None, return_variance: bool = False):
    """pt_denoise_var_host: denoise() with the variance-guided filter; `variance` is the (H, W) variance of
    the luminance of image / samples (demodulated when params.demodulate), as PathTracer.variance gives it.
    With return_variance also the (H, W) variance of the filtered image."""
    img = np.ascontiguousarray(image, dtype=np.float32)
    shape = img.shape[:2]
    var = np.ascontiguousarray(variance, dtype=np.float32).reshape(shape)
    mat = np.ascontiguousarray(gbuffer["mat"], dtype=np.int32).view(np.float32)
    ga = _plane4(gbuffer["normal"], mat, shape)
    gb = _plane4(gbuffer["position"], np.asarray(gbuffer["t"], np.float32), shape)
    al = _plane4(gbuffer["albedo"], np.zeros(shape, np.float32), shape)
    prm = params if params is not None else N.DenoiseVarParams.default()
    out = np.empty(shape + (3,), np.float32)
    ovar = np.empty(shape, np.float32) if return_variance else None
    check_pt(lib().pt_denoise_var_host(shape[1], shape[0], img.ctypes.data, float(samples), var.ctypes.data,
                                       ga.ctypes.data, gb.ctypes.data, al.ctypes.data, C.byref(prm), out.ctypes.data,
                                       ovar.ctypes.data if return_variance else None))
    return (out, ovar) if return_variance else out


class TemporalHistory:
    """pt_temporal: the denoiser's history of a full (height, width) image across camera moves
    (DESIGN.md §12).  It belongs to no context: feed it a frame after every pass, from whichever
    PathTracer renders the current camera, and take the image to show from image()."""

    CASES = {0: None, 1: "empty", 2: "same_view", 3: "new_view"}   # PT_TEMPORAL_*

    def __init__(self, width: int, height: int, params: "N.TemporalParams | None" = None):
        self.width, self.height = int(width), int(height)
        self._h = C.c_void_p()
        check_pt(lib().pt_temporal_create(self.width, self.height, C.byref(params) if params is not None else None,
                                          C.byref(self._h)))

    def free(self) -> None:
        if self._h is not None and self._h.value:
            check_pt(lib().pt_temporal_destroy(self._h))
        self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def reset(self) -> None:
        """Forget the history: the next frame starts from nothing (pt_temporal_reset)."""
        check_pt(lib().pt_temporal_reset(self._h))

    def info(self) -> dict:
        n, bs, k = C.c_int32(), C.c_float(), C.c_int32()
        check_pt(lib().pt_temporal_info(self._h, C.byref(n), C.byref(bs), C.byref(k)))
        return {"frames": int(n.value), "batch_samples": float(bs.value), "last_case": self.CASES[int(k.value)]}

    def frame(self, tracer: PathTracer, samples: float, stream=None) -> None:
        """One frame from a world == 1 context of this size whose accumulator holds `samples` samples
        (pt_temporal_frame_ctx); the context may be freed afterwards."""
        check_pt(lib().pt_temporal_frame_ctx(self._h, tracer._h, float(samples), _stream_ptr(stream)))

    def frame_arrays(self, camera: "N.Camera", image: np.ndarray, samples: float, gbuffer: dict) -> None:
        """The same from host arrays (pt_temporal_frame_host): the camera (Scene.camera()), the
        accumulated (H, W, 3) image and the planes of PathTracer.gbuffer() made with that camera."""
        shape = (self.height, self.width)
        img = np.ascontiguousarray(image, dtype=np.float32)
        if img.shape != shape + (3,):
            raise ValueError(f"image shape {img.shape} != {shape + (3,)}")
        mat = np.ascontiguousarray(gbuffer["mat"], dtype=np.int32).view(np.float32)
        ga = _plane4(gbuffer["normal"], mat, shape)
        gb = _plane4(gbuffer["position"], np.asarray(gbuffer["t"], np.float32), shape)
        al = _plane4(gbuffer["albedo"], np.zeros(shape, np.float32), shape)
        check_pt(lib().pt_temporal_frame_host(self._h, C.byref(camera), img.ctypes.data, float(samples), ga.ctypes.data,
                                              gb.ctypes.data, al.ctypes.data))

    def image(self, var_params: "N.DenoiseVarParams | None" = None, return_variance: bool = False,
              return_history: bool = False):
        """The history's image, (H, W, 3) float32 per-sample radiance (tonemap(..., 1.0) writes it): the
        resolved mean, or with var_params the variance-guided filter's output on it (pt_temporal_image).
        return_variance adds the (H, W) variance of its luminance, return_history the (H, W) history
        length in samples."""
        shape = (self.height, self.width)
        out = np.empty(shape + (3,), np.float32)
        var = np.empty(shape, np.float32) if return_variance else None
        his = np.empty(shape, np.float32) if return_history else None
        check_pt(lib().pt_temporal_image(self._h, C.byref(var_params) if var_params is not None else None,
                                         out.ctypes.data, var.ctypes.data if return_variance else None,
                                         his.ctypes.data if return_history else None))
        res = (out,) + ((var,) if return_variance else ()) + ((his,) if return_history else ())
        return res if len(res) > 1 else out

    def _planes(self) -> dict:
        """The state as it stands (pt_temporal_get; for tests): mean (H, W, 3), h (H, W), mu (H, W, 2),
        gA, gB, albedo (H, W, 4) and prev (H, W, 3)."""
        s = (self.height, self.width)
        h0, ga, gb, al = (np.empty(s + (4,), np.float32) for _ in range(4))
        h1, pv = np.empty(s + (2,), np.float32), np.empty(s + (3,), np.float32)
        check_pt(lib().pt_temporal_get(self._h, h0.ctypes.data, h1.ctypes.data, ga.ctypes.data, gb.ctypes.data,
                                       pv.ctypes.data, al.ctypes.data))
        return {"mean": h0[..., :3].copy(), "h": h0[..., 3].copy(), "mu": h1, "gA": ga, "gB": gb, "prev": pv, "albedo": al}


def _jpeg_params(quality: int, subsampling, mirror_x: bool) -> "N.JpegParams":
    sub = {"444": N.JPEG_444, "420": N.JPEG_420, N.JPEG_444: N.JPEG_444, N.JPEG_420: N.JPEG_420}.get(subsampling)
    if sub is None:
        raise ValueError(f"subsampling {subsampling!r}: '444' or '420'")
    p = N.JpegParams.default()
    p.quality, p.subsampling, p.mirror_x = int(quality), sub, int(bool(mirror_x))
    return p


class _Encoder:
    """What the device encoders share: an object for (height, width) images that owns its scratch and a device
    output buffer of `cap` bytes (default: `bound`, which every file fits).  A subclass names its format, its
    parameter type and, in _entry(library), its create, bound, destroy, pixels and accum entry points."""

    def __init__(self, width: int, height: int, params=None, cap: int | None = None):
        self.width, self.height = int(width), int(height)
        self._h = C.c_void_p()
        self._out = self._size = self._pix = None
        create, bound, self._destroy, self._pixels, self._accum = self._entry(lib())
        prm = params if params is not None else self._params.default()
        check_pt(create(self.width, self.height, C.byref(prm), C.byref(self._h)))
        self.bound = int(bound(self._h))
        self.cap = self.bound if cap is None else int(cap)

    def free(self) -> None:
        if self._h is not None and self._h.value:
            check_pt(self._destroy(self._h))
        self._h = None
        self._out = self._size = self._pix = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def _buffers(self):
        import torch
        if self._out is None:
            self._out = torch.empty(max(self.cap, 1), dtype=torch.uint8, device="cuda")
            self._size = torch.zeros(1, dtype=torch.int64, device="cuda")
        return self._out, self._size

    def _pixel_buffer(self):
        """Device RGBA8 pixels of the encoder's size (PathTracer.preview_jpeg / preview_png with display=)."""
        import torch
        if self._pix is None:
            self._pix = torch.empty((self.height, self.width, 4), dtype=torch.uint8, device="cuda")
        return self._pix

    def _read(self, stream) -> bytes:
        """The size first, then that many bytes."""
        import torch
        if stream is not None:   # (a copy on torch's stream does not wait for another stream's encode)
            (stream if hasattr(stream, "synchronize") else torch.cuda.ExternalStream(int(stream))).synchronize()
        size = int(self._size.cpu()[0])
        if size < 0:
            raise N.PtError(1, f"the {self._format} file needs {-size} bytes, the output buffer holds {self.cap}")
        return self._out[:size].cpu().numpy().tobytes()

    def encode(self, src, pixel_stride: int | None = None, samples: float | None = None, stream=None) -> bytes:
        """One file.  src: an (H, W, 3 | 4) uint8 array or tensor (RGB8 / RGBA8, alpha ignored), or with
        `samples` an (H, W, 3) float32 accumulator of that many samples; or a device pointer (int) to
        either, pixels with their pixel_stride (3 or 4).  Asynchronous on `stream` up to the copy of the
        size word and then the file's bytes."""
        import torch
        keep = None
        if isinstance(src, int):
            ptr = src
            if samples is None and pixel_stride is None:
                raise ValueError("a device pointer needs pixel_stride (pixels) or samples (an accumulator)")
        else:
            want = torch.float32 if samples is not None else torch.uint8
            t = src if isinstance(src, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(src))
            chans = (3,) if samples is not None else (3, 4)
            if t.dtype != want or t.dim() != 3 or tuple(t.shape[:2]) != (self.height, self.width) or t.shape[2] not in chans:
                raise ValueError(f"source {tuple(t.shape)} {t.dtype}: expected ({self.height}, {self.width}, "
                                 f"{' | '.join(map(str, chans))}) {want}")
            keep = t.contiguous().cuda()
            ptr, pixel_stride = keep.data_ptr(), int(t.shape[2])
        out, size = self._buffers()
        if samples is not None:
            check_pt(self._accum(self._h, C.c_void_p(ptr), float(samples), out.data_ptr(), self.cap, size.data_ptr(),
                                 _stream_ptr(stream)))
        else:
            check_pt(self._pixels(self._h, C.c_void_p(ptr), int(pixel_stride), out.data_ptr(), self.cap, size.data_ptr(),
                                  _stream_ptr(stream)))
        data = self._read(stream)
        del keep
        return data


class JpegEncoder(_Encoder):
    """pt_jpeg_enc: a baseline JPEG encoder on the device; params: a JpegParams (default: quality
    90, 4:2:0)."""

    _format, _params = "JPEG", N.JpegParams

    _entry = staticmethod(lambda L: (L.pt_jpeg_enc_create, L.pt_jpeg_enc_bound, L.pt_jpeg_enc_destroy, L.pt_jpeg_enc_pixels,
                                     L.pt_jpeg_enc_accum))

    def header(self) -> bytes:
        """The file header SOI .. SOS (pt_jpeg_enc_header; no device needed)."""
        n = int(lib().pt_jpeg_enc_header(self._h, None, 0))
        buf = (C.c_uint8 * n)()
        lib().pt_jpeg_enc_header(self._h, buf, n)
        return bytes(buf)


class PngEncoder(_Encoder):
    """pt_png_enc: a PNG encoder on the device; params: a PngParams (default: adaptive filter,
    32 KiB deflate blocks)."""

    _format, _params = "PNG", N.PngParams

    _entry = staticmethod(lambda L: (L.pt_png_enc_create, L.pt_png_enc_bound, L.pt_png_enc_destroy, L.pt_png_enc_pixels,
                                     L.pt_png_enc_accum))


class HdrEncoder(_Encoder):
    """pt_hdr_enc: a Radiance HDR encoder on the device; params: an HdrParams (default: no
    mirror).  Its source is always a float accumulator."""

    _format, _params = "HDR", N.HdrParams

    _entry = staticmethod(lambda L: (L.pt_hdr_enc_create, L.pt_hdr_enc_bound, L.pt_hdr_enc_destroy, None, L.pt_hdr_enc_accum))

    def encode(self, src, samples: float, stream=None) -> bytes:
        """One file.  src: an (H, W, 3) float32 array or tensor of `samples` samples, or a device pointer (int)
        to one."""
        return super().encode(src, samples=float(samples), stream=stream)


def _encode_host(entry, rgb8: np.ndarray, prm, bound) -> bytes:
    """encode_jpeg and encode_png: bound(w, h) is the encoder's bound, restated."""
    img = np.ascontiguousarray(rgb8, dtype=np.uint8)
    if img.ndim != 3 or img.shape[2] not in (3, 4):
        raise ValueError(f"image shape {img.shape}: expected (H, W, 3 | 4)")
    h, w = img.shape[:2]
    out = np.empty(bound(w, h), np.uint8)
    n = C.c_int64(0)
    check_pt(entry(w, h, img.ctypes.data, img.shape[2], C.byref(prm), out.ctypes.data, out.size, C.byref(n)))
    return out[:n.value].tobytes()


def encode_jpeg(rgb8: np.ndarray, quality: int = 90, subsampling="420", mirror_x: bool = False) -> bytes:
    """An (H, W, 3 | 4) uint8 image as a baseline JPEG file, encoded on the device (pt_jpeg_encode_host)."""
    prm = _jpeg_params(quality, subsampling, mirror_x)
    m = 8 if prm.subsampling == N.JPEG_444 else 16
    per = 3 if m == 8 else 6   # blocks of an MCU; pt_jpeg_enc_bound: 208 bytes a block, twice when stuffed
    return _encode_host(lib().pt_jpeg_encode_host, rgb8, prm,
                        lambda w, h: 623 + 2 * (per * ((w + m - 1) // m) * ((h + m - 1) // m) * 208) + 2)


def _exr_channels(channels) -> "C.Array":
    """A ctypes array of pt_exr_channel from ExrChannel objects or (name, type) pairs."""
    items = [c if isinstance(c, N.ExrChannel) else N.ExrChannel(*c) for c in channels]
    return (N.ExrChannel * max(len(items), 1))(*items)


class ExrEncoder(_Encoder):
    """pt_exr_enc: an OpenEXR encoder on the device for `channels` (ExrChannel objects or (name, type)
    pairs, in any order; an encode takes its planes in this order); params: an ExrParams (default: ZIP, no mirror).
    Its source is a list of float planes."""

    _format, _params = "EXR", N.ExrParams

    def __init__(self, width: int, height: int, channels, params=None, cap: int | None = None):
        self.width, self.height = int(width), int(height)
        self._h = C.c_void_p()
        self._out = self._size = self._pix = None
        L = lib()
        self._destroy = L.pt_exr_enc_destroy
        self.channels = list(channels)
        prm = params if params is not None else N.ExrParams.default()
        check_pt(L.pt_exr_enc_create(self.width, self.height, _exr_channels(self.channels), len(self.channels), C.byref(prm),
                                     C.byref(self._h)))
        self.bound = int(L.pt_exr_enc_bound(self._h))
        self.cap = self.bound if cap is None else int(cap)

    def header(self) -> bytes:
        """The file from its magic number through the header's final zero byte (pt_exr_enc_header; no device needed)."""
        n = int(lib().pt_exr_enc_header(self._h, None, 0))
        buf = (C.c_uint8 * n)()
        lib().pt_exr_enc_header(self._h, buf, n)
        return bytes(buf)

    def encode(self, planes, strides=None, divisors=None, stream=None) -> bytes:
        """One file.  planes: per channel, in creation order, an array or tensor of 4-byte elements (float32, or
        uint32 / int32 for a UINT channel) that holds the pixel p at element p * stride, or a device pointer (int) to
        one; the same object may be given for several channels.  strides, divisors: per channel, default 1."""
        import torch
        n = len(self.channels)
        if len(planes) != n:
            raise ValueError(f"{len(planes)} planes for {n} channels")
        strides = [1] * n if strides is None else [int(s) for s in strides]
        divisors = [1.0] * n if divisors is None else [float(d) for d in divisors]
        keep, arr = {}, (N.ExrPlane * n)()
        for k, src in enumerate(planes):
            if isinstance(src, int):
                ptr = src
            else:
                if id(src) not in keep:
                    if not isinstance(src, torch.Tensor) and np.asarray(src).dtype.itemsize != 4:
                        raise ValueError(f"plane {k}: {np.asarray(src).dtype}, expected 4-byte elements")
                    t = src if isinstance(src, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(src).view(np.int32))
                    need = (self.width * self.height - 1) * strides[k] + 1
                    if t.element_size() != 4 or t.numel() < need:
                        raise ValueError(f"plane {k}: {tuple(t.shape)} {t.dtype}, expected at least {need} 4-byte elements")
                    keep[id(src)] = t.contiguous().cuda()
                ptr = keep[id(src)].data_ptr()
            arr[k] = N.ExrPlane(ptr, strides[k], divisors[k])
        out, size = self._buffers()
        check_pt(lib().pt_exr_enc_planes(self._h, arr, out.data_ptr(), self.cap, size.data_ptr(), _stream_ptr(stream)))
        data = self._read(stream)
        del keep
        return data


_EXR_COMPRESSION = {"none": N.EXR_NONE, "zips": N.EXR_ZIPS, "zip": N.EXR_ZIP}


def encode_exr(channels: dict, half=(), compression="zip", mirror_x: bool = False) -> bytes:
    """{name: (H, W) float32 or uint32 array} as an OpenEXR file written on the device (pt_exr_encode_host): a float32
    array is a FLOAT channel, or HALF when its name is in `half`; a uint32 (or int32) array is a UINT channel."""
    names = list(channels)
    arrs = [np.ascontiguousarray(channels[k]) for k in names]
    if not arrs or any(a.ndim != 2 or a.shape != arrs[0].shape or a.dtype.itemsize != 4 for a in arrs):
        raise ValueError("encode_exr: (H, W) arrays of one shape, float32 or uint32")
    h, w = arrs[0].shape
    types = [N.EXR_UINT if a.dtype.kind in "ui" else (N.EXR_HALF if k in half else N.EXR_FLOAT) for k, a in zip(names, arrs)]
    prm = N.ExrParams.default()
    comp = _EXR_COMPRESSION.get(compression, compression)
    if comp not in _EXR_COMPRESSION.values():
        raise ValueError(f"compression {compression!r}: 'none', 'zips' or 'zip'")
    prm.compression, prm.mirror_x = comp, int(bool(mirror_x))
    chans = _exr_channels(list(zip(names, types)))
    ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
    nchunks = -(-h // (16 if comp == N.EXR_ZIP else 1))
    # pt_exr_enc_bound, with room for the largest header
    out = np.empty(1280 + 16 * nchunks + h * w * sum(2 if t == N.EXR_HALF else 4 for t in types), np.uint8)
    n = C.c_int64(0)
    check_pt(lib().pt_exr_encode_host(w, h, chans, len(arrs), ptrs, None, None, C.byref(prm), out.ctypes.data, out.size,
                                      C.byref(n)))
    return out[:n.value].tobytes()


def exr_ctx_channels(layers: int, half: int = 0) -> list:
    """pt_exr_ctx_channels: the (name, type) pairs of a render context's `layers` (a mask of EXR_BEAUTY .. EXR_ID), HALF
    for the layers of `half` that may be."""
    out, n = (N.ExrChannel * 16)(), C.c_int32(0)
    check_pt(lib().pt_exr_ctx_channels(int(layers), int(half), out, C.byref(n)))
    return [(out[k].name.decode(), int(out[k].type)) for k in range(n.value)]


def _png_params(filter=None, block_bytes: int | None = None, conv: int | None = None, mirror_x: bool = False) -> "N.PngParams":
    p = N.PngParams.default()
    if filter is not None:
        p.filter = int(filter)
    if block_bytes is not None:
        p.block_bytes = int(block_bytes)
    if conv is not None:
        p.conv = int(conv)
    p.mirror_x = int(bool(mirror_x))
    return p


def encode_png(rgb8: np.ndarray, filter=None, block_bytes: int | None = None, mirror_x: bool = False) -> bytes:
    """An (H, W, 3 | 4) uint8 image as an 8-bit RGB PNG file, written on the device (pt_png_encode_host)."""
    prm = _png_params(filter, block_bytes, None, mirror_x)

    def bound(w, h):   # pt_png_enc_bound
        n_f = h * (1 + 3 * w)
        return (9 * n_f + 10 * -(-n_f // max(prm.block_bytes, 1)) + 7) // 8 + 63
    return _encode_host(lib().pt_png_encode_host, rgb8, prm, bound)


class DisplayTransform:
    """pt_display: the display transform on the device for (height, width) accumulators; params: a
    DisplayParams (default: pt_tonemap's conversion without its mirror).  meter / apply / frame take an
    (H, W, 3) float32 array or tensor of `samples` samples, or a device pointer (int) to one."""

    def __init__(self, width: int, height: int, params: "N.DisplayParams | None" = None):
        self.width, self.height = int(width), int(height)
        self._h = C.c_void_p()
        prm = params if params is not None else N.DisplayParams.default()
        self.automatic = prm.exposure_mode == N.DISPLAY_AUTO
        check_pt(lib().pt_display_create(self.width, self.height, C.byref(prm), C.byref(self._h)))

    def free(self) -> None:
        if self._h is not None and self._h.value:
            check_pt(lib().pt_display_destroy(self._h))
        self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def _source(self, src):
        """(device pointer, what keeps it alive)."""
        import torch
        if isinstance(src, int):
            return src, None
        t = src if isinstance(src, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(src))
        if t.dtype != torch.float32 or tuple(t.shape) != (self.height, self.width, 3):
            raise ValueError(f"source {tuple(t.shape)} {t.dtype}: expected ({self.height}, {self.width}, 3) torch.float32")
        keep = t.contiguous().cuda()
        return keep.data_ptr(), keep

    def meter(self, src, samples: float, stream=None) -> None:
        """pt_display_meter: the histogram of src / samples and the exposure state's step; asynchronous."""
        ptr, keep = self._source(src)
        check_pt(lib().pt_display_meter(self._h, C.c_void_p(ptr), float(samples), _stream_ptr(stream)))
        if keep is not None:
            self._wait(stream)

    def _wait(self, stream) -> None:
        import torch
        if stream is None:   # (the null stream: not torch's current one)
            torch.cuda.synchronize()
        else:
            (stream if hasattr(stream, "synchronize") else torch.cuda.ExternalStream(int(stream))).synchronize()

    def _bytes(self, entry, src, samples: float, dst_ptr, pixel_stride: int, stream):
        import torch
        ptr, keep = self._source(src)
        out = None
        if dst_ptr is None:
            out = torch.empty((self.height, self.width, int(pixel_stride)), dtype=torch.uint8, device="cuda")
            dst_ptr = out.data_ptr()
        check_pt(entry(self._h, C.c_void_p(ptr), float(samples), C.c_void_p(int(dst_ptr)), int(pixel_stride), _stream_ptr(stream)))
        if out is None and keep is None:
            return None   # (device to device: asynchronous)
        self._wait(stream)
        return out.cpu().numpy() if out is not None else None

    def apply(self, src, samples: float, dst_ptr: int | None = None, pixel_stride: int = 3, stream=None):
        """pt_display_apply: the bytes to the device pointer dst_ptr (asynchronous when src is a pointer too), or
        without one returned as an (H, W, pixel_stride) uint8 array."""
        return self._bytes(lib().pt_display_apply, src, samples, dst_ptr, pixel_stride, stream)

    def frame(self, src, samples: float, dst_ptr: int | None = None, pixel_stride: int = 3, stream=None):
        """pt_display_frame: meter, then apply."""
        return self._bytes(lib().pt_display_frame, src, samples, dst_ptr, pixel_stride, stream)

    def reset(self, stream=None) -> None:
        """The next metering jumps to its target (pt_display_reset)."""
        check_pt(lib().pt_display_reset(self._h, _stream_ptr(stream)))

    def info(self) -> dict:
        """pt_display_info (synchronous): hist (257 uint32, as last resolved; [256]: the uncounted pixels), e (the
        exposure in 1/256 octave), mult (the multiplier apply uses) and metered."""
        hist = np.zeros(257, np.uint32)
        e, mult, metered = C.c_int32(), C.c_float(), C.c_int32()
        check_pt(lib().pt_display_info(self._h, hist.ctypes.data, C.byref(e), C.byref(mult), C.byref(metered)))
        return {"hist": hist, "e": int(e.value), "mult": float(mult.value), "metered": int(metered.value)}


def display_tables() -> dict:
    """pt_display_tables (no device): srgb (256 float32 thresholds, [0] unused), pow2 (256 float32) and hable_white."""
    srgb, pow2 = np.zeros(256, np.float32), np.zeros(256, np.float32)
    hw = C.c_float()
    lib().pt_display_tables(srgb.ctypes.data, pow2.ctypes.data, C.byref(hw))
    return {"srgb": srgb, "pow2": pow2, "hable_white": np.float32(hw.value)}


def display_transform(acc: np.ndarray, samples: float, params: "N.DisplayParams | None" = None, pixel_stride: int = 3) -> np.ndarray:
    """An (H, W, 3) float32 host accumulator of `samples` samples through the display transform on the device
    (pt_display_host; auto mode meters this one image) -> (H, W, pixel_stride) uint8."""
    img = np.ascontiguousarray(acc, dtype=np.float32)
    if img.ndim != 3 or img.shape[2] != 3:
        raise ValueError(f"image shape {img.shape}: expected (H, W, 3)")
    prm = params if params is not None else N.DisplayParams.default()
    out = np.empty((img.shape[0], img.shape[1], int(pixel_stride)), np.uint8)
    check_pt(lib().pt_display_host(img.shape[1], img.shape[0], img.ctypes.data, float(samples), C.byref(prm), out.ctypes.data,
                                   int(pixel_stride)))
    return out


class Bloom:
    """pt_bloom: bloom on the device for (height, width) accumulators; params: a BloomParams (default:
    threshold 1, strength 0.25, spread 0.75, levels from the size).  apply takes an (H, W, 3) float32 array or tensor
    of `samples` samples, or a device pointer (int) to one; its output is an accumulator of as many samples."""

    def __init__(self, width: int, height: int, params: "N.BloomParams | None" = None):
        self.width, self.height = int(width), int(height)
        self._h = C.c_void_p()
        self._buf = None
        prm = params if params is not None else N.BloomParams.default()
        check_pt(lib().pt_bloom_create(self.width, self.height, C.byref(prm), C.byref(self._h)))

    def free(self) -> None:
        if self._h is not None and self._h.value:
            check_pt(lib().pt_bloom_destroy(self._h))
        self._h = None
        self._buf = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    _source, _wait = DisplayTransform._source, DisplayTransform._wait

    def _buffer(self):
        """The device accumulator the object keeps for its output (PathTracer's bloom= arguments)."""
        import torch
        if self._buf is None:
            self._buf = torch.empty((self.height, self.width, 3), dtype=torch.float32, device="cuda")
        return self._buf

    def apply(self, src, samples: float, dst_ptr: "int | None" = None, stream=None):
        """pt_bloom_apply: the floats to the device pointer dst_ptr (asynchronous when src is a pointer too; dst_ptr
        may be src's), or without one returned as an (H, W, 3) float32 array."""
        import torch
        ptr, keep = self._source(src)
        out = None
        if dst_ptr is None:
            out = torch.empty((self.height, self.width, 3), dtype=torch.float32, device="cuda")
            dst_ptr = out.data_ptr()
        check_pt(lib().pt_bloom_apply(self._h, C.c_void_p(ptr), float(samples), C.c_void_p(int(dst_ptr)), _stream_ptr(stream)))
        if out is None and keep is None:
            return None   # (device to device: asynchronous)
        self._wait(stream)
        return out.cpu().numpy() if out is not None else None

    def info(self) -> dict:
        """pt_bloom_info (no device): levels (K) and the widths and heights of the levels 1 .. K."""
        k, w, h = C.c_int32(), (C.c_int32 * 12)(), (C.c_int32 * 12)()
        check_pt(lib().pt_bloom_info(self._h, C.byref(k), w, h))
        return {"levels": int(k.value), "widths": [int(v) for v in w[:k.value]], "heights": [int(v) for v in h[:k.value]]}


def bloom(acc: np.ndarray, samples: float, params: "N.BloomParams | None" = None) -> np.ndarray:
    """An (H, W, 3) float32 host accumulator of `samples` samples through the bloom on the device (pt_bloom_host) ->
    (H, W, 3) float32, an accumulator of as many samples."""
    img = np.ascontiguousarray(acc, dtype=np.float32)
    if img.ndim != 3 or img.shape[2] != 3:
        raise ValueError(f"image shape {img.shape}: expected (H, W, 3)")
    prm = params if params is not None else N.BloomParams.default()
    out = np.empty_like(img)
    check_pt(lib().pt_bloom_host(img.shape[1], img.shape[0], img.ctypes.data, float(samples), C.byref(prm), out.ctypes.data))
    return out


def tonemap(image: np.ndarray, samples: float) -> np.ndarray:
    """saveImage + Image::savePNG pixel math (x-mirrored, clamp, x255, truncation) -> (H, W, 3) uint8."""
    img = np.ascontiguousarray(image, dtype=np.float32)
    H, W = img.shape[0], img.shape[1]
    out = np.empty((H, W, 3), dtype=np.uint8)
    check_pt(lib().pt_tonemap(img.ctypes.data, W, H, float(samples), out.ctypes.data))
    return out


def save_image(path: str, image: np.ndarray, samples: float) -> str:
    img = np.ascontiguousarray(image, dtype=np.float32)
    check_pt(lib().pt_save_png(str(path).encode(), img.ctypes.data, img.shape[1], img.shape[0], float(samples)))
    return str(path)


def encode_hdr(image: np.ndarray, samples: float) -> bytes:
    """Image::saveHDR file bytes (Radiance RGBE, stb_image_write's run-length coding)."""
    img = np.ascontiguousarray(image, dtype=np.float32)
    n = C.c_int64(0)
    check_pt(lib().pt_encode_hdr(img.ctypes.data, img.shape[1], img.shape[0], float(samples), None, 0, C.byref(n)))
    buf = (C.c_uint8 * n.value)()
    check_pt(lib().pt_encode_hdr(img.ctypes.data, img.shape[1], img.shape[0], float(samples), buf, n.value,
                                 C.byref(n)))
    return bytes(buf)


def encode_hdr_device(image: np.ndarray, samples: float, mirror_x: bool = True) -> bytes:
    """encode_hdr's file written on the device (pt_hdr_encode_host); mirror_x=False keeps the array's columns."""
    img = np.ascontiguousarray(image, dtype=np.float32)
    if img.ndim != 3 or img.shape[2] != 3:
        raise ValueError(f"image shape {img.shape}: expected (H, W, 3)")
    h, w = img.shape[:2]
    prm = N.HdrParams.default()
    prm.mirror_x = int(bool(mirror_x))
    flat = w < 8 or w >= 32768   # pt_hdr_enc_bound, with room for the header
    out = np.empty(160 + (4 * w * h if flat else h * (4 + 4 * (w + (w + 127) // 128))), np.uint8)
    n = C.c_int64(0)
    check_pt(lib().pt_hdr_encode_host(w, h, img.ctypes.data, float(samples), C.byref(prm), out.ctypes.data, out.size,
                                      C.byref(n)))
    return out[:n.value].tobytes()


def save_image_hdr(path: str, image: np.ndarray, samples: float) -> str:
    img = np.ascontiguousarray(image, dtype=np.float32)
    check_pt(lib().pt_save_hdr(str(path).encode(), img.ctypes.data, img.shape[1], img.shape[0], float(samples)))
    return str(path)


def render(scene_path: str, iterations: int | None = None, out_dir: str | None = None,
           gui: GuiDataContainer | None = None, denoise: "bool | str" = False,
           adaptive: "N.AdaptiveParams | bool | None" = None, adaptive_every: int = 4):
    """Headless runCuda loop (main.cpp:114-168): ITERATIONS passes, then saveImage.  denoise=True
    additionally saves FILE.<UTC>.<spp>samp.denoised.png (PathTracer.denoised); the raw PNG is the same.
    denoise="variance" tracks the variance (an update after every pass; the passes and the raw PNG are
    the same) and saves FILE.<UTC>.<spp>samp.denoised-var.png (PathTracer.denoised_variance, or the
    plain filter when there are fewer than 2 batches).

    adaptive (AdaptiveParams, or True for the defaults): adaptive sampling — an update
    after every pass, a selection of the active 64-pixel blocks every `adaptive_every` passes, until no
    block is active or ITERATIONS passes are done.  Returns (accumulator, path, report) then; report holds
    the resolved image (accumulator / the samples of the pixel's block), samples_per_block, the
    active_blocks after every selection, passes and the segments traced.  Saves the resolved image as
    FILE.<UTC>.<spp>samp.adaptive.png and, with denoise="variance", its variance-filtered version as
    ....adaptive.denoised-var.png (no raw PNG: the accumulator's pixels hold different sample counts)."""
    if denoise not in (False, True, "variance"):
        raise ValueError(f"denoise must be False, True or 'variance', not {denoise!r}")
    scene = Scene(scene_path)
    st = scene.state()
    iters = iterations if iterations is not None else st.iterations
    pt = PathTracer(scene, gui)
    if adaptive is not None and adaptive is not False:
        return _render_adaptive(pt, st, iters, out_dir, denoise, adaptive, adaptive_every)
    if denoise == "variance":
        pt.track_variance(True)
    for it in range(1, iters + 1):
        pt.render_pass(it)
        if denoise == "variance":
            pt.variance_update()
    img = pt.image()
    path = None
    if out_dir is not None:
        stamp = time.strftime("%Y-%m-%d_%H-%M-%Sz", time.gmtime())
        path = str(Path(out_dir) / f"{st.imageName}.{stamp}.{iters}samp.png")
        save_image(path, img, iters)
        if denoise == "variance":
            dn = pt.denoised_variance(iters) if pt.variance_info()["batches"] >= 2 else pt.denoised(iters)
            save_image(path[:-len(".png")] + ".denoised-var.png", dn, 1.0)
        elif denoise:
            save_image(path[:-len(".png")] + ".denoised.png", pt.denoised(iters), 1.0)
    pt.free()
    return img, path


def _render_adaptive(pt: PathTracer, st, iters: int, out_dir, denoise, adaptive, every: int):
    if every < 1:
        raise ValueError("adaptive_every must be >= 1")
    if denoise is True:
        raise ValueError("adaptive rendering filters with denoise='variance' only")
    prm = N.AdaptiveParams.default() if adaptive is True else adaptive
    pt.adaptive(True)
    active, passes = [], 0
    for it in range(1, iters + 1):
        pt.render_pass(it)
        pt.adaptive_update()
        passes = it
        if it % every == 0 and it < iters:
            sel = pt.adaptive_select(prm)
            active.append(sel["active_blocks"])
            if sel["active_blocks"] == 0:
                break
    img = pt.image()
    resolved = pt.adaptive_image()
    state = pt.adaptive_state()
    report = {"resolved": resolved, "samples_per_block": state["nb"].astype(np.int64) * pt.spp, "active_blocks": active,
              "passes": passes, "segments": pt.stats()["segments"]}
    path = None
    if out_dir is not None:
        stamp = time.strftime("%Y-%m-%d_%H-%M-%Sz", time.gmtime())
        path = str(Path(out_dir) / f"{st.imageName}.{stamp}.{passes}samp.adaptive.png")
        save_image(path, resolved, 1.0)
        if denoise == "variance":
            save_image(path[:-len(".png")] + ".denoised-var.png", pt.adaptive_image(N.DenoiseVarParams.default()), 1.0)
    pt.free()
    return img, path, report


# ---- the reference's global-state API (pathtrace.h:6-9) ------------------------------------
_GLOBAL: dict = {"gui": None, "ctx": None}


def InitDataContainer(gui: GuiDataContainer) -> None:  # noqa: N802
    _GLOBAL["gui"] = gui
    if _GLOBAL["ctx"] is not None:
        _GLOBAL["ctx"].set_flags(gui)


def pathtraceInit(scene: Scene) -> None:  # noqa: N802
    pathtraceFree()
    _GLOBAL["ctx"] = PathTracer(scene, _GLOBAL["gui"])


def pathtraceFree() -> None:  # noqa: N802
    if _GLOBAL["ctx"] is not None:
        _GLOBAL["ctx"].free()
    _GLOBAL["ctx"] = None


def pathtrace(pbo_ptr: int | None, frame: int, iteration: int) -> None:
    """One iteration; writes the RGBA preview into pbo_ptr (device) when given."""
    ctx = _GLOBAL["ctx"]
    if ctx is None:
        raise RuntimeError("pathtraceInit() was not called")
    if _GLOBAL["gui"] is not None:
        ctx.set_flags(_GLOBAL["gui"])
    ctx.render_pass(iteration)
    if pbo_ptr:
        ctx.preview_rgba(iteration, pbo_ptr)
