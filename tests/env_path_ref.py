"""path_ref's replay with an environment (a helper, not collected by pytest).

replay_env() restates path_ref.replay's bounce loop with the one term DESIGN.md §19 adds: a path whose ray
meets nothing ends with c * L(d) instead of 0, L being env_ref.lookup in the replay's dtype, and 0 for a
direction that is not finite (glm::refract's NaN ray).  Nothing else differs: no draw is added, the routes
and the rules that exclude a pixel are path_ref's.  path_ref's pieces are imported, not copied.

VARIANTS: one deliberate error each, for the tests that show the comparison has teeth:
  env_transpose   the map read with its axes swapped
  env_no_rot      the rotation dropped (identity)
  env_nan_L       a NaN ray shaded with L of the last finite direction instead of 0

open_lantern() is path_ref.lantern with part of the tile shell removed (REMOVED) and part made non-emissive
(DARK): the camera looks out through the missing -z, +y and -x walls, the +x wall only scatters.
"""
import json
import shutil
from pathlib import Path

import numpy as np

from cuda_pathtracer_amd import Scene

import env_ref as E
import mesh_ref as M
import path_ref as R
import rng_ref
from path_ref import (DIFFUSE, EMIT, EXIT, FRESNEL, LIFT, LUMA, MARGIN, MIRROR, MISS, NAN_RAY, REFRACT, REFRACT_NAN,  # noqa: F401
                      RR_KILL, RR_LIVE, TEX, EDGE_EPS, F, _glm_max, _hemisphere, _raygen, _tex_color)

VARIANTS = ("env_transpose", "env_no_rot", "env_nan_L")
SPECULAR = MIRROR | REFRACT | FRESNEL

# tiles of lantern(k=2) by wall: -x 0..3, +x 4..7, -y 8..11, +y 12..15, -z 16..19, +z 20..23
REMOVED = tuple(range(0, 4)) + tuple(range(12, 16)) + tuple(range(16, 20))
DARK = tuple(range(4, 8))
ENV_N = 8
ENV_SCALE = 0.37
ENV_ROTATE = (25.0, -40.0, 15.0)


def env_texels(n=ENV_N):
    """(n, n, 3) float32, every texel its own colour, none dark (as the tiles are)."""
    i = np.arange(n * n).reshape(n, n)
    return np.stack([0.3 + 1.7 * ((7 * i) % 23) / 23, 0.3 + 1.7 * ((5 * i) % 29) / 29, 0.3 + 1.7 * ((3 * i) % 31) / 31],
                    -1).astype(np.float32)


# A narrow view of the glass cube of ior 1.5 along one of its body diagonals, 3 units from its centre: the three
# faces it shows are met at 54.7 degrees, beyond the 41.8 degrees past which glm::refract(d, n, 1.5) has k < 0, so
# nearly every camera path that is not Fresnel-reflected goes on as a NaN ray.
GLASS_CAMERA = dict(FOVY=8.0, EYE=[0.63, 4.4, -1.31], LOOKAT=[-1.0, 4.6, 1.2])


def open_lantern(tmp, glass_view=False, **kw):
    """path_ref.lantern(tmp, **kw) opened: (path of the JSON scene, textures).  glass_view: GLASS_CAMERA."""
    path, textures = R.lantern(tmp, **kw)
    src = Path(path).parent
    dst = src.with_name(src.name + ("_open_glass" if glass_view else "_open"))
    shutil.copytree(src, dst)
    spec = json.loads(Path(path).read_text())
    if glass_view:
        spec["Camera"].update(GLASS_CAMERA)
    gone = {f"t{t:03d}" for t in REMOVED}
    spec["Objects"] = [o for o in spec["Objects"] if o["MATERIAL"] not in gone]
    for t in DARK:
        spec["Materials"][f"t{t:03d}"]["EMITTANCE"] = 0.0
    out = dst / "lantern.json"
    out.write_text(json.dumps(spec))
    return str(out), textures


def replay_env(scene, textures, env, iters, depth, flags, rank=0, world=1, mode="bvh", use_bbox=False, dt=np.float64,
               variant=None):
    """path_ref.replay with the environment env = dict(map (n + 2, n + 2, 4) padded, scale, rotate) or None
    (then it is path_ref.replay's result).  Returns replay's dict and "env" (len(iters), depth, rows, W):
    where a path ended in the environment with a finite direction."""
    assert variant is None or variant in VARIANTS
    fl = flags
    cam, geoms = scene.camera(), scene.geoms()
    tris = M.triangle_table(scene)
    mats = scene.materials()
    color = np.array([list(m.color) for m in mats], F).astype(dt)
    spec = np.array([list(m.spec_color) for m in mats], F).astype(dt)
    refl = np.array([m.has_reflective for m in mats], F).astype(dt)
    refr = np.array([m.has_refractive for m in mats], F) != 0
    ior = np.array([m.ior for m in mats], F).astype(dt)
    emit = np.array([m.emittance for m in mats], F).astype(dt)
    texid = np.array([m.texture_id for m in mats], np.int64)
    if env is not None:
        rot = E.rotation((0.0, 0.0, 0.0) if variant == "env_no_rot" else env["rotate"])

        def radiance(dirs):
            return E.lookup(env["map"], env["scale"], rot, dirs, dt, transpose=variant == "env_transpose")
    W, Hh = cam.res[0], cam.res[1]
    ys = np.arange(rank, Hh, world)
    y, x = (a.reshape(-1) for a in np.meshgrid(ys, np.arange(W), indexing="ij"))
    pixel = x + y * W
    n = len(pixel)
    image = np.zeros((n, 3), dt)
    risky = np.zeros(n, bool)
    route = np.zeros((len(iters), depth, n), np.int32)
    hit_geom = np.full((len(iters), depth, n), -1, np.int32)
    hit_risky = np.zeros((len(iters), depth, n), bool)
    env_end = np.zeros((len(iters), depth, n), bool)
    with np.errstate(all="ignore"):
        for ii, it in enumerate(iters):
            o, d, rk = _raygen(cam, x, y, rng_ref.u01_table(it, pixel, depth, 4).astype(dt), fl, dt, None)
            risky |= rk
            c = np.ones((n, 3), dt)
            last = d.copy()                                               # the last finite direction of a path
            ix = np.arange(n)
            for b in range(depth):
                if ix.size == 0:
                    break
                remaining = depth - b
                h = M.mesh_hit_ref(tris, geoms, o[ix], d[ix], dt, mode, EDGE_EPS, use_bbox)
                nan_ray = ~np.isfinite(d[ix]).all(-1)
                assert (h["mat"][nan_ray] < 0).all()
                hit_risky[ii, b, ix] = ~h["keep"] & ~nan_ray
                risky[ix] |= hit_risky[ii, b, ix]
                got = h["mat"] >= 0
                hit_geom[ii, b, ix] = h["geom"]
                route[ii, b, ix[~got]] = MISS
                route[ii, b, ix[nan_ray]] |= NAN_RAY
                # the miss: c * L(d), 0 for a direction that is not finite
                sky = ix[~got & ~nan_ray]
                if env is None:
                    c[ix[~got]] = 0
                else:
                    c[sky] = c[sky] * radiance(d[sky])
                    env_end[ii, b, sky] = True
                    dead = ix[~got & nan_ray]
                    c[dead] = c[dead] * radiance(last[dead]) if variant == "env_nan_L" else 0
                mat = np.where(got, h["mat"], 0)
                lit = got & (emit[mat] > 0)
                c[ix[lit]] = c[ix[lit]] * (color[mat[lit]] * emit[mat[lit]][:, None])
                route[ii, b, ix[lit]] = EMIT
                s = got & ~lit
                j, m = ix[s], mat[s]
                if j.size == 0:
                    ix = j
                    continue
                u = rng_ref.u01_table(it, pixel[j], remaining, 4).astype(dt)
                nrm, dd, t = h["n"][s], d[j], h["t"][s]
                point = o[j] + (t - dt(LIFT))[:, None] * R.R._normalize(dd, dt)
                new_o = point + dt(LIFT) * nrm
                alb = color[m].copy()
                code = np.zeros(len(j), np.int32)
                for tid in np.unique(texid[m]):
                    if tid >= 0:
                        w = texid[m] == tid
                        alb[w], near = _tex_color(textures[tid], h["uv"][s][w], dt)
                        risky[j[w]] |= near
                        code[w] |= TEX
                cj = c[j] * alb
                glass = refr[m]
                eta = ior[m]
                r0 = ((eta - dt(1)) * (eta - dt(1))) / ((eta + dt(1)) * (eta + dt(1)))
                X = dt(1) - np.abs(R.R._dot(dd, nrm))
                X2 = X * X
                fres = r0 + (dt(1) - r0) * ((X * X2) * X2)
                u0 = u[:, 0]
                through = glass & (fres < u0)
                bounce = glass & ~(fres < u0)
                mirror = ~glass & (u0 < refl[m])
                diffuse = ~glass & ~mirror
                risky[j] |= glass & (np.abs(fres - u0) < MARGIN)
                dv = R.R._dot(nrm, dd)
                k = dt(1) - eta * eta * (dt(1) - dv * dv)
                d_refr = (eta[:, None] * dd - (eta * dv + np.sqrt(k))[:, None] * nrm) * (k >= 0).astype(dt)[:, None]
                risky[j] |= through & (np.abs(k) < MARGIN)
                d_refl = dd - nrm * R.R._dot(nrm, dd)[:, None] * dt(2)
                d_hemi, near = _hemisphere(nrm, u[:, 1], u[:, 2], dt, None)
                risky[j] |= diffuse & near
                new_d = np.where(through[:, None], d_refr, np.where(diffuse[:, None], d_hemi, d_refl))
                cj = np.where(through[:, None], cj * color[m], np.where(diffuse[:, None], cj, cj * spec[m]))
                if not fl["singleAlbedo"]:
                    cj = cj * color[m]
                code |= np.where(through, np.where(k >= 0, REFRACT, REFRACT_NAN),
                                 np.where(bounce, FRESNEL, np.where(mirror, MIRROR, DIFFUSE)))
                draws = np.where(diffuse, 3, 1)
                alive = np.ones(len(j), bool)
                if remaining - 1 == 0:
                    cj[:] = 0
                    alive[:] = False
                    code |= EXIT
                elif fl["russianRoulette"] and b + 1 > 3:
                    luma = (cj[:, 0] * dt(LUMA[0]) + cj[:, 1] * dt(LUMA[1])) + cj[:, 2] * dt(LUMA[2])
                    q = _glm_max(dt(F(0.05)), dt(1) - luma)
                    ur = u[np.arange(len(j)), draws]
                    risky[j] |= np.abs(ur - q) < MARGIN
                    kill = ur < q
                    cj = np.where(kill[:, None], dt(0), cj / (dt(1) - q)[:, None])
                    alive = ~kill
                    code |= np.where(kill, RR_KILL, RR_LIVE)
                c[j], o[j], d[j] = cj, new_o, new_d
                fin = np.isfinite(new_d).all(-1)
                last[j[fin]] = new_d[fin]
                route[ii, b, j] = code
                ix = j[alive]
            assert ix.size == 0
            image = image + c
    assert image.dtype == dt
    rows = len(ys)
    shape = (len(iters), depth, rows, W)
    return {"image": image.reshape(rows, W, 3), "keep": ~risky.reshape(rows, W), "route": route.reshape(shape),
            "geom": hit_geom.reshape(shape), "hit_risky": hit_risky.reshape(shape), "env": env_end.reshape(shape)}


def env_shares(ref):
    """Over the kept pixels: (share with a path that ends in the environment, share that reaches it only after
    a mirror or glass bounce: some path does so through one, and no camera ray of the pixel leaves directly)."""
    keep = ref["keep"]
    env, rt = ref["env"], ref["route"]
    any_env = env.any(axis=(0, 1))
    spec_before = np.cumsum((rt & SPECULAR) != 0, axis=1) - ((rt & SPECULAR) != 0) > 0     # a specular bounce earlier
    via = (env & spec_before).any(axis=(0, 1)) & ~env[:, 0].any(axis=0)
    return float(any_env[keep].mean()), float(via[keep].mean())


# ---- the replays, cases and constants that tests/test_env_cpu.py and tests/test_env_gpu.py share ----------------------
GOLDEN_HDR = Path(__file__).resolve().parent / "golden" / "env_sky.hdr"
LENS = dict(aperture=0.15, focal_len=6.5)
PLAIN = dict(ssaa=False, dof=False)
# replay -> (lantern arguments, glass view, depth, the replay's flags)
REPLAYS = {
    "open_d2": (dict(k=2), False, 2, PLAIN),
    "open_d8": (dict(k=2), False, 8, LENS),
    "open_mats": (dict(k=2, extra_materials=100), False, 8, LENS),
    "open_mesh": (dict(k=2, mesh=True), False, 4, LENS),
    "glass_d2": (dict(k=2), True, 2, PLAIN),
}
# D_c as measured (the float32-vs-float64 deviation of the same replay over the kept pixels, the largest over the
# replay's iteration sets and tiles; tests/test_env_cpu.py measures it again): the values to four digits, the
# fourth rounded up.  The table in tests/test_env_gpu.py's header says what they belong to.
D = {"open_d2": 3.005e-04, "open_d8": 4.021e-04, "open_mats": 6.935e-05, "open_mesh": 1.343e-04, "glass_d2": 5.352e-07}
# case -> replay, process environment, further GuiDataContainer attributes, spp, first iteration of every pass, world, and
# what the context must report (expect: lanes; traverse: the BVH walk ran as a kernel of its own, kMeshPre, or did not)
CASES = {
    "open_d2": dict(replay="open_d2"),
    "open_d8": dict(replay="open_d8"),
    "open_d8_spp3": dict(replay="open_d8", spp=3, passes=(5,)),
    "open_d8_lanes2_spp5": dict(replay="open_d8", env=dict(PT_AMD_LANES="2"), spp=5, passes=(3,), lanes=2),
    "open_d8_thrust": dict(replay="open_d8", gui=dict(useThrustPartition=True)),   # (no effect on the fused pipeline: it works)
    "open_d8_world2": dict(replay="open_d8", world=2),
    "open_mats": dict(replay="open_mats", materials_over=128),  # more than kLdsMats materials: kAnalyticGM
    "open_mesh": dict(replay="open_mesh", traverse=True),       # BVH walk ahead of the bounce: kMeshPre
    "open_mesh_inline": dict(replay="open_mesh", env=dict(PT_AMD_MESH_INLINE="1"), traverse=False),
}
TEETH = {"env_transpose": "open_d2", "env_no_rot": "open_d2", "env_nan_L": "glass_d2"}


def case_iterations(case):
    spp = case.get("spp", 1)
    return tuple(it for first in case.get("passes", (1, 7)) for it in range(first, first + spp))


def replay_requests():
    """Every (replay, iterations, rank, world) the cases and the teeth need, each once."""
    out = []
    for case in CASES.values():
        world = case.get("world", 1)
        for rank in range(world):
            req = (case["replay"], case_iterations(case), rank, world)
            if req not in out:
                out.append(req)
    for key in TEETH.values():
        if (key, (1, 7), 0, 1) not in out:
            out.append((key, (1, 7), 0, 1))
    return out


def the_environment():
    return dict(texels=env_texels(), scale=ENV_SCALE, rotate=ENV_ROTATE)


class Replays:
    """The scenes (with their environment set) and the replays of a test module: each computed once."""

    def __init__(self, tmp):
        self.tmp, self.scenes, self.cache = Path(tmp), {}, {}

    def scene(self, key):
        """(Scene with the environment, texel arrays by texture id, path of its JSON file, the replay's env dict)."""
        if key not in self.scenes:
            kw, glass, depth, _ = REPLAYS[key]
            path, textures = open_lantern(self.tmp / key, glass_view=glass, depth=depth, **kw)
            scene = Scene(path)
            env = the_environment()
            scene.set_environment_octa(env["texels"], scale=env["scale"], rotate=env["rotate"])
            got = scene.environment()
            self.scenes[key] = (scene, textures, path, dict(map=got["map"], scale=got["scale"], rotate=got["rotate"]))
        return self.scenes[key]

    def __call__(self, key, iters, rank=0, world=1, dt=np.float64, variant=None):
        req = (key, tuple(iters), rank, world, dt, variant)
        if req not in self.cache:
            scene, textures, _, env = self.scene(key)
            depth, fl = REPLAYS[key][2:]
            self.cache[req] = replay_env(scene, textures, env, tuple(iters), depth, R.default_flags(**fl), rank, world,
                                            "bvh", False, dt, variant)
        return self.cache[req]
