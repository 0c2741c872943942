"""A float64 replay of whole paths (a helper, not collected by pytest).

replay() restates, in plain numpy and in a chosen dtype dt, what the reference does with a path from the
camera to its end, over all pixels of a tile at once:

  generateRayFromCamera                   pathtrace.cu:183-227
  computeIntersections                    pathtrace.cu:230-298, by mesh_ref.mesh_hit_ref (cubes and spheres by
                                          denoise_ref.geom_hit, triangles by brute force, no BVH)
  shadeMaterials                          pathtrace.cu:300-344
  scatterRay, calculateRandomDirectionInHemisphere      interactions.cu:43-85, :3-41
  glm::reflect, glm::refract              glm/detail/func_geometric.inl:176-179, :193-199 (refract's
                                          "* T(k >= 0)" after sqrt(k): a NaN direction when k < 0)
  getPointOnRay                           intersections.h:29-32
  Texture::get_color                      sceneStructs.h:176-189
  finalGather                             pathtrace.cu:347-356

It shares no code with oracle/ or csrc/.  float64 is the yardstick; dt=np.float32 measures the format's own
error.  The uniforms are the reference's own (tests/rng_ref.py: integer-exact, so both dtypes and the
kernels consume the same numbers), keyed by the GLOBAL pixel for shading (pt_flags.rng_key_pixel): a path's
draws depend only on (iteration, pixel, remaining bounces), so the replay follows the kernels' path except
where a rounding error can flip a discrete choice.  Those places are named below, on the replay's own values.

Order of the draws.  Every engine is makeSeededRandomEngine(iter, index, depth) (pathtrace.cu:57-62).
  raygen, engine (iter, pixel, traceDepth)                    pathtrace.cu:197
    1, 2   jitter in x, then in y (SSAA only)                 pathtrace.cu:203, :204
    next   lens radius, then lens angle (DoF only)            pathtrace.cu:214, :215
  shading of the bounce with `remaining` bounces left, a NEW engine (iter, pixel, remaining)   pathtrace.cu:315
  (at the first bounce remaining == traceDepth: the same engine as raygen's, started again)
    refractive material:  1  the Fresnel test R < u           interactions.cu:69
    otherwise:            1  the mirror test u < hasReflective     interactions.cu:77
                          2  up = sqrt(u), 3  around = u * TWO_PI (diffuse only)   interactions.cu:9, :11
    next   the roulette test u < q (roulette on and bounces > 3 only)       pathtrace.cu:335
  An emissive hit and a miss draw nothing.

Constants the reference holds in float32 enter as their float32 values: 0.0001f (the back-off and the lift
of the new origin), PI, TWO_PI, SQRT_OF_ONE_THIRD (utilities.h:12-14), the luma weights (glm::vec3 of double
literals, pathtrace.cu:331), 0.05f, 0.003921568627f, and the flags' aperture and focal distance.

One place follows the project and not the text: get_color computes no bound for a NEGATIVE texel index
(the reference reads in front of the image); kernels and oracle clamp it to 0, and so does the replay.

keep.  A pixel is not kept if any iteration or bounce of its path meets one of these, each decided on the
replay's own values (use the float64 ones):
  * mesh_ref.mesh_hit_ref's rules for the hit (edges, silhouettes, near-tied distances, grazing triangles,
    the culling threshold), with edge_eps = EDGE_EPS = 1e-3;
  * |R - u| < MARGIN of the Fresnel test, |k| < MARGIN of refract (when refraction is taken),
    |u - q| < MARGIN of the roulette test;  MARGIN = 1e-5
  * ||n.x| - sqrt(1/3)| or ||n.y| - sqrt(1/3)| < MARGIN_NORMAL = 1e-4 on a diffuse bounce;
  * a texel coordinate within MARGIN of a texel boundary that changes the texel;
  * |d.z| < MARGIN_LENS = 1e-3 in the lens division.
A path whose direction is NaN after refract is NOT excluded: it misses everything and contributes 0.

Known blind spots: dropping the 0.0001 * n lift of the new origin, or the 1e-4 back-off of the hit point
beyond the first hit, moves a colour by at most 0.03 % on these scenes and is not seen.
"""
import json
from pathlib import Path

import numpy as np

import denoise_ref as R
import mesh_ref as M
import rng_ref

F = np.float32
EDGE_EPS = 1e-3
MARGIN = 1e-5
MARGIN_NORMAL = 1e-4
MARGIN_LENS = 1e-3

PI = F(3.1415926535897932384626422832795028841971)
TWO_PI = F(6.2831853071795864769252867665590057683943)
SQRT_OF_ONE_THIRD = F(0.5773502691896257645091487805019574556476)
LUMA = (F(0.2126), F(0.7152), F(0.0722))
LIFT = F(0.0001)
TEXEL = F(0.003921568627)

# route bits of one bounce (replay()["route"])
(MISS, EMIT, DIFFUSE, MIRROR, REFRACT, REFRACT_NAN, FRESNEL, EXIT, RR_KILL, RR_LIVE, TEX,
 NAN_RAY) = (1 << i for i in range(12))
ROUTE_NAMES = ("miss", "emit", "diffuse", "mirror", "refract", "refract_k<0", "fresnel", "exit", "rr_kill", "rr_live",
               "tex", "nan_ray")
VARIANTS = ("sincos_swap", "up_linear", "xy_order", "jitter_swap", "lens_pi", "inv_ior", "schlick4", "rr_gate")


def route_text(code):
    return "+".join(n for i, n in enumerate(ROUTE_NAMES) if code & (1 << i)) or "-"


def _v3(x, dt):
    return np.asarray(list(x), dt)


def _cross(a, b):
    """glm::cross."""
    return np.stack([a[..., 1] * b[..., 2] - b[..., 1] * a[..., 2], a[..., 2] * b[..., 0] - b[..., 2] * a[..., 0],
                     a[..., 0] * b[..., 1] - b[..., 0] * a[..., 1]], -1)


def _glm_min(a, b):
    return np.where(b < a, b, a)


def _glm_max(a, b):
    return np.where(a < b, b, a)


def _tex_color(px, uv, dt):
    """Texture::get_color for (h, w, 3) uint8 texels: (colour, near a texel boundary)."""
    h, w = px.shape[:2]
    ux, uy = dt(1) * dt(w) * uv[:, 0], dt(1) * dt(h) * (dt(1) - uv[:, 1])
    fx, fy = _glm_min(ux, dt(1) * dt(w) - dt(1)), _glm_min(uy, dt(1) * dt(h) - dt(1))
    X, Y = np.trunc(fx).astype(np.int64), np.trunc(fy).astype(np.int64)      # (int) truncates toward zero
    X, Y = np.maximum(X, 0), np.maximum(Y, 0)                                # (the project's clamp)
    near = np.zeros(len(fx), bool)
    for f, size in ((ux, w), (uy, h)):                                       # the texel changes at 1 .. size - 1
        j = np.rint(f)
        near |= (np.abs(f - j) < MARGIN) & (j >= 1) & (j <= size - 1)
    return dt(TEXEL) * px[Y, X].astype(dt), near


def _raygen(cam, x, y, u, fl, dt, variant):
    """generateRayFromCamera for the pixels (x, y) with their uniforms u (n, 4): (o, d, risky)."""
    W, Hh = cam.res[0], cam.res[1]
    view, up, right = (_v3(v, dt) for v in (cam.view, cam.up, cam.right))
    plx, ply = dt(cam.pixel_length[0]), dt(cam.pixel_length[1])
    ax = x.astype(dt) - dt(W) * dt(0.5)
    ay = y.astype(dt) - dt(Hh) * dt(0.5)
    k = 0
    if fl["ssaa"]:
        jx, jy = (u[:, 1], u[:, 0]) if variant == "jitter_swap" else (u[:, 0], u[:, 1])
        ax, ay, k = ax + jx, ay + jy, 2
    d = R._normalize((view - (right * plx) * ax[:, None]) - (up * ply) * ay[:, None], dt)
    o = np.broadcast_to(_v3(cam.position, dt), d.shape).copy()
    risky = np.zeros(len(x), bool)
    if fl["dof"]:
        r = u[:, k] * dt(F(fl["aperture"]))
        th = u[:, k + 1] * dt(PI) if variant == "lens_pi" else (u[:, k + 1] * dt(2)) * dt(PI)
        lens = np.stack([r * np.cos(th), r * np.sin(th), np.zeros_like(r)], -1)
        risky |= np.abs(d[:, 2]) < MARGIN_LENS
        ft = dt(F(fl["focal_len"])) / np.abs(d[:, 2])
        focus = o + ft[:, None] * d
        o = o + lens
        d = R._normalize(focus - o, dt)
    return o, d, risky


def _hemisphere(n, u_up, u_around, dt, variant):
    """calculateRandomDirectionInHemisphere: (direction, near a threshold of "direction not normal")."""
    up = u_up if variant == "up_linear" else np.sqrt(u_up)
    over = np.sqrt(dt(1) - up * up)
    around = u_around * dt(TWO_PI)
    S = dt(SQRT_OF_ONE_THIRD)
    a, b = (1, 0) if variant == "xy_order" else (0, 1)
    first, second = np.abs(n[:, a]) < S, np.abs(n[:, b]) < S
    dnn = np.zeros_like(n)
    dnn[first, a] = 1
    dnn[~first & second, b] = 1
    dnn[~first & ~second, 2] = 1
    near = (np.abs(np.abs(n[:, 0]) - S) < MARGIN_NORMAL) | (np.abs(np.abs(n[:, 1]) - S) < MARGIN_NORMAL)
    p1 = R._normalize(_cross(n, dnn), dt)
    p2 = R._normalize(_cross(n, p1), dt)
    ca, sa = np.cos(around), np.sin(around)
    if variant == "sincos_swap":
        ca, sa = sa, ca
    return (up[:, None] * n + (ca * over)[:, None] * p1) + (sa * over)[:, None] * p2, near


def default_flags(**kw):
    """The flags replay() reads, with GuiDataContainer's defaults (utilities.h:17-34)."""
    fl = dict(ssaa=True, dof=True, aperture=0.1, focal_len=10.0, russianRoulette=True, singleAlbedo=False)
    assert set(kw) <= set(fl), kw
    fl.update(kw)
    return fl


def replay(scene, textures, iters, depth, flags, rank=0, world=1, mode="bvh", use_bbox=False, dt=np.float64,
           variant=None):
    """The sum over the iterations `iters` of every path of the tile {rows y : y % world == rank}.

    scene: its geoms(), materials(), camera() and triangles() are read; textures: a list of (h, w, 3) uint8
    arrays by texture id; flags: default_flags(); mode / use_bbox: mesh_ref's mesh path; variant: one
    deliberate error (VARIANTS), for the tests that show the replay has teeth.

    Returns dict(image (rows, W, 3) dt; keep (rows, W); route (len(iters), depth, rows, W) int32, the ROUTE
    bits of every bounce; geom (same shape) the geom hit at every bounce, -1 for none; hit_risky (same shape)
    where the hit's own rules call the surface uncertain)."""
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
    with np.errstate(all="ignore"):
        for ii, it in enumerate(iters):
            o, d, rk = _raygen(cam, x, y, rng_ref.u01_table(it, pixel, depth, 4).astype(dt), fl, dt, variant)
            risky |= rk
            c = np.ones((n, 3), dt)
            ix = np.arange(n)
            for b in range(depth):
                if ix.size == 0:
                    break
                remaining = depth - b
                h = M.mesh_hit_ref(tris, geoms, o[ix], d[ix], dt, mode, EDGE_EPS, use_bbox)
                nan_ray = ~np.isfinite(d[ix]).all(-1)
                assert (h["mat"][nan_ray] < 0).all()                      # (every comparison with a NaN fails)
                hit_risky[ii, b, ix] = ~h["keep"] & ~nan_ray
                risky[ix] |= hit_risky[ii, b, ix]
                got = h["mat"] >= 0
                hit_geom[ii, b, ix] = h["geom"]
                route[ii, b, ix[~got]] = MISS
                route[ii, b, ix[nan_ray]] |= NAN_RAY
                c[ix[~got]] = 0
                mat = np.where(got, h["mat"], 0)
                lit = got & (emit[mat] > 0)
                c[ix[lit]] = c[ix[lit]] * (color[mat[lit]] * emit[mat[lit]][:, None])
                route[ii, b, ix[lit]] = EMIT
                s = got & ~lit
                j, m = ix[s], mat[s]
                if j.size == 0:
                    ix = j
                    continue
                # scatterRay
                u = rng_ref.u01_table(it, pixel[j], remaining, 4).astype(dt)
                nrm, dd, t = h["n"][s], d[j], h["t"][s]
                point = o[j] + (t - dt(LIFT))[:, None] * R._normalize(dd, dt)
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
                X = dt(1) - np.abs(R._dot(dd, nrm))
                X2 = X * X
                fres = r0 + (dt(1) - r0) * ((X * X2) * (X if variant == "schlick4" else X2))
                u0 = u[:, 0]
                through = glass & (fres < u0)
                bounce = glass & ~(fres < u0)
                mirror = ~glass & (u0 < refl[m])
                diffuse = ~glass & ~mirror
                risky[j] |= glass & (np.abs(fres - u0) < MARGIN)
                # glm::refract
                dv = R._dot(nrm, dd)
                if variant == "inv_ior":
                    eta = dt(1) / eta
                k = dt(1) - eta * eta * (dt(1) - dv * dv)
                d_refr = (eta[:, None] * dd - (eta * dv + np.sqrt(k))[:, None] * nrm) * (k >= 0).astype(dt)[:, None]
                risky[j] |= through & (np.abs(k) < MARGIN)
                # glm::reflect
                d_refl = dd - nrm * R._dot(nrm, dd)[:, None] * dt(2)
                d_hemi, near = _hemisphere(nrm, u[:, 1], u[:, 2], dt, variant)
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
                elif fl["russianRoulette"] and b + 1 > (2 if variant == "rr_gate" else 3):
                    luma = (cj[:, 0] * dt(LUMA[0]) + cj[:, 1] * dt(LUMA[1])) + cj[:, 2] * dt(LUMA[2])
                    q = _glm_max(dt(F(0.05)), dt(1) - luma)
                    ur = u[np.arange(len(j)), draws]
                    risky[j] |= np.abs(ur - q) < MARGIN
                    kill = ur < q
                    cj = np.where(kill[:, None], dt(0), cj / (dt(1) - q)[:, None])
                    alive = ~kill
                    code |= np.where(kill, RR_KILL, RR_LIVE)
                c[j], o[j], d[j] = cj, new_o, new_d
                route[ii, b, j] = code
                ix = j[alive]
            assert ix.size == 0
            image = image + c
    assert image.dtype == dt
    rows = len(ys)
    return {"image": image.reshape(rows, W, 3), "keep": ~risky.reshape(rows, W),
            "route": route.reshape(len(iters), depth, rows, W), "geom": hit_geom.reshape(len(iters), depth, rows, W),
            "hit_risky": hit_risky.reshape(len(iters), depth, rows, W)}


def deviation(a, b):
    """max_c |a_c - b_c| / max(max_c b_c, 1e-3) per pixel; b is the yardstick.  NaN counts as infinite."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    dev = np.abs(a - b).max(-1) / np.maximum(b.max(-1), 1e-3)
    return np.where(np.isfinite(dev), dev, np.inf)


def describe(ref, yx):
    """The replay's route of pixel (row, column): one line per iteration."""
    r, col = yx
    out = []
    for ii in range(ref["route"].shape[0]):
        steps = [f"{route_text(int(ref['route'][ii, b, r, col]))}@g{int(ref['geom'][ii, b, r, col])}"
                 for b in range(ref["route"].shape[1]) if ref["route"][ii, b, r, col]]
        out.append(" > ".join(steps))
    return " | ".join(out)


# ---- scenes ----------------------------------------------------------------------------------------------
BOX_CENTRE, BOX_SIZE, WALL = (0.0, 5.0, 0.0), 12.0, 0.2
# (TYPE, TRANS, ROTAT, SCALE, material); the materials pairwise differ by at least 0.02 in some channel
OBJECTS = [
    ("cube", (-2.6, 3.0, -1.0), (20.0, 35.0, 10.0), (2.0, 1.4, 1.8), {"RGB": [0.85, 0.45, 0.30]}),
    ("sphere", (2.4, 3.2, -0.5), (0.0, 30.0, 40.0), (2.4, 1.5, 1.9), {"RGB": [0.35, 0.80, 0.45]}),
    ("sphere", (-0.3, 7.6, -2.0), (15.0, 0.0, 25.0), (2.6, 1.6, 2.0),
     {"RGB": [0.90, 0.85, 0.60], "SPECRGB": [0.70, 0.95, 0.90], "REFLECTIVE": 1.0}),
    ("cube", (2.8, 6.8, -1.5), (-15.0, 50.0, 25.0), (1.6, 2.2, 1.5),
     {"RGB": [0.55, 0.60, 0.95], "SPECRGB": [0.95, 0.75, 0.65], "REFLECTIVE": 0.5}),
    ("cube", (-1.0, 4.6, 1.2), (10.0, 20.0, 30.0), (1.3, 1.3, 1.3),
     {"RGB": [0.95, 0.90, 0.80], "SPECRGB": [0.80, 0.90, 0.97], "REFRACTIVE": 1.0, "IOR": 1.5}),
    ("sphere", (0.9, 5.4, 1.0), (0.0, 0.0, 0.0), (1.5, 1.2, 1.4),
     {"RGB": [0.80, 0.97, 0.88], "SPECRGB": [0.97, 0.82, 0.90], "REFRACTIVE": 1.0, "IOR": 0.75}),
    ("cube", (-3.4, 7.5, 0.5), (40.0, 10.0, -20.0), (1.2, 1.2, 2.0), {"RGB": [0.65, 0.35, 0.75]}),
]
DIFFUSE_CUBE, DIFFUSE_SPHERE, MIRROR_OBJ, HALF_OBJ, GLASS_15, GLASS_075, EXTRA_CUBE = range(7)
CAMERA = {"RES": [48, 36], "FOVY": 30.0, "ITERATIONS": 1, "DEPTH": 8, "FILE": "lantern",
          "EYE": [0.7, 4.3, 4.6], "LOOKAT": [-0.4, 5.6, -0.5], "UP": [0.0, 1.0, 0.0]}
# a narrow view along the y axis of the half-mirror cube, 2.5 units from its face: the face fills the frame
FACE_CAMERA = dict(CAMERA, FOVY=8.0, EYE=[1.82, 10.25, -1.22], LOOKAT=[2.8, 6.8, -1.5])
TEXTURE = (6, 8)    # (h, w) of lantern_mesh's generated texture


def tile_colour(i):
    return [0.35 + 0.6 * ((7 * i) % 11) / 11, 0.35 + 0.6 * ((5 * i) % 13) / 13, 0.35 + 0.6 * ((3 * i) % 17) / 17]


def texture_pixels():
    """Distinct texels, none dark."""
    h, w = TEXTURE
    i = np.arange(h * w).reshape(h, w)
    return np.stack([90 + (37 * i) % 160, 80 + (53 * i) % 170, 100 + (71 * i) % 150], -1).astype(np.uint8)


def lantern(tmp, k=2, extra_materials=0, mesh=False, depth=8, face=False):
    """The lantern: a 12-unit box of k x k thin emissive cube tiles per wall, every tile its own colour and
    an emittance in {1, 2, 3}, around OBJECTS — a rotated diffuse cube, a stretched diffuse sphere, a
    stretched mirror sphere whose specular colour is not its colour, a half-mirror cube, a glass cube of
    ior 1.5, a glass sphere of ior 0.75 and one more cube — seen from inside, off every symmetry plane.  A
    path's colour is then the product of everything it met.  6 k^2 + 7 geoms: 31 at k = 2, 103 at k = 4.
    extra_materials: unused materials after the used ones.  mesh=True replaces the diffuse sphere by
    mesh_ref's UV sphere (smooth normals; rotated and non-uniformly scaled but NOT mirrored: a ray that leaves
    a reversed-winding mesh starts 2e-4 in front of its own front-facing triangle, which mesh_ref's
    |t| < edge_eps rule excludes, so no such path would be kept) and the last cube by a torus that carries a
    generated texture.  face=True looks at one face of the half-mirror cube from so close that every camera
    ray meets it first (FACE_CAMERA).  Written as a JSON scene under tmp (materials get their ids in the
    order of their names), with DEPTH = depth.  Returns (path, textures): the texel arrays by texture id."""
    name = (f"lantern{k}_d{depth}" + (f"_x{extra_materials}" if extra_materials else "") + ("_mesh" if mesh else "")
            + ("_face" if face else ""))
    d = Path(tmp) / name
    (d / "Models").mkdir(parents=True)
    (d / "Textures").mkdir()
    mats, objs, textures = {}, [], []
    for i, (typ, t, r, s, m) in enumerate(OBJECTS):
        m = dict(m)
        o = {"TYPE": typ, "MATERIAL": f"o{i}", "TRANS": list(t), "ROTAT": list(r), "SCALE": list(s)}
        if mesh and i == DIFFUSE_SPHERE:
            M.uv_sphere_obj(d / "Models" / "uvsphere.obj", nu=16, nv=10)
            o.update(TYPE="mesh", OBJ_FILE="uvsphere.obj", SCALE=[1.4, 0.9, 1.1])
        if mesh and i == EXTRA_CUBE:
            from PIL import Image
            M.torus_obj(d / "Models" / "torus.obj", nu=12, nv=8)
            Image.fromarray(texture_pixels(), "RGB").save(d / "Textures" / "tiles.png")
            textures.append(texture_pixels())
            o.update(TYPE="mesh", OBJ_FILE="torus.obj", SCALE=[1.3, 1.5, 1.2])
            m["TEXTURE_FILE"] = "tiles.png"
        mats[f"o{i}"] = m
        objs.append(o)
    c, half, size = BOX_CENTRE, BOX_SIZE / 2, BOX_SIZE / k
    tile = 0
    for axis in range(3):
        for side in (-1, 1):
            u, v = [a for a in range(3) if a != axis]
            for iu in range(k):
                for iv in range(k):
                    t, s = [0.0] * 3, [size] * 3
                    t[axis], s[axis] = c[axis] + side * (half + WALL / 2), WALL
                    t[u], t[v] = c[u] - half + (iu + 0.5) * size, c[v] - half + (iv + 0.5) * size
                    mats[f"t{tile:03d}"] = {"RGB": tile_colour(tile), "EMITTANCE": float(tile % 3 + 1)}
                    objs.append({"TYPE": "cube", "MATERIAL": f"t{tile:03d}", "TRANS": t, "ROTAT": [0.0, 0.0, 0.0],
                                 "SCALE": s})
                    tile += 1
    for i in range(extra_materials):
        mats[f"x{i:03d}"] = {"RGB": [0.5, 0.25 + 0.001 * i, 0.75]}
    spec = {"Extensions": {"REFRACTION": True}, "Materials": mats, "Objects": objs,
            "Camera": dict(FACE_CAMERA if face else CAMERA, DEPTH=depth)}
    path = d / "lantern.json"
    path.write_text(json.dumps(spec))
    return str(path), textures
