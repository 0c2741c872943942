"""A brute-force first-hit reference for scenes with meshes (a helper, not collected by pytest).

mesh_first_hit_ref restates, in a chosen dtype, what the reference computes for the deterministic
camera ray of every pixel (computeIntersections, pathtrace.cu:230-298): cubes and spheres by
denoise_ref.geom_hit, triangles by glm::intersectRayTriangle as written (glm/gtx/intersect.inl:37-74)
against EVERY world triangle — no BVH.  float64 is the yardstick; float32 measures the format's own
error.  The triangles come from Scene.triangles() (the reordered array, each with its load-order id).

The two mesh paths of the reference differ, and both are evaluated literally:
  mode="bvh"     BVHIntersectionTest + Triangle::intersect (intersections.cu:169-224, sceneStructs.h:145-160):
                 the closest triangle of the whole scene with t >= 0; it belongs to the geom whose
                 [tri_start, tri_end) holds its id; n = n0*bx + n1*by + n2*(1-bx-by),
                 uv = uv0*(1-bx-by) + uv1*bx + uv2*by.
  mode="linear"  meshIntersectionTest (intersections.cu:119-167): each mesh geom loops over the array
                 POSITIONS [tri_start, tri_end) — of the array the BVH build has reordered, so with more
                 than one mesh a geom tests (and lends its material to) triangles loaded for another —
                 keeps bz > 0, and n = w*n0 + n1 + n2, uv = w*uv0 + uv1 + uv2 with w = 1-bx-by.
                 use_bbox=True adds its cull by the geom's own world box (intersections.cu:126-139),
                 which then hides the foreign triangles in its range from rays that miss that box.
  mode="textbook"  bvh's hit with n = w*n0 + bx*n1 + by*n2: what neither path computes (for the tests
                 that show the three apart).

keep is decided in the evaluation's own dtype (use the float64 one) and is False where rounding may
choose another surface: see mesh_first_hit_ref.
"""
import json
from pathlib import Path

import numpy as np

import denoise_ref as R

SCENES = Path(__file__).resolve().parent / "scenes"

FLT_EPSILON = 1.1920928955078125e-07
TRI_DTYPE = np.dtype([("id", "<i4"), ("v", "<f4", (3, 3)), ("uv", "<f4", (3, 2)), ("n", "<f4", (3, 3)),
                      ("bmin", "<f4", (3,)), ("bmax", "<f4", (3,))])
assert TRI_DTYPE.itemsize == 124


def triangle_table(scene):
    """Scene.triangles() as one structured array (fields id, v, uv, n)."""
    tris = scene.triangles()
    return np.frombuffer(b"".join(bytes(t) for t in tris), TRI_DTYPE) if tris else np.zeros(0, TRI_DTYPE)


def _cross(a, b):
    """glm::cross, componentwise on (..., 3) given as tuples of arrays."""
    return (a[1] * b[2] - b[1] * a[2], a[2] * b[0] - b[2] * a[0], a[0] * b[1] - b[0] * a[1])


def _dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _comps(x):
    return tuple(x[..., k] for k in range(3))


def _glm_min(a, b):
    return np.where(b < a, b, a)


def _glm_max(a, b):
    return np.where(a < b, b, a)


def _box_cull(g, o, d, dt):
    """meshIntersectionTest's world-box test: (culled, near its threshold)."""
    inv = dt(1) / d
    lo = (np.asarray(list(g.min_bound), dt) - o) * inv
    hi = (np.asarray(list(g.max_bound), dt) - o) * inv
    mn = _glm_max(_glm_max(_glm_min(lo[..., 0], hi[..., 0]), _glm_min(lo[..., 1], hi[..., 1])),
                  _glm_min(lo[..., 2], hi[..., 2]))
    mx = _glm_min(_glm_min(_glm_max(lo[..., 0], hi[..., 0]), _glm_max(lo[..., 1], hi[..., 1])),
                  _glm_max(lo[..., 2], hi[..., 2]))
    return (mx < 0) | (mn > mx), mx, mn


def mesh_first_hit_ref(tris, geoms, cam, dt=np.float64, mode="bvh", edge_eps=1e-3, use_bbox=False, chunk=256):
    """Closest hit of every pixel's camera ray over cubes, spheres and all triangles, every step in dt.

    Returns dict(mat (-1 miss), geom (-1), tri (the triangle's id; -1 for a miss, cube or sphere),
    t (-1), P, n, uv (0 unless a triangle is hit), keep, back).  back counts the triangles of the hit
    geom's id range that the ray crosses from behind (a < 0) before the hit: the near side of a closed
    mesh whose winding is reversed.

    keep is False where
      * a triangle not behind the closest hit (t <= best + edge_eps) faces the ray and is met with a
        barycentric weight within edge_eps of 0, inside or outside (min(bx, by, 1-bx-by) in [-eps, eps));
      * such a triangle is met at grazing incidence, |a| < 1e-3 |e1 x e2| (there the weights themselves are
        ill-conditioned, so "met" is: the ray passes the triangle's bounding sphere);
      * such a triangle has a within a factor 4 of FLT_EPSILON, the culling threshold;
      * a triangle is met with |t| < edge_eps;
      * two candidate distances (triangles, cubes, spheres) lie within edge_eps of each other;
      * denoise_ref.geom_hit's rules for cubes and spheres apply;
      * use_bbox: a mesh geom's box test is within edge_eps of its threshold (Max of 0, min of Max).
    """
    H, W = cam.res[1], cam.res[0]
    with np.errstate(all="ignore"):
        d_all = R.camera_rays(cam, dt).reshape(-1, 3)
    res = mesh_hit_ref(tris, geoms, np.asarray(list(cam.position), dt), d_all, dt, mode, edge_eps, use_bbox, chunk)
    return {k: val.reshape((H, W) + val.shape[1:]) for k, val in res.items()}


def mesh_hit_ref(tris, geoms, o, d_all, dt=np.float64, mode="bvh", edge_eps=1e-3, use_bbox=False, chunk=256):
    """mesh_first_hit_ref's closest hit for the rays (o, d_all[i]): d_all is (n, 3); o is one origin (3,)
    shared by all rays or one per ray (n, 3).  Every elementwise operation is the same in both forms (a
    shared origin broadcasts), so a shared origin gives the same numbers as one repeated per ray.
    Returns mesh_first_hit_ref's dict with flat (n, ...) arrays."""
    assert mode in ("bvh", "linear", "textbook")
    assert not (use_bbox and mode != "linear")
    eps = dt(FLT_EPSILON)
    with np.errstate(all="ignore"):
        d_all = np.asarray(d_all, dt).reshape(-1, 3)
        o_all = np.asarray(o, dt).reshape(-1, 3)
        per_ray = o_all.shape[0] != 1
        assert not per_ray or o_all.shape == d_all.shape
        nr = d_all.shape[0]
        v = tris["v"].astype(dt)
        vn = tris["n"].astype(dt)
        vt = tris["uv"].astype(dt)
        tid = tris["id"].astype(np.int64)
        nt = len(tid)
        v0, e1, e2 = v[:, 0], v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
        e1c = tuple(e1[:, k][None, :] for k in range(3))
        e2c = tuple(e2[:, k][None, :] for k in range(3))
        area2 = np.sqrt(_dot3(_cross(_comps(e1), _comps(e2)), _cross(_comps(e1), _comps(e2))))
        cen = (v[:, 0] + v[:, 1] + v[:, 2]) / dt(3)
        rad = np.sqrt(((v - cen[:, None, :]) ** 2).sum(-1)).max(-1)
        mesh_geoms = [(gi, g) for gi, g in enumerate(geoms) if g.type == 2]
        geom_of_id = geom_of_triangle(tid, geoms)                    # by the id range (bvh)
        geom_of_pos = geom_of_triangle(np.arange(nt), geoms)         # by the array position (linear)
        mat_of_geom = np.array([g.material_id for g in geoms] + [-1], np.int32)

        out = {k: [] for k in ("mat", "geom", "tri", "t", "P", "n", "uv", "keep", "back")}
        for c0 in range(0, nr, chunk):
            d = d_all[c0:c0 + chunk]                          # (r, 3)
            r = d.shape[0]
            o = o_all[c0:c0 + chunk] if per_ray else o_all    # (r, 3) or (1, 3)
            ob = np.broadcast_to(o, d.shape)
            risky = np.zeros(r, bool)
            best_t = np.full(r, np.inf, dt)
            second_t = np.full(r, np.inf, dt)
            best_n = np.zeros((r, 3), dt)
            best_uv = np.zeros((r, 2), dt)
            best_geom = np.full(r, -1, np.int64)
            best_tri = np.full(r, -1, np.int64)

            if nt:
                dc = tuple(d[:, k][:, None] for k in range(3))                 # (r, 1)
                sc = tuple(o[:, k][:, None] - v0[:, k][None, :] for k in range(3))   # o - v0: (r, T) or (1, T)
                q = _cross(sc, e1c)                                            # glm::cross(s, e1)
                e2q = _dot3(e2c, q)
                p = _cross(dc, e2c)                                            # (r, T) x 3
                a = _dot3(e1c, p)
                f = dt(1) / a
                bx = f * _dot3(sc, p)
                by = f * _dot3(dc, q)
                bz = f * e2q
                hit = ~(a < eps) & ~(bx < 0) & ~(bx > 1) & ~(by < 0) & ~(by + bx > 1) & (bz >= 0)
                if mode == "linear":
                    hit &= bz > 0
                allowed = np.ones((r, nt), bool)
                if use_bbox:
                    for gi, g in mesh_geoms:
                        culled, mx, mn = _box_cull(g, o, d, dt)
                        risky |= (np.abs(mx) < edge_eps) | (np.abs(mx - mn) < edge_eps)
                        allowed &= ~(culled[:, None] & (geom_of_pos == gi)[None, :])
                if mode == "linear":
                    allowed &= (geom_of_pos >= 0)[None, :]   # (a position outside every range is never tested)
                th = np.where(hit & allowed, bz, np.inf)     # (r, T)
                # what rounding could turn into another answer, with the distance it would have
                w = (dt(1) - bx) - by
                m = np.minimum(np.minimum(bx, by), w)
                front = a >= eps / 4
                graze = np.abs(a) < dt(1e-3) * area2[None, :]
                co = cen[None, :, :] - o[:, None, :]                                      # (r, T, 3) or (1, T, 3)
                t_sph = _dot3(_comps(co), dc)                                             # closest approach
                d2 = (co ** 2).sum(-1) - t_sph * t_sph
                near_sph = (d2 <= (rad[None, :] + edge_eps) ** 2) & (t_sph + rad[None, :] >= 0)
                met = front & ~graze & (m >= -edge_eps) & (bz >= -edge_eps)
                bad = met & ((m < edge_eps) | (a < 4 * eps) | (np.abs(bz) < edge_eps))
                risk_t = np.where(bad & allowed, bz, np.inf)
                risk_t = np.minimum(risk_t, np.where(graze & near_sph & allowed, t_sph - rad[None, :], np.inf))
                risk_tmin = risk_t.min(axis=1)
                two = np.partition(th, 1, axis=1)[:, :2] if nt > 1 else np.concatenate([th, np.full((r, 1), np.inf)], 1)
            else:
                risk_tmin = np.full(r, np.inf, dt)
                two = np.full((r, 2), np.inf, dt)

            for gi, g in enumerate(geoms):
                edge = np.zeros(r, bool)
                if g.type == 2:
                    if not nt:
                        continue
                    if mode == "linear":
                        tg = np.where((geom_of_pos == gi)[None, :], th, np.inf)
                        k = tg.argmin(axis=1)                # (the first of equal distances, as `<` keeps it)
                        tw = tg[np.arange(r), k]
                    else:
                        k = th.argmin(axis=1)
                        tw = np.where(geom_of_id[k] == gi, th[np.arange(r), k], np.inf)
                    rr = np.arange(r)
                    x, y = bx[rr, k][:, None], by[rr, k][:, None]
                    wz = (dt(1) - x) - y
                    if mode == "linear":
                        nrm = (wz * vn[k, 0] + vn[k, 1]) + vn[k, 2]
                        g_uv = (wz * vt[k, 0] + vt[k, 1]) + vt[k, 2]
                    else:
                        if mode == "bvh":
                            nrm = (vn[k, 0] * x + vn[k, 1] * y) + vn[k, 2] * wz
                        else:
                            nrm = (vn[k, 0] * wz + vn[k, 1] * x) + vn[k, 2] * y
                        g_uv = (vt[k, 0] * wz + vt[k, 1] * x) + vt[k, 2] * y
                    nrm = R._normalize(nrm, dt)
                    g_tri = tid[k]
                else:
                    tw, nrm, always, edge = R.geom_hit(g, ob, d, dt, edge_eps)
                    risky |= always
                    g_uv, g_tri = np.zeros((r, 2), dt), np.full(r, -1, np.int64)
                closer = (tw > 0) & (tw < best_t)
                second_t = np.where(closer, best_t, np.minimum(second_t, tw))
                best_t = np.where(closer, tw, best_t)
                best_n = np.where(closer[:, None], nrm, best_n)
                best_uv = np.where(closer[:, None], g_uv, best_uv)
                best_geom = np.where(closer, gi, best_geom)
                best_tri = np.where(closer, g_tri, best_tri)
                risky = np.where(closer, risky | edge, risky)
            # the runner-up among the triangles (their closest entered above, once per geom in linear mode)
            mesh_best = best_tri >= 0
            second_t = np.minimum(second_t, np.where(mesh_best, two[:, 1], two[:, 0]))
            got = best_geom >= 0
            risky |= got & (second_t - best_t < edge_eps)
            risky |= np.isfinite(risk_tmin) & (risk_tmin <= best_t + edge_eps)
            back = np.zeros(r, np.int64)
            if nt:
                inside = (bx >= 0) & (by >= 0) & (bx + by <= 1) & (a < 0) & (bz > 0) & (bz < best_t[:, None])
                same = mesh_best[:, None] & (geom_of_id[None, :] == geom_of_triangle(best_tri, geoms)[:, None])
                back = (inside & same).sum(axis=1)
            t = np.where(got, best_t, dt(-1))
            P = np.where(got[:, None], ob + (t - dt(0.0001))[:, None] * R._normalize(d, dt), dt(0))
            out["mat"].append(mat_of_geom[best_geom])
            out["geom"].append(best_geom.astype(np.int32))
            out["tri"].append(best_tri.astype(np.int32))
            out["t"].append(t)
            out["P"].append(P)
            out["n"].append(np.where(got[:, None], best_n, dt(0)))
            out["uv"].append(np.where(mesh_best[:, None], best_uv, dt(0)))
            out["keep"].append(~risky)
            out["back"].append(back)
    return {k: np.concatenate(val) for k, val in out.items()}


def geom_of_triangle(tri_id, geoms):
    """The first geom in index order whose [tri_start, tri_end) holds the triangle id (-1: none)."""
    out = np.full(tri_id.shape, -1, np.int64)
    for gi, g in enumerate(geoms):
        if g.type == 2:
            out[(out < 0) & (tri_id >= g.tri_start) & (tri_id < g.tri_end)] = gi
    return out


def errors(ref64, t, P, n, uv):
    """Largest deviation of (t, P, n, uv) from the float64 reference over its kept pixels that hit, by
    the kind of surface: {"tri": (e_t, e_p, e_n, e_uv), "prim": (e_t, e_p, e_n, 0)} — triangles, and cubes
    and spheres.  e_t and e_p are relative to max(1, t), e_n and e_uv per component; a kind that no kept
    pixel shows gives zeros.  (uv is compared on triangles only: a cube or sphere leaves the texture
    coordinates an earlier mesh test wrote, or nothing, computeIntersections' tmp_coord.)"""
    out = {}
    for kind, sel in (("tri", ref64["tri"] >= 0), ("prim", (ref64["tri"] < 0) & (ref64["mat"] >= 0))):
        k = ref64["keep"] & sel
        if not k.any():
            out[kind] = (0.0, 0.0, 0.0, 0.0)
            continue
        scale = np.maximum(1.0, ref64["t"][k])
        e_t = (np.abs(t[k].astype(np.float64) - ref64["t"][k]) / scale).max()
        e_p = (np.abs(P[k].astype(np.float64) - ref64["P"][k]) / scale[:, None]).max()
        e_n = np.abs(n[k].astype(np.float64) - ref64["n"][k]).max()
        e_uv = np.abs(uv[k].astype(np.float64) - ref64["uv"][k]).max() if kind == "tri" else 0.0
        out[kind] = (float(e_t), float(e_p), float(e_n), float(e_uv))
    return out


def deviations(ref64, ref32):
    """errors() of the float32 evaluation: float32's own error D_t, D_p, D_n, D_uv per kind.  Asserts that
    both evaluations chose the same surface — geom and triangle — on every kept pixel."""
    keep = ref64["keep"]
    for key in ("mat", "geom", "tri"):
        assert np.array_equal(ref64[key][keep], ref32[key][keep]), key
    return errors(ref64, ref32["t"], ref32["P"], ref32["n"], ref32["uv"])


# ---- scenes the tests build ----------------------------------------------------------------------------
def _write_obj(path, pos, nrm, uv, faces):
    """faces: (F, 3, 3) indices (v, vt, vn) per corner, 0-based.  Returns the face corners as written:
    (positions (F, 3, 3), normals (F, 3, 3), texture coordinates (F, 3, 2)), rounded to the file's 7 decimals."""
    lines = [f"v {x:.7f} {y:.7f} {z:.7f}" for x, y, z in pos]
    lines += [f"vt {u:.7f} {w:.7f}" for u, w in uv]
    lines += [f"vn {x:.7f} {y:.7f} {z:.7f}" for x, y, z in nrm]
    lines += ["f " + " ".join(f"{a + 1}/{b + 1}/{c + 1}" for a, b, c in f) for f in faces]
    path.write_text("\n".join(lines) + "\n")
    pos, nrm, uv = (np.round(np.asarray(x, np.float64), 7) for x in (pos, nrm, uv))
    return pos[faces[..., 0]], nrm[faces[..., 2]], uv[faces[..., 1]]


def _outward(pos, nrm, faces):
    """Wind every face counter-clockwise about its vertex normals and drop the degenerate ones."""
    out = []
    for f in faces:
        p = pos[[c[0] for c in f]]
        g = np.cross(p[1] - p[0], p[2] - p[0])
        if np.linalg.norm(g) < 1e-9:
            continue
        if g @ nrm[[c[2] for c in f]].sum(0) < 0:
            f = [f[0], f[2], f[1]]
        out.append(f)
    return np.array(out)


def uv_sphere_obj(path, nu=24, nv=16):
    """A unit sphere of nu x nv quads split into triangles, one shared vn per vertex (the pole rows
    collapse to triangles), vt on an (nu+1) x (nv+1) grid.  Returns _write_obj's corners."""
    th = np.pi * np.arange(nv + 1) / nv
    ph = 2 * np.pi * np.arange(nu) / nu
    pos = np.array([[np.sin(t) * np.cos(p), np.cos(t), np.sin(t) * np.sin(p)] for t in th for p in ph])
    uv = np.array([[i / nu, 1 - j / nv] for j in range(nv + 1) for i in range(nu + 1)])
    faces = []
    for j in range(nv):
        for i in range(nu):
            c = [(j * nu + i, j * (nu + 1) + i), (j * nu + (i + 1) % nu, j * (nu + 1) + i + 1),
                 ((j + 1) * nu + (i + 1) % nu, (j + 1) * (nu + 1) + i + 1), ((j + 1) * nu + i, (j + 1) * (nu + 1) + i)]
            for tri in ((0, 1, 2), (0, 2, 3)):
                faces.append([(c[k][0], c[k][1], c[k][0]) for k in tri])
    return _write_obj(path, pos, pos, uv, _outward(pos, pos, faces))


def torus_obj(path, nu=24, nv=12, major=1.0, minor=0.4):
    """A torus about the y axis, nu x nv quads split into triangles, shared vn and vt like uv_sphere_obj."""
    u = 2 * np.pi * np.arange(nu) / nu
    w = 2 * np.pi * np.arange(nv) / nv
    pos = np.array([[(major + minor * np.cos(b)) * np.cos(a), minor * np.sin(b), (major + minor * np.cos(b)) * np.sin(a)]
                    for b in w for a in u])
    nrm = np.array([[np.cos(b) * np.cos(a), np.sin(b), np.cos(b) * np.sin(a)] for b in w for a in u])
    uv = np.array([[i / nu, j / nv] for j in range(nv + 1) for i in range(nu + 1)])
    faces = []
    for j in range(nv):
        for i in range(nu):
            c = [(j * nu + i, j * (nu + 1) + i), (j * nu + (i + 1) % nu, j * (nu + 1) + i + 1),
                 (((j + 1) % nv) * nu + (i + 1) % nu, (j + 1) * (nu + 1) + i + 1),
                 (((j + 1) % nv) * nu + i, (j + 1) * (nu + 1) + i)]
            for tri in ((0, 1, 2), (0, 2, 3)):
                faces.append([(c[k][0], c[k][1], c[k][0]) for k in tri])
    return _write_obj(path, pos, nrm, uv, _outward(pos, nrm, faces))


# (type, OBJ, TRANS, ROTAT, SCALE); geom 2 is mirrored in x: its winding is reversed
SMOOTH_OBJECTS = [
    ("mesh", "uvsphere.obj", (-2.1, 6.3, 0.0), (20.0, 35.0, 10.0), (2.5, 1.2, 1.8)),
    ("mesh", "torus.obj", (2.1, 6.3, 0.0), (60.0, 20.0, 15.0), (1.5, 1.1, 1.3)),
    ("mesh", "uvsphere.obj", (-2.0, 3.6, 0.3), (-15.0, 50.0, 25.0), (-1.7, 1.1, 1.3)),
    ("mesh", "torus.obj", (2.2, 3.6, 0.0), (100.0, 0.0, 30.0), (1.3, 1.7, 1.1)),
    ("cube", None, (0.1, 5.0, 2.0), (10.0, 20.0, 30.0), (1.3, 0.8, 0.8)),
    ("sphere", None, (-0.6, 3.5, 2.5), (0.0, 30.0, 40.0), (1.2, 0.8, 1.0)),
]
SMOOTH_REVERSED = 2


def smooth_colour(i):
    """Geom i's emissive colour in the `emissive` variant: binary fractions, distinct per geom."""
    return ((i + 1) / 16.0, ((3 * i) % 7 + 1) / 8.0, 0.5)


def smooth_scene(tmp, emissive=False, sky=False, res=(48, 36), depth=4):
    """Two UV spheres and two tori with shared per-vertex normals and texture coordinates under rotated,
    non-uniform scales (one mirrored), partly hidden by a cube and a sphere; every geom its own material.
    emissive=False: diffuse meshes and sphere, the cube is the light.  emissive=True: every material
    emits its smooth_colour, so that a depth-1 render shows the geom of every pixel.  sky=True encloses
    the scene and the camera in a large emissive sphere, so that a path that leaves the meshes still
    carries what it met into the image.  Returns the path."""
    d = tmp / ("smooth_e" if emissive else "smooth_sky" if sky else "smooth")
    (d / "Models").mkdir(parents=True)
    uv_sphere_obj(d / "Models" / "uvsphere.obj")
    torus_obj(d / "Models" / "torus.obj")
    mats, objs = {}, []
    for i, (typ, obj, t, r, s) in enumerate(SMOOTH_OBJECTS):
        name = f"m{i:02d}"
        if emissive:
            mats[name] = {"RGB": list(smooth_colour(i)), "EMITTANCE": 1.0}
        elif typ == "cube":
            mats[name] = {"RGB": [1.0, 1.0, 1.0], "EMITTANCE": 6.0}
        else:
            mats[name] = {"RGB": [0.35 + 0.1 * i, 0.8 - 0.09 * i, 0.5 + 0.05 * (i % 3)]}
        o = {"TYPE": typ, "MATERIAL": name, "TRANS": list(t), "ROTAT": list(r), "SCALE": list(s)}
        if obj:
            o["OBJ_FILE"] = obj
        objs.append(o)
    if sky:
        mats["sky"] = {"RGB": [0.9, 0.95, 1.0], "EMITTANCE": 1.0}
        objs.append({"TYPE": "sphere", "MATERIAL": "sky", "TRANS": [0.0, 5.0, 0.0], "ROTAT": [0.0, 0.0, 0.0],
                     "SCALE": [60.0, 60.0, 60.0]})
    spec = {"Materials": mats, "Objects": objs,
            "Camera": {"RES": list(res), "FOVY": 16.0, "ITERATIONS": 2, "DEPTH": 1 if emissive else depth,
                       "FILE": "smooth", "EYE": [0.0, 5.0, 10.5], "LOOKAT": [0.1, 5.0, 0.0], "UP": [0.0, 1.0, 0.0]}}
    path = d / "smooth.json"
    path.write_text(json.dumps(spec))
    return str(path)


# (the loaded camera is put on runCuda's orbit, main.cpp:59-73 and 117-136, which mirrors the eye's height
# about the look-at point: these eyes lie below it so that the views look down, at about (1.5, 3, 4)
# and (2, 6, 6))
ROOM_VIEWS = {"room_chair": dict(EYE=[1.5, -0.6, 4.0], LOOKAT=[0.0, 1.2, -1.0], FOVY=16.0),
              "room_wall": dict(EYE=[2.0, 4.0, 6.0], LOOKAT=[0.0, 5.0, -4.8], FOVY=14.0)}


def room_view(tmp, name, res=(48, 36)):
    """tests/scenes/room.json with a closer camera (ROOM_VIEWS).  Returns the path."""
    spec = json.loads((SCENES / "room.json").read_text())
    spec["Camera"].update(ROOM_VIEWS[name], RES=list(res))
    d = tmp / name
    d.mkdir()
    (d / "Textures").symlink_to(SCENES / "Textures")
    (d / "Models").symlink_to(SCENES / "Models")
    path = d / "room.json"
    path.write_text(json.dumps(spec))
    return str(path)


MESH_SCENES = ("smooth", "room_chair", "room_wall")


def mesh_scene(tmp, name):
    return smooth_scene(tmp) if name == "smooth" else room_view(tmp, name)
