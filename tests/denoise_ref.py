"""References for the G-buffer and denoiser tests (a helper, not collected by pytest).

atrous_ref: the filter of DESIGN.md §10 restated in numpy with every intermediate in np.float32 (numpy's
float32 +, -, *, / are single correctly rounded IEEE operations, as the kernels' are), so the GPU result
must equal it bit for bit.

first_hit_ref: the reference's sphere and cube intersection tests (intersections.cu:4-115, with
getPointOnRay's 1e-4 back-off and the world-distance t) over a scene's float32 matrices, evaluated in
a chosen dtype: float64 is the yardstick, float32 measures the format's own error.
"""
import numpy as np

F = np.float32
H5 = (F(1 / 16), F(1 / 4), F(3 / 8), F(1 / 4), F(1 / 16))
ALB_MIN = F(2.0 ** -10)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _modulate(c, alb3, divide):
    m = alb3 >= ALB_MIN
    safe = np.where(m, alb3, F(1))
    return np.where(m, c / safe if divide else c * safe, c).astype(F)


def _shift(a, oy, ox):
    """a[y + oy, x + ox] with the validity mask of the source position."""
    Hh, Ww = a.shape[:2]
    ys, xs = np.arange(Hh) + oy, np.arange(Ww) + ox
    vy, vx = (ys >= 0) & (ys < Hh), (xs >= 0) & (xs < Ww)
    return a[np.clip(ys, 0, Hh - 1)][:, np.clip(xs, 0, Ww - 1)], vy[:, None] & vx[None, :]


def atrous_ref(rgb, samples, gA, gB, alb, levels, sigma_c, sigma_n, sigma_p, demodulate=True):
    """rgb (H, W, 3), gA / gB / alb (H, W, 4), all float32 -> (H, W, 3) float32."""
    rgb, gA, gB, alb = (np.ascontiguousarray(v, F) for v in (rgb, gA, gB, alb))
    with np.errstate(all="ignore"):
        inv_c = F(1) / (F(sigma_c) * F(sigma_c))
        inv_n = F(1) / (F(sigma_n) * F(sigma_n))
        inv_p = F(1) / (F(sigma_p) * F(sigma_p))
        c = (rgb / F(samples)).astype(F)
        if demodulate:
            c = _modulate(c, alb[..., :3], True)
        mat = gA[..., 3].copy().view(np.int32)
        Np, Pp = gA[..., :3], gB[..., :3]
        for i in range(levels):
            s = 1 << i
            inv_ci = inv_c * F(4 ** i)
            acc = np.zeros_like(c)
            wsum = np.zeros(c.shape[:2], F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    cq, inside = _shift(c, dy * s, dx * s)
                    Nq, _ = _shift(Np, dy * s, dx * s)
                    Pq, _ = _shift(Pp, dy * s, dx * s)
                    mq, _ = _shift(mat, dy * s, dx * s)
                    valid = inside & (mq >= 0)
                    k = H5[dx + 2] * H5[dy + 2]
                    d = cq - c
                    xc = _dot(d, d) * inv_ci
                    xn = np.maximum(F(0), F(1) - _dot(Np, Nq)) * inv_n
                    e = _dot(Np, Pq - Pp)
                    xp = (e * e) * inv_p
                    w = (k / (((F(1) + xc) * (F(1) + xn)) * (F(1) + xp))).astype(F)
                    acc = np.where(valid[..., None], acc + w[..., None] * cq, acc)
                    wsum = np.where(valid, wsum + w, wsum)
            hit = mat >= 0
            c = np.where(hit[..., None], acc / np.where(hit, wsum, F(1))[..., None], c).astype(F)
        if demodulate:
            c = _modulate(c, alb[..., :3], False)
    assert c.dtype == F
    return c


# ---- first hit of the deterministic camera ray ----------------------------------------------
def _mv(M, v, w, dt):
    """glm mat4 (column-major, a[4c + r]) times (v, w) -> xyz."""
    m = np.asarray(list(M), dt).reshape(4, 4)   # m[c][r]
    return (v[..., 0:1] * m[0, :3] + v[..., 1:2] * m[1, :3]) + (v[..., 2:3] * m[2, :3] + dt(w) * m[3, :3])


def _normalize(v, dt):
    return v * (dt(1) / np.sqrt(_dot(v, v)))[..., None]


def camera_rays(cam, dt):
    """generateRayFromCamera without jitter or lens (pathtrace.cu:183-227): (H, W, 3) directions."""
    W, Hh = cam.res[0], cam.res[1]
    x = np.arange(W, dtype=dt)[None, :] - dt(W) * dt(0.5)
    y = np.arange(Hh, dtype=dt)[:, None] - dt(Hh) * dt(0.5)
    view, up, right = (np.asarray(list(v), dt) for v in (cam.view, cam.up, cam.right))
    plx, ply = dt(cam.pixel_length[0]), dt(cam.pixel_length[1])
    d = (view - (right * plx) * x[..., None]) - (up * ply) * y[..., None]
    return _normalize(d.astype(dt), dt)


def geom_hit(g, ob, d, dt, edge_eps):
    """One sphere (type 0) or cube (type 1) against the rays (ob, d), every step in dtype dt:
    (world distance, inf on a miss; normal; risky whether hit or not; risky if this is the closest hit)."""
    shape = d.shape[:-1]
    always = np.zeros(shape, bool)
    qo = _mv(g.inverse_transform, ob, 1, dt)
    qd = _normalize(_mv(g.inverse_transform, d, 0, dt), dt)
    if g.type == 1:
        tmin = np.full(shape, -1e38, dt)
        tmax = np.full(shape, 1e38, dt)
        nmin = np.zeros(shape + (3,), dt)
        nmax = np.zeros(shape + (3,), dt)
        for a in range(3):
            t1 = (dt(-0.5) - qo[..., a]) / qd[..., a]
            t2 = (dt(0.5) - qo[..., a]) / qd[..., a]
            ta, tb = np.minimum(t1, t2), np.maximum(t1, t2)
            n = np.zeros(shape + (3,), dt)
            n[..., a] = np.where(t2 < t1, dt(1), dt(-1))
            up_ = (ta > 0) & (ta > tmin)
            tmin = np.where(up_, ta, tmin)
            nmin = np.where(up_[..., None], n, nmin)
            lo = tb < tmax
            tmax = np.where(lo, tb, tmax)
            nmax = np.where(lo[..., None], n, nmax)
        always |= np.abs(tmax - tmin) < 4 * edge_eps     # grazes an edge or corner, hit or miss
        hit = (tmax >= tmin) & (tmax > 0)
        inside = tmin <= 0
        tmin = np.where(inside, tmax, tmin)
        nmin = np.where(inside[..., None], nmax, nmin)
        obj = qo + (tmin - dt(0.0001))[..., None] * _normalize(qd, dt)
        near = (np.abs(np.abs(qo + tmin[..., None] * qd) - 0.5) < edge_eps).sum(axis=-1)
        edge = hit & (near >= 2)
        nrm = _normalize(_mv(g.inv_transpose, nmin, 0, dt), dt)
    else:
        vdd = _dot(qo, qd)
        rad = vdd * vdd - (_dot(qo, qo) - dt(0.25))
        always |= np.abs(rad) < edge_eps
        sq = np.sqrt(np.where(rad < 0, dt(0), rad))
        t1, t2 = -vdd + sq, -vdd - sq
        hit = (rad >= 0) & ~((t1 < 0) & (t2 < 0))
        outside = (t1 > 0) & (t2 > 0)
        t = np.where(outside, np.minimum(t1, t2), np.maximum(t1, t2))
        obj = qo + (t - dt(0.0001))[..., None] * _normalize(qd, dt)
        nrm = _normalize(_mv(g.inv_transpose, obj, 0, dt), dt)
        nrm = np.where(outside[..., None], nrm, -nrm)
        edge = np.zeros(shape, bool)
    ip = _mv(g.transform, obj, 1, dt)
    diff = ob - ip
    tw = np.sqrt(_dot(diff, diff))
    hit &= tw > 0
    return np.where(hit, tw, np.inf), nrm, always, edge


def first_hit_ref(geoms, cam, dt=np.float64, edge_eps=1e-3):
    """Closest hit over the scene's spheres (type 0) and cubes (type 1), every step in dtype dt.
    Returns dict(mat (-1 miss), n, t, P, keep): keep is False where the ray passes within edge_eps
    (object space) of a cube edge or of a sphere's silhouette (|discriminant| < edge_eps), or where two
    geoms' distances lie within edge_eps of each other — there the choice of surface depends on
    rounding."""
    with np.errstate(all="ignore"):
        d = camera_rays(cam, dt)
        o = np.asarray(list(cam.position), dt)
        shape = d.shape[:2]
        best_t = np.full(shape, np.inf, dt)
        second_t = np.full(shape, np.inf, dt)
        best_n = np.zeros(shape + (3,), dt)
        best_mat = np.full(shape, -1, np.int32)
        risky = np.zeros(shape, bool)
        ob = np.broadcast_to(o, d.shape)
        for g in geoms:
            tw, nrm, always, edge = geom_hit(g, ob, d, dt, edge_eps)
            risky |= always
            closer = tw < best_t
            second_t = np.where(closer, best_t, np.minimum(second_t, tw))
            best_t = np.where(closer, tw, best_t)
            best_n = np.where(closer[..., None], nrm, best_n)
            best_mat = np.where(closer, np.int32(g.material_id), best_mat)
            risky = np.where(closer, risky | edge, risky)   # (an edge of an occluded cube does not matter)
        got = best_mat >= 0
        risky |= got & (second_t - best_t < edge_eps)
        t = np.where(got, best_t, dt(-1))
        P = np.where(got[..., None], ob + (t - dt(0.0001))[..., None] * _normalize(d, dt), dt(0))
        n = np.where(got[..., None], best_n, dt(0))
    return {"mat": best_mat, "n": n, "t": t, "P": P, "keep": ~risky}


def three_body_scene(P, res=(40, 30)):
    """Two rotated, non-uniformly scaled cubes and a stretched sphere in front of the camera (materials
    1..3; 0 is unused so that an id of 0 cannot pass by accident)."""
    s = P.Scene()
    s.add_material(rgb=(0.1, 0.1, 0.1))
    m = [s.add_material(rgb=c) for c in ((0.8, 0.3, 0.2), (0.2, 0.7, 0.3), (0.3, 0.4, 0.9))]
    s.add_geom(P.CUBE, m[0], (-2.4, 4.2, 0.5), (20.0, 35.0, 10.0), (2.5, 1.2, 1.8))
    s.add_geom(P.CUBE, m[1], (2.6, 5.6, -1.0), (-15.0, 50.0, 25.0), (1.5, 3.0, 2.2))
    s.add_geom(P.SPHERE, m[2], (0.2, 5.3, 1.5), (0.0, 30.0, 40.0), (2.2, 1.4, 1.8))
    s.set_camera(res, 20.0, (0.0, 5.0, 10.5), (0.2, 5.0, 0.0), (0.0, 1.0, 0.0))
    s.set_render(1, 4, "three_body")
    s.finalize()
    return s


def inside_scene(P, shell, res=(40, 30)):
    """The camera inside a stretched, rotated sphere (shell = P.SPHERE) or a rotated cube (P.CUBE), with
    a cube and a sphere in front of it: every ray that passes them meets the shell from within
    (intersections.cu:46-51 and 99-112, outside = false).  Materials 1..3; there are no misses."""
    s = P.Scene()
    s.add_material(rgb=(0.1, 0.1, 0.1))
    m = [s.add_material(rgb=c) for c in ((0.8, 0.3, 0.2), (0.2, 0.7, 0.3), (0.3, 0.4, 0.9))]
    if shell == P.SPHERE:
        s.add_geom(P.SPHERE, m[0], (0.0, 5.0, 0.0), (0.0, 30.0, 40.0), (24.0, 14.0, 20.0))
    else:
        s.add_geom(P.CUBE, m[0], (0.0, 5.0, 0.0), (10.0, 25.0, 5.0), (20.0, 12.0, 24.0))
    s.add_geom(P.CUBE, m[1], (-1.6, 4.4, 0.5), (20.0, 35.0, 10.0), (1.5, 1.2, 1.8))
    s.add_geom(P.SPHERE, m[2], (1.5, 5.6, 1.0), (0.0, 30.0, 40.0), (1.6, 1.0, 1.3))
    s.set_camera(res, 20.0, (0.0, 5.0, 6.0), (0.2, 5.0, 0.0), (0.0, 1.0, 0.0))
    s.set_render(1, 4, "inside")
    s.finalize()
    return s


def deviations(ref64, ref32):
    """Largest deviation of the float32 evaluation from the float64 one over the kept pixels that hit:
    (D_n per normal component, D_t and D_p relative to max(1, t))."""
    k = ref64["keep"] & (ref64["mat"] >= 0)
    assert np.array_equal(ref64["mat"][k], ref32["mat"][k])
    scale = np.maximum(1.0, ref64["t"][k])
    d_n = np.abs(ref32["n"][k].astype(np.float64) - ref64["n"][k]).max()
    d_t = (np.abs(ref32["t"][k].astype(np.float64) - ref64["t"][k]) / scale).max()
    d_p = (np.abs(ref32["P"][k].astype(np.float64) - ref64["P"][k]) / scale[:, None]).max()
    return float(d_n), float(d_t), float(d_p)


def tex_color_ref(pixels, u, v):
    """Texture::get_color (sceneStructs.h:176-189) for an (h, w, 3) uint8 texture, float32 steps."""
    h, w = pixels.shape[:2]
    u, v = np.asarray(u, F), np.asarray(v, F)
    X = np.minimum(F(1) * F(w) * u, F(1) * F(w) - F(1)).astype(np.int32)
    Y = np.minimum(F(1) * F(h) * (F(1) - v), F(1) * F(h) - F(1)).astype(np.int32)
    X, Y = np.maximum(X, 0), np.maximum(Y, 0)
    return (F(0.003921568627) * pixels[Y, X].astype(F)).astype(F)
