"""Reference for the temporal reprojection tests (a helper, not collected by pytest): DESIGN.md §12
restated in numpy with every intermediate in np.float32, in the stated order, so the GPU results must
equal it bit for bit (numpy's float32 +, -, *, / and floor are single correctly rounded IEEE operations,
as the kernels' are).  The shared pieces (dot, modulation, shifts, lum) are tests/denoise_ref.py's and
tests/denoise_var_ref.py's.

Temporal is the state of a pt_temporal object: frame() is pt_temporal_frame (all three cases),
resolve() is pt_temporal_resolve (both variance branches), image() is pt_temporal_image (the chaining
into atrous_var_ref).  Cameras are anything with the fields of pt_camera (position, view, up, right,
pixel_length); make_camera builds one.
"""
from types import SimpleNamespace

import numpy as np

from denoise_ref import F, _dot, _modulate, _shift
from denoise_var_ref import atrous_var_ref, lum

EMPTY, SAME_VIEW, NEW_VIEW = 1, 2, 3
DEFAULTS = dict(max_history=32.0, min_ndot=0.9, plane_tol=0.02, demodulate=1, min_frames=4)


def make_camera(position, view, up, right, pixel_length, res=(0, 0), look_at=(0, 0, 0), fov=(0, 0)):
    """A pt_camera stand-in whose fields are float32 values."""
    f = lambda v: tuple(float(F(x)) for x in v)   # noqa: E731
    return SimpleNamespace(res=tuple(res), position=f(position), look_at=f(look_at), view=f(view), up=f(up),
                           right=f(right), fov=f(fov), pixel_length=f(pixel_length))


def _cam_key(cam):
    return tuple(np.asarray(list(getattr(cam, k)), F).tobytes() for k in
                 ("position", "look_at", "view", "up", "right", "fov", "pixel_length")) + (tuple(cam.res),)


def _v3(x):
    return np.asarray(list(x), F)


def _dot3(a, b):   # the host's dot of two 3-vectors
    return F(F(a[0] * b[0]) + F(a[1] * b[1])) + F(a[2] * b[2])


def reproject_coords(cam, gB, W, H):
    """(fx, fy, z) of every pixel's position in the view of `cam` (float32, the kernel's order)."""
    with np.errstate(all="ignore"):
        pos, view, right, up = _v3(cam.position), _v3(cam.view), _v3(cam.right), _v3(cam.up)
        vv, rr, uu = _dot3(view, view), _dot3(right, right), _dot3(up, up)
        plx, ply = F(cam.pixel_length[0]), F(cam.pixel_length[1])
        v = (gB[..., :3] - pos).astype(F)
        z = _dot(v, view) / vv
        ax = -((_dot(v, right) / rr) / (plx * z))
        ay = -((_dot(v, up) / uu) / (ply * z))
        fx = ax + F(W) * F(0.5)
        fy = ay + F(H) * F(0.5)
    assert fx.dtype == F and fy.dtype == F and z.dtype == F
    return fx, fy, z


class Temporal:
    def __init__(self, h, w, **params):
        self.H, self.W = h, w
        self.p = dict(DEFAULTS, **params)
        self.reset()

    def reset(self):
        self.frames, self.batch, self.prev_samples, self.last_case, self.cam = 0, None, 0.0, 0, None

    # ---- the blend, the same in all three cases ------------------------------------------------
    def _blend(self, c, b, mean, mu1, mu2, h):
        maxh = F(self.p["max_history"])
        with np.errstate(all="ignore"):
            hn = (h + F(b)).astype(F)
            if maxh > 0:
                hn = np.where(hn < maxh, hn, maxh).astype(F)
            a = (F(b) / hn).astype(F)
            mean = (mean + a[..., None] * (c - mean)).astype(F)
            l = lum(c)
            mu1 = (mu1 + a * (l - mu1)).astype(F)
            mu2 = (mu2 + a * (l * l - mu2)).astype(F)
        assert mean.dtype == F and mu1.dtype == F and mu2.dtype == F and hn.dtype == F
        self.mean, self.mu1, self.mu2, self.h = mean, mu1, mu2, hn

    def case_of(self, cam, samples):
        if self.frames == 0:
            return EMPTY, float(samples)
        if _cam_key(cam) == _cam_key(self.cam) and samples > self.prev_samples:
            return SAME_VIEW, float(F(samples) - F(self.prev_samples))
        return NEW_VIEW, float(samples)

    def frame(self, cam, rgb, samples, gA, gB, alb):
        """rgb (H, W, 3) accumulated, gA / gB / alb (H, W, 4), float32."""
        H, W = self.H, self.W
        rgb, gA, gB, alb = (np.ascontiguousarray(v, F) for v in (rgb, gA, gB, alb))
        kind, b = self.case_of(cam, samples)
        if self.frames > 0 and b != self.batch:
            raise ValueError("batch size differs")
        if self.p["max_history"] > 0 and b > self.p["max_history"]:
            raise ValueError("max_history is smaller than one batch")
        zero3, zero = np.zeros((H, W, 3), F), np.zeros((H, W), F)
        with np.errstate(all="ignore"):
            if kind == SAME_VIEW:
                c = ((rgb - self.prev) / F(b)).astype(F)
                if self.p["demodulate"]:
                    c = _modulate(c, self.alb[..., :3], True)
                hit = self.gA[..., 3].copy().view(np.int32) >= 0
                mean = np.where(hit[..., None], self.mean, zero3)
                mu1, mu2, h = (np.where(hit, v, zero) for v in (self.mu1, self.mu2, self.h))
            else:
                c = (rgb / F(samples)).astype(F)
                if self.p["demodulate"]:
                    c = _modulate(c, alb[..., :3], True)
                if kind == EMPTY:
                    mean, mu1, mu2, h = zero3, zero, zero, zero
                    self.kept = np.zeros((H, W), bool)
                else:
                    mean, mu1, mu2, h = self._gather(gA, gB)
                self.gA, self.gB, self.alb = gA.copy(), gB.copy(), alb.copy()
            self._blend(c, b, mean, mu1, mu2, h)
        self.prev = rgb.copy()
        self.cam, self.prev_samples, self.batch, self.last_case = cam, float(samples), b, kind
        self.frames += 1
        return kind

    def _gather(self, gA, gB):
        """The history of every new pixel from the four bilinear taps in the stored frame."""
        H, W = self.H, self.W
        fx, fy, z = reproject_coords(self.cam, gB, W, H)
        mat = gA[..., 3].copy().view(np.int32)
        omat = self.gA[..., 3].copy().view(np.int32)
        Np, Pp, tp = gA[..., :3], gB[..., :3], gB[..., 3]
        ok = (mat >= 0) & (z > 0) & (fx >= F(-1)) & (fx < F(W)) & (fy >= F(-1)) & (fy < F(H))
        x0f = np.floor(np.where(ok, fx, F(0))).astype(F)
        y0f = np.floor(np.where(ok, fy, F(0))).astype(F)
        x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
        tx, ty = (fx - x0f).astype(F), (fy - y0f).astype(F)
        wx, wy = (F(1) - tx, tx), (F(1) - ty, ty)
        tol = F(self.p["plane_tol"]) * tp
        sm, s1, s2, sh, wsum = np.zeros((H, W, 3), F), *(np.zeros((H, W), F) for _ in range(4))
        self.tap_valid = []
        for k in range(4):   # (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1)
            qx, qy = x0 + (k & 1), y0 + (k >> 1)
            inside = ok & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
            cx, cy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
            valid = inside & (omat[cy, cx] == mat)
            valid &= ~(_dot(Np, self.gA[cy, cx, :3]) < F(self.p["min_ndot"]))
            valid &= ~(np.abs(_dot(Np, self.gB[cy, cx, :3] - Pp)) > tol)
            w = (wx[k & 1] * wy[k >> 1]).astype(F)
            sm = np.where(valid[..., None], sm + w[..., None] * self.mean[cy, cx], sm).astype(F)
            s1 = np.where(valid, s1 + w * self.mu1[cy, cx], s1).astype(F)
            s2 = np.where(valid, s2 + w * self.mu2[cy, cx], s2).astype(F)
            sh = np.where(valid, sh + w * self.h[cy, cx], sh).astype(F)
            wsum = np.where(valid, wsum + w, wsum).astype(F)
            self.tap_valid.append(valid)
        kept = wsum > 0
        ws = np.where(kept, wsum, F(1))
        zero = np.zeros((H, W), F)
        self.kept, self.fx, self.fy = kept, fx, fy
        return (np.where(kept[..., None], sm / ws[..., None], F(0)).astype(F), np.where(kept, s1 / ws, zero).astype(F),
                np.where(kept, s2 / ws, zero).astype(F), np.where(kept, sh / ws, zero).astype(F))

    # ---- resolve ------------------------------------------------------------------------------
    def resolve(self):
        """(rgb (H, W, 3), var (H, W), h (H, W)) as pt_temporal_resolve writes them."""
        H, W = self.H, self.W
        with np.errstate(all="ignore"):
            rgb = self.mean.copy()
            if self.p["demodulate"]:
                rgb = _modulate(rgb, self.alb[..., :3], False)
            mat = self.gA[..., 3].copy().view(np.int32)
            b = F(self.batch)
            thr = F(self.p["min_frames"]) * b
            temporal = (np.maximum(F(0), self.mu2 - self.mu1 * self.mu1) * (b / self.h)).astype(F)
            l = lum(self.mean)
            s1, s2, cnt = (np.zeros((H, W), F) for _ in range(3))
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    lq, inside = _shift(l, dy, dx)
                    mq, _ = _shift(mat, dy, dx)
                    valid = inside & (mq == mat)
                    s1 = np.where(valid, s1 + lq, s1).astype(F)
                    s2 = np.where(valid, s2 + lq * lq, s2).astype(F)
                    cnt = np.where(valid, cnt + F(1), cnt).astype(F)
            m = (s1 / cnt).astype(F)
            spatial = np.maximum(F(0), s2 / cnt - m * m).astype(F)
            self.on_temporal = (mat >= 0) & (self.h >= thr)
            var = np.where(mat < 0, F(0), np.where(self.h >= thr, temporal, spatial)).astype(F)
        assert rgb.dtype == F and var.dtype == F
        return rgb, var, self.h.copy()

    def image(self, var_params=None):
        """pt_temporal_image: resolve, then with var_params (levels, sigma_l, sigma_n, sigma_p, demodulate)
        the variance-guided filter on the resolved image (samples = 1) -> (rgb, var, h)."""
        rgb, var, h = self.resolve()
        if var_params is not None:
            rgb, var = atrous_var_ref(rgb, 1.0, var, self.gA, self.gB, self.alb, var_params.levels, var_params.sigma_l,
                                      var_params.sigma_n, var_params.sigma_p, bool(var_params.demodulate))
        return rgb, var, h


# ---- synthetic views ---------------------------------------------------------------------------
def look_at_camera(eye, target, fovy_deg, W, H):
    """An orthogonal camera frame like the scene loader's: view normalised, right = view x (0, 1, 0)
    (not unit length), up = right x view; pixel lengths from the field of view."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    view = target - eye
    view /= np.linalg.norm(view)
    right = np.cross(view, [0.0, 1.0, 0.0])
    up = np.cross(right, view)
    yscaled = np.tan(np.radians(fovy_deg))
    xscaled = yscaled * W / H
    return make_camera(eye, view, up, right, (2 * xscaled / W, 2 * yscaled / H), res=(W, H), look_at=target)


def camera_dirs(cam, W, H):
    """float64 ray directions of the deterministic camera rays (raygen_at without jitter), (H, W, 3)."""
    x = np.arange(W, dtype=np.float64)[None, :, None] - W * 0.5
    y = np.arange(H, dtype=np.float64)[:, None, None] - H * 0.5
    view, up, right = (np.asarray(v, np.float64) for v in (cam.view, cam.up, cam.right))
    d = view - right * cam.pixel_length[0] * x - up * cam.pixel_length[1] * y
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def crease_gbuffer(cam, W, H, miss_rows=(), miss_band=None):
    """First hits of cam's rays on two planes of different materials meeting at a crease (a floor y = -1,
    material 1, in front of a back wall z = -6, material 2); rows `miss_rows` of the image, and the hits
    whose world x lies in the interval `miss_band`, are forced to misses: gA, gB, alb as (H, W, 4) float32
    planes in the G-buffer's layout."""
    o = np.asarray(cam.position, np.float64)
    d = camera_dirs(cam, W, H)
    with np.errstate(all="ignore"):
        t_floor = np.where(d[..., 1] < 0, (-1.0 - o[1]) / d[..., 1], np.inf)
        t_wall = np.where(d[..., 2] < 0, (-6.0 - o[2]) / d[..., 2], np.inf)
    t = np.minimum(t_floor, t_wall)
    floor = t_floor <= t_wall
    hit = np.isfinite(t) & (t > 0)
    if len(miss_rows):
        hit[list(miss_rows), :] = False
    t = np.where(hit, t, 1.0)
    P = o + d * t[..., None]
    if miss_band is not None:
        hit &= ~((P[..., 0] >= miss_band[0]) & (P[..., 0] < miss_band[1]))
    gA, gB, alb = (np.zeros((H, W, 4), F) for _ in range(3))
    n = np.where(floor[..., None], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0])
    gA[..., :3] = np.where(hit[..., None], n, 0.0)
    gA[..., 3] = np.where(hit, np.where(floor, 1, 2), -1).astype(np.int32).view(F)
    gB[..., :3] = np.where(hit[..., None], P, 0.0)
    gB[..., 3] = np.where(hit, t, -1.0)
    alb[..., :3] = np.where(hit[..., None], np.where(floor[..., None], [0.7, 0.6, 0.5], [0.3, 0.8, 0.9]), 1.0)
    return gA, gB, alb
