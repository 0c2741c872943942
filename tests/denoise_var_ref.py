"""References for the variance tests (a helper, not collected by pytest): DESIGN.md §11 restated in
numpy with every intermediate in np.float32, in the stated order, so the GPU results must equal them
bit for bit (numpy's float32 +, -, *, / and sqrt are single correctly rounded IEEE operations, as the
kernels' are).  The shared pieces (tap kernel, shifts, modulation) are tests/denoise_ref.py's.

Moments: the state of a pt_moments object; moments_update is one pt_moments_update, moments_variance
is pt_moments_variance.  atrous_var_ref is pt_denoiser_run_var / pt_denoise_var_host.
"""
import numpy as np

from denoise_ref import F, H5, _dot, _modulate, _shift

G3 = (F(0.25), F(0.5), F(0.25))
V_EPS = F(2.0 ** -30)


def lum(c):
    return (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]


class Moments:
    def __init__(self, h, w, base=None):
        self.reset(h, w, base)

    def reset(self, h, w, base=None):
        self.prev = np.zeros((h, w, 3), F) if base is None else np.array(base, F).reshape(h, w, 3)
        self.m1 = np.zeros((h, w), F)
        self.m2 = np.zeros((h, w), F)
        self.batches = 0
        self.batch_samples = None

    def update(self, rgb, batch_samples, alb=None):
        """alb: (H, W, >= 3) or None."""
        rgb = np.ascontiguousarray(rgb, F)
        with np.errstate(all="ignore"):
            d = ((rgb - self.prev) / F(batch_samples)).astype(F)
            if alb is not None:
                d = _modulate(d, np.asarray(alb, F)[..., :3], True)
            l = lum(d)
            self.m1 = (self.m1 + l).astype(F)
            self.m2 = (self.m2 + l * l).astype(F)
        self.prev = rgb.copy()
        self.batches += 1
        self.batch_samples = float(batch_samples)

    def variance(self, samples):
        nf = F(self.batches)
        with np.errstate(all="ignore"):
            scale = (nf * F(self.batch_samples)) / ((nf - F(1)) * F(samples))
            mean = self.m1 / nf
            ex2 = self.m2 / nf
            var = np.maximum(F(0), ex2 - mean * mean) * scale
        assert var.dtype == F and scale.dtype == F
        return var


def atrous_var_ref(rgb, samples, var, gA, gB, alb, levels, sigma_l, sigma_n, sigma_p, demodulate=True):
    """rgb (H, W, 3), var (H, W), gA / gB / alb (H, W, 4), all float32 -> ((H, W, 3), (H, W)) float32."""
    rgb, var, gA, gB, alb = (np.ascontiguousarray(v, F) for v in (rgb, var, gA, gB, alb))
    with np.errstate(all="ignore"):
        sl = F(sigma_l)
        inv_n = F(1) / (F(sigma_n) * F(sigma_n))
        inv_p = F(1) / (F(sigma_p) * F(sigma_p))
        c = (rgb / F(samples)).astype(F)
        if demodulate:
            c = _modulate(c, alb[..., :3], True)
        v = var.copy()
        mat = gA[..., 3].copy().view(np.int32)
        hit = mat >= 0
        Np, Pp = gA[..., :3], gB[..., :3]
        for i in range(levels):
            s = 1 << i
            gs = np.zeros(v.shape, F)
            gw = np.zeros(v.shape, F)
            for ey in range(-1, 2):
                for ex in range(-1, 2):
                    vq, inside = _shift(v, ey, ex)
                    mq, _ = _shift(mat, ey, ex)
                    valid = inside & (mq >= 0)
                    kk = G3[ex + 1] * G3[ey + 1]
                    gs = np.where(valid, gs + kk * vq, gs)
                    gw = np.where(valid, gw + kk, gw)
            g = gs / np.where(hit, gw, F(1))
            rl = (F(1) / (sl * np.sqrt(np.maximum(F(0), g) + V_EPS))).astype(F)
            lp = lum(c)
            acc = np.zeros_like(c)
            vsum = np.zeros(v.shape, F)
            wsum = np.zeros(v.shape, F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    cq, inside = _shift(c, dy * s, dx * s)
                    vq, _ = _shift(v, dy * s, dx * s)
                    Nq, _ = _shift(Np, dy * s, dx * s)
                    Pq, _ = _shift(Pp, dy * s, dx * s)
                    mq, _ = _shift(mat, dy * s, dx * s)
                    valid = inside & (mq >= 0)
                    k = H5[dx + 2] * H5[dy + 2]
                    xl = np.abs(lum(cq) - lp) * rl
                    xn = np.maximum(F(0), F(1) - _dot(Np, Nq)) * inv_n
                    e = _dot(Np, Pq - Pp)
                    xp = (e * e) * inv_p
                    w = (k / (((F(1) + xl) * (F(1) + xn)) * (F(1) + xp))).astype(F)
                    acc = np.where(valid[..., None], acc + w[..., None] * cq, acc)
                    vsum = np.where(valid, vsum + (w * w) * vq, vsum)
                    wsum = np.where(valid, wsum + w, wsum)
            ws = np.where(hit, wsum, F(1))
            c = np.where(hit[..., None], acc / ws[..., None], c).astype(F)
            v = np.where(hit, vsum / (ws * ws), v).astype(F)
        if demodulate:
            c = _modulate(c, alb[..., :3], False)
    assert c.dtype == F and v.dtype == F
    return c, v
