"""Reference for the adaptive-sampling tests (a helper, not collected by pytest): DESIGN.md §13 restated
in numpy with every intermediate in np.float32, in the stated order, so the GPU results must equal it
bit for bit (numpy's float32 +, -, *, / and sqrt are single correctly rounded IEEE operations, as the
kernels' are).  lum and the albedo rule are tests/denoise_var_ref.py's and tests/denoise_ref.py's.

Adaptive is the state of a pt_adaptive object: update / select / set_mask / apply / resolve are the
object's calls of the same names.  A BLOCK is 64 consecutive pixels of the image in row-major order;
block_of, expand and dilate_blocks are the vectorised geometry, the *_brute functions the per-pixel
loops tests/test_adaptive_cpu.py compares them with.
"""
import numpy as np

from denoise_ref import F, _modulate
from denoise_var_ref import lum

BLOCK = 64


def nblocks(h, w):
    return (h * w + BLOCK - 1) // BLOCK


def block_of(h, w):
    """(h, w) int64: the block of every pixel."""
    return (np.arange(h * w, dtype=np.int64) // BLOCK).reshape(h, w)


def expand(per_block, h, w):
    """A per-block array as an (h, w) plane."""
    return np.asarray(per_block)[block_of(h, w)]


def dilate(hot, r):
    """(h, w) bool: some pixel of the (2r + 1)^2 box around the pixel, clipped to the image, is hot."""
    hot = np.asarray(hot, bool)
    h, w = hot.shape
    out = np.zeros((h, w), bool)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
            xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
            out[yd, xd] |= hot[ys, xs]
    return out


def dilate_blocks(hot, r):
    """(nblocks,) uint32: act of every block from the hot plane."""
    h, w = np.asarray(hot).shape
    d = dilate(hot, r).reshape(-1)
    act = np.zeros(nblocks(h, w), np.uint32)
    np.maximum.at(act, np.arange(h * w) // BLOCK, d.astype(np.uint32))
    return act


def dilate_blocks_brute(hot, r):
    """The same with a loop over every pixel and every box cell."""
    hot = np.asarray(hot, bool)
    h, w = hot.shape
    act = np.zeros(nblocks(h, w), np.uint32)
    for i in range(h * w):
        y, x = divmod(i, w)
        for yy in range(y - r, y + r + 1):
            for xx in range(x - r, x + r + 1):
                if 0 <= yy < h and 0 <= xx < w and hot[yy, xx]:
                    act[i // BLOCK] = 1
    return act


def block_pixels_brute(h, w, b):
    """The (y, x) of block b's pixels, by a loop over the image."""
    return [(y, x) for y in range(h) for x in range(w) if (y * w + x) // BLOCK == b]


class Adaptive:
    def __init__(self, h, w, base=None):
        self.h, self.w = h, w
        self.reset(base)

    def reset(self, base=None):
        h, w = self.h, self.w
        self.prev = np.zeros((h, w, 3), F) if base is None else np.array(base, F).reshape(h, w, 3)
        self.m1 = np.zeros((h, w), F)
        self.m2 = np.zeros((h, w), F)
        self.hot = np.ones((h, w), np.uint8)
        self.nb = np.zeros(nblocks(h, w), np.uint32)
        self.act = np.ones(nblocks(h, w), np.uint32)
        self.batch_samples = None

    def set_mask(self, mask):
        mask = np.asarray(mask).reshape(-1)
        assert mask.size == self.nb.size
        self.act = (mask != 0).astype(np.uint32)

    def update(self, rgb, batch_samples, alb=None):
        """Pixels of inactive blocks keep their planes; their rgb is not used (NaN there changes nothing)."""
        rgb = np.ascontiguousarray(rgb, F).reshape(self.h, self.w, 3)
        on = expand(self.act, self.h, self.w) != 0
        with np.errstate(all="ignore"):
            d = ((rgb - self.prev) / F(batch_samples)).astype(F)
            if alb is not None:
                d = _modulate(d, np.asarray(alb, F)[..., :3], True)
            l = lum(d)
            self.m1 = np.where(on, (self.m1 + l).astype(F), self.m1)
            self.m2 = np.where(on, (self.m2 + l * l).astype(F), self.m2)
        self.prev = np.where(on[..., None], rgb, self.prev)
        self.nb = (self.nb + (self.act != 0)).astype(np.uint32)
        self.batch_samples = float(batch_samples)

    def error(self, floor):
        """(h, w) float32: e of every pixel (garbage where nb < 2; select masks those)."""
        nbf = expand(self.nb, self.h, self.w).astype(F)
        with np.errstate(all="ignore"):
            mean = self.m1 / nbf
            ex2 = self.m2 / nbf
            vm = np.maximum(F(0), ex2 - mean * mean) / (nbf - F(1))
            e = np.sqrt(vm) / (mean + F(floor))
        assert e.dtype == F
        return e

    def select(self, threshold, floor, min_batches, dilate_r):
        nbp = expand(self.nb, self.h, self.w)
        e = self.error(floor)
        with np.errstate(all="ignore"):
            hot = np.where(nbp < min_batches, True, e > F(threshold))   # (NaN > x is False: not hot)
        self.hot = hot.astype(np.uint8)
        self.act = dilate_blocks(hot, dilate_r)
        return int(self.act.sum())

    def apply(self, cmask):
        return np.where(self.act != 0, np.asarray(cmask, np.uint32), np.uint32(0)).astype(np.uint32)

    def resolve(self, rgb):
        """((h, w, 3), (h, w)) float32: rgb / (nb * bs), and pt_moments_variance's expression per block."""
        rgb = np.ascontiguousarray(rgb, F).reshape(self.h, self.w, 3)
        nbp = expand(self.nb, self.h, self.w)
        nf = nbp.astype(F)
        bs = F(self.batch_samples)
        with np.errstate(all="ignore"):
            ns = nf * bs
            out = np.where((nbp != 0)[..., None], rgb / ns[..., None], F(0)).astype(F)
            scale = ns / ((nf - F(1)) * ns)
            mean = self.m1 / nf
            ex2 = self.m2 / nf
            var = np.where(nbp >= 2, np.maximum(F(0), ex2 - mean * mean) * scale, F(0)).astype(F)
        assert out.dtype == F and var.dtype == F
        return out, var
