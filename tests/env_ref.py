"""numpy restatements of the environment's definitions, DESIGN.md §19 (a helper, not collected by pytest).

  decode_rgbe / decode_hdr   a Radiance .hdr file's floats, written from the format's description alone
  rotation                   the world-to-map matrix of rotate_deg (float64 products, one rounding to float32)
  pad                        the gutter rule: the padded (n + 2, n + 2, 4) map of an (n, n, 3) octahedral map
  resample                   the lat-long -> octahedral resampler, in float64 (returned unrounded)
  lookup                     L(d) in a chosen dtype: float32 is the device's own arithmetic, operation by
                             operation (every numpy float32 operation is one correctly rounded IEEE operation),
                             float64 is the yardstick of the path replay (tests/env_path_ref.py)

It shares no code with csrc/.  math.sin / math.cos are the C library's, which the host code calls too.
"""
import math

import numpy as np

F = np.float32


# ---- Radiance HDR --------------------------------------------------------------------------------------
def decode_rgbe(rgbe):
    """(..., 4) uint8 -> (..., 3) float32: m * 2^(e - 136), 0 where e == 0."""
    rgbe = np.asarray(rgbe, np.uint8)
    e = rgbe[..., 3].astype(np.int32)
    f = np.where(e > 0, np.ldexp(np.float64(1), e - 136), 0.0)
    out = rgbe[..., :3].astype(np.float64) * f[..., None]
    assert np.array_equal(out.astype(F).astype(np.float64), out)      # (exact in float32, denormals included)
    return out.astype(F)


def decode_hdr(data):
    """The pixels of a '-Y H +X W' file, (H, W, 3) float32 in file order: flat or new-style RLE scanlines."""
    head, sep, rest = data.partition(b"\n\n")
    assert sep and head.startswith(b"#?") and b"\nFORMAT=32-bit_rle_rgbe" in head
    dims, _, body = rest.partition(b"\n")
    my, H, px, W = dims.split(b" ")
    assert (my, px) == (b"-Y", b"+X")
    H, W = int(H), int(W)
    out = np.zeros((H, W, 4), np.uint8)
    pos = 0
    for y in range(H):
        if 8 <= W < 32768 and body[pos:pos + 2] == b"\x02\x02" and body[pos + 2] < 128 and \
                (body[pos + 2] << 8 | body[pos + 3]) == W:
            pos += 4
            for k in range(4):
                x = 0
                while x < W:
                    n = body[pos]
                    pos += 1
                    if n > 128:
                        out[y, x:x + n - 128, k] = body[pos]
                        pos += 1
                        x += n - 128
                    else:
                        assert n > 0
                        out[y, x:x + n, k] = np.frombuffer(body[pos:pos + n], np.uint8)
                        pos += n
                        x += n
                assert x == W
        else:
            out[y] = np.frombuffer(body[pos:pos + 4 * W], np.uint8).reshape(W, 4)
            pos += 4 * W
    assert pos == len(body)
    return decode_rgbe(out)


def flat_hdr(rgbe):
    """A hand-built file of flat scanlines from (H, W, 4) uint8 RGBE pixels."""
    rgbe = np.asarray(rgbe, np.uint8)
    H, W = rgbe.shape[:2]
    return b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y %d +X %d\n" % (H, W) + rgbe.tobytes()


# ---- the map ---------------------------------------------------------------------------------------------
def rotation(rotate_deg):
    """Rx Ry Rz (degrees, world to map), each entry (a b + c d) + e f in float64, then float32: (3, 3)."""
    mats = []
    for a in range(3):
        t = float(F(rotate_deg[a])) * (math.pi / 180.0)
        c, s = math.cos(t), math.sin(t)
        u, v = (a + 1) % 3, (a + 2) % 3
        m = [[1.0 if r == q else 0.0 for q in range(3)] for r in range(3)]
        m[u][u], m[u][v], m[v][u], m[v][v] = c, -s, s, c
        mats.append(m)

    def mul(A, B):
        return [[(A[r][0] * B[0][q] + A[r][1] * B[1][q]) + A[r][2] * B[2][q] for q in range(3)] for r in range(3)]
    return np.array(mul(mul(mats[0], mats[1]), mats[2]), np.float64).astype(F)


def pad(texels):
    """The padded map of (n, n, 3) texels [row j along z, column i along x]: (n + 2, n + 2, 4), alpha 0.
    A step across an edge of the square lands at the mirrored position along that edge; a corner is the
    rule applied twice (the opposite corner)."""
    t = np.asarray(texels)
    n = t.shape[0]
    out = np.zeros((n + 2, n + 2, 4), t.dtype)

    def src(i, j):
        """The interior texel (column, row) that padded column i, row j (-1 .. n) shows."""
        for _ in range(2):
            if i < 0:
                i, j = 0, n - 1 - j
            elif i > n - 1:
                i, j = n - 1, n - 1 - j
            elif j < 0:
                i, j = n - 1 - i, 0
            elif j > n - 1:
                i, j = n - 1 - i, n - 1
        return i, j
    for j in range(-1, n + 1):
        for i in range(-1, n + 1):
            si, sj = src(i, j)
            out[j + 1, i + 1, :3] = t[sj, si]
    return out


def texel_direction(n):
    """The directions (not normalised) of the n x n texel centres, float64: (n, n, 3) [row j, column i]."""
    c = (2.0 * (np.arange(n, dtype=np.float64) + 0.5)) / n - 1.0
    pz, px = np.meshgrid(c, c, indexing="ij")
    ay = (1.0 - np.abs(px)) - np.abs(pz)
    fold = ay < 0
    x = np.where(fold, (1.0 - np.abs(pz)) * np.where(px >= 0, 1.0, -1.0), px)
    z = np.where(fold, (1.0 - np.abs(px)) * np.where(pz >= 0, 1.0, -1.0), pz)
    return np.stack([x, ay, z], -1)


def default_size(height):
    return max(1, min(2048, height // 2))


def resample(src, n):
    """The octahedral map of a lat-long (H, W, 3) image in float64: (texels (n, n, 3), largest |source texel|
    each texel reads (n, n))."""
    src = np.asarray(src, F).astype(np.float64)
    H, W = src.shape[:2]
    fx, fy = (W + 4 * n - 1) // (4 * n), (H + 2 * n - 1) // (2 * n)
    if fx > 1 or fy > 1:                                # block means, the last block of a row or column smaller
        Hr, Wr = (H + fy - 1) // fy, (W + fx - 1) // fx
        img = np.zeros((Hr, Wr, 3))
        big = np.zeros((Hr, Wr))
        for y in range(Hr):
            for x in range(Wr):
                blk = src[y * fy:(y + 1) * fy, x * fx:(x + 1) * fx].reshape(-1, 3)
                img[y, x] = blk.sum(0) / len(blk)
                big[y, x] = np.abs(blk).max()
    else:
        Hr, Wr, img, big = H, W, src, np.abs(src).max(-1)
    d = texel_direction(n)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    cy = np.clip(y / np.sqrt((x * x + y * y) + z * z), -1.0, 1.0)
    phi, theta = np.arctan2(x, -z), np.arccos(cy)
    sx = (phi / (2.0 * math.pi) + 0.5) * Wr - 0.5
    sy = (theta / math.pi) * Hr - 0.5
    fx, fy = np.floor(sx), np.floor(sy)
    wx, wy = (sx - fx)[..., None], (sy - fy)[..., None]
    xa, xb = fx.astype(np.int64) % Wr, (fx.astype(np.int64) + 1) % Wr
    ya, yb = np.clip(fy.astype(np.int64), 0, Hr - 1), np.clip(fy.astype(np.int64) + 1, 0, Hr - 1)
    A, B, C, D = img[ya, xa], img[ya, xb], img[yb, xa], img[yb, xb]
    top, bot = A + (B - A) * wx, C + (D - C) * wx
    reads = np.maximum(np.maximum(big[ya, xa], big[ya, xb]), np.maximum(big[yb, xa], big[yb, xb]))
    return top + (bot - top) * wy, reads


def lookup(padded, scale, rot, d, dt=F, transpose=False):
    """L(d) for directions d (m, 3) in dtype dt, §19's operations in §19's order.  padded: (n + 2, n + 2, 4);
    rot: (3, 3) float32.  transpose: one deliberate error (the map read with its axes swapped)."""
    P = np.asarray(padded, F).astype(dt)
    n = P.shape[0] - 2
    R = np.asarray(rot, F).astype(dt)
    d = np.asarray(d, dt)
    one, half = dt(1), dt(0.5)
    with np.errstate(all="ignore"):
        r = [(R[k, 0] * d[:, 0] + R[k, 1] * d[:, 1]) + R[k, 2] * d[:, 2] for k in range(3)]
        s = (np.abs(r[0]) + np.abs(r[1])) + np.abs(r[2])
        ok = (s > 0) & (s < np.inf)
        s1 = np.where(ok, s, one)
        px, pz = r[0] / s1, r[2] / s1
        fold = r[1] < 0
        qx = (one - np.abs(pz)) * np.where(px >= 0, one, -one)
        qz = (one - np.abs(px)) * np.where(pz >= 0, one, -one)
        px, pz = np.where(fold, qx, px), np.where(fold, qz, pz)
        px, pz = np.where(ok, px, dt(0)), np.where(ok, pz, dt(0))
        nf = dt(n)
        fx = (px * half + half) * nf + half
        fz = (pz * half + half) * nf + half
        ix = np.clip(np.floor(fx).astype(np.int64), 0, n)
        iz = np.clip(np.floor(fz).astype(np.int64), 0, n)
        wx, wz = (fx - ix.astype(dt))[:, None], (fz - iz.astype(dt))[:, None]
        if transpose:
            a, b, c, e = P[ix, iz], P[ix + 1, iz], P[ix, iz + 1], P[ix + 1, iz + 1]
        else:
            a, b, c, e = P[iz, ix], P[iz, ix + 1], P[iz + 1, ix], P[iz + 1, ix + 1]
        t = a + (b - a) * wx
        u = c + (e - c) * wx
        out = ((t + (u - t) * wz) * dt(F(scale)))[:, :3]
    assert out.dtype == dt
    return np.where(ok[:, None], out, dt(0))
