"""The corner detector and binary descriptor of this project in numpy: the contract `stitching_amd.FeatureEstimator` is tested against,
byte for byte.

This is the project's OWN detector, in the family of oriented FAST + rotated BRIEF.  It is NOT cv.ORB and does not claim the names
"orb" / "sift".  It is integer only; what needs floating point (level sizes, quotas, the direction tables, the rotation of the
pattern) is computed in float64 on the host.  The only thing taken from the package is the base pattern, a table of 256 point pairs.

For one u8 BGR image (h0 x w0), an optional u8 mask (h0 x w0) and nfeatures, nlevels, scale, fast_threshold:
  grey         g = (1868 B + 9617 G + 4899 R + 8192) >> 14
  pyramid      level 0 is g; level l has size (floor(w0 / scale**l + 0.5), floor(h0 / scale**l + 0.5)) and is the exact linear resize
               (cv::resize INTER_LINEAR_EXACT: 8.8 fixed point rows, 16.16 columns) of level l - 1; the first level with a side below
               33 is dropped with every level after it
  blur         B = (sum k_i k_j g + 128) >> 8 with k = [1 4 6 4 1], border REFLECT_101, no intermediate rounding
  score        ring r_0 .. r_15 of radius 3 (Bresenham, from (0, -3), clockwise), centre c:
               s = max_a max(min_{k<9} (r_{a+k} - c), min_{k<9} (c - r_{a+k})); a candidate lies in [16, w - 17] x [16, h - 17], has
               s > fast_threshold and s strictly above the scores of its 8 neighbours
  mask         candidate (x, y) of level l is kept iff mask[((2y+1) h0) // (2 h_l), ((2x+1) w0) // (2 w_l)] != 0
  response     Ix = g(x+1, y) - g(x-1, y), Iy likewise; over the 7 x 7 window a = sum Ix^2, b = sum Ix Iy, c = sum Iy^2;
               R = (25 (a c - b^2) - (a + c)^2) >> 16 in int64 (arithmetic shift); |R| < 2^33
  selection    quotas n_l: q = 1 / scale, d = nfeatures (1 - q) / (1 - q**L), n_l = floor(d + 0.5) but no more than nfeatures less the
               quotas before it, d *= q; the last of the L kept levels takes max(nfeatures - sum, 0).  A level keeps its first n_l
               candidates by (R descending, y, x); keypoints are listed by level, then in that order
  orientation  over the disc u^2 + v^2 <= 225: m10 = sum u g, m01 = sum v g; bin = argmax_b (m10 CX[b] + m01 CY[b]), b in 0 .. 35,
               CX[b] = rint(16384 cos(2 pi b / 36)), CY with the sine; ties go to the smallest b
  descriptor   bit i (byte i // 8, bit i % 8 from the least significant) = B(k + P_bin[i]) < B(k + Q_bin[i]); P_b, Q_b are the base
               pattern's points turned by theta = 2 pi b / 36: (rint(px cos - py sin), rint(px sin + py cos)) in float64
"""
import math

import numpy as np

from stitching_amd.feature_estimation import pattern  # the table of 256 point pairs: data

BORDER = 16
MIN_SIDE = 33
BINS = 36
# (dx, dy) of the 16 ring pixels, from (0, -3) clockwise (y grows downwards)
RING = ((0, -3), (1, -3), (2, -2), (3, -1), (3, 0), (3, 1), (2, 2), (1, 3), (0, 3), (-1, 3), (-2, 2), (-3, 1), (-3, 0), (-3, -1), (-2, -2),
        (-1, -3))
NO_SCORE = -256  # where the ring does not fit into the level

_th = 2.0 * np.pi * np.arange(BINS, dtype=np.float64) / BINS
CX = np.rint(16384.0 * np.cos(_th)).astype(np.int64)
CY = np.rint(16384.0 * np.sin(_th)).astype(np.int64)
_v, _u = np.mgrid[-15:16, -15:16]
_disc = _u * _u + _v * _v <= 225
DISC_U, DISC_V = _u[_disc].astype(np.int64), _v[_disc].astype(np.int64)


def grey(img):
    p = np.asarray(img, np.uint8).astype(np.int64)
    return ((1868 * p[..., 0] + 9617 * p[..., 1] + 4899 * p[..., 2] + 8192) >> 14).astype(np.uint8)


def _coeffs(src_n, dst_n):
    scale = 1.0 / (float(dst_n) / float(src_n))
    f = scale * (np.arange(dst_n, dtype=np.float64) + 0.5) - 0.5
    i = np.floor(f).astype(np.int64)
    inner = (i >= 0) & (i < src_n - 1) & (src_n > 1)
    ofs = np.where(inner, i, np.where((i >= src_n - 1) & (i >= 0) & (src_n > 1), src_n - 1, 0))
    c1 = np.where(inner, np.rint((f - i) * 256.0), 0).astype(np.int64)
    return ofs, 256 - c1, c1, inner


def resize_linear_exact(src, size):
    """The exact linear resize of one u8 plane to size = (w, h): the arithmetic stitching_amd.resize_linear_exact is tested for."""
    s = np.asarray(src, np.uint8).astype(np.int64)
    sh, sw = s.shape
    ox, a0, a1, _ = _coeffs(sw, int(size[0]))
    oy, b0, b1, iy = _coeffs(sh, int(size[1]))
    h = s[:, ox] * a0[None, :] + s[:, np.minimum(ox + 1, sw - 1)] * a1[None, :]
    v = h[oy] * b0[:, None] + h[np.minimum(oy + 1, sh - 1)] * b1[:, None]
    return np.where(iy[:, None], (v + 32768) >> 16, (h[oy] + 128) >> 8).astype(np.uint8)


def level_sizes(w0, h0, nlevels, scale):
    out = []
    for l in range(nlevels):
        f = float(scale) ** l
        w, h = int(math.floor(w0 / f + 0.5)), int(math.floor(h0 / f + 0.5))
        if w < MIN_SIDE or h < MIN_SIDE:
            break
        out.append((w, h))
    return out


def quotas(nfeatures, scale, levels):
    if levels == 0:
        return []
    q = 1.0 / float(scale)
    d = nfeatures * (1.0 - q) / (1.0 - q ** levels)
    out = []
    for _ in range(levels - 1):
        out.append(min(int(math.floor(d + 0.5)), nfeatures - sum(out)))
        d *= q
    out.append(max(nfeatures - sum(out), 0))
    return out


def pyramid(g, nlevels, scale):
    out = []
    for w, h in level_sizes(g.shape[1], g.shape[0], nlevels, scale):
        out.append(g if not out else resize_linear_exact(out[-1], (w, h)))
    return out


def blur(g):
    p = np.pad(np.asarray(g, np.uint8).astype(np.int64), 2, mode="reflect")  # numpy's "reflect" is REFLECT_101
    k = (1, 4, 6, 4, 1)
    h, w = g.shape
    rows = sum(k[i] * p[:, i:i + w] for i in range(5))
    return ((sum(k[j] * rows[j:j + h] for j in range(5)) + 128) >> 8).astype(np.uint8)


def score_map(g):
    """int16 (h, w): the score where the radius-3 ring lies inside the level, NO_SCORE elsewhere."""
    g = np.asarray(g, np.uint8).astype(np.int16)
    h, w = g.shape
    out = np.full((h, w), NO_SCORE, np.int16)
    if h < 7 or w < 7:
        return out
    c = g[3:h - 3, 3:w - 3]
    d = [g[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] - c for dx, dy in RING]
    s = np.full(c.shape, NO_SCORE, np.int16)
    for a in range(16):
        arc = np.stack([d[(a + k) % 16] for k in range(9)])
        s = np.maximum(s, np.maximum(arc.min(axis=0), -arc.max(axis=0)))
    out[3:h - 3, 3:w - 3] = s
    return out


def candidates(g, fast_threshold):
    """(ys, xs) of the candidates of one level, in raster order."""
    h, w = g.shape
    s = score_map(g).astype(np.int32)
    inner = s[BORDER:h - BORDER, BORDER:w - BORDER]
    ok = inner > fast_threshold
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                ok &= inner > s[BORDER + dy:h - BORDER + dy, BORDER + dx:w - BORDER + dx]
    ys, xs = np.nonzero(ok)
    return ys + BORDER, xs + BORDER


def response(g, ys, xs):
    """int64 R of the pixels (ys, xs), each at least 4 pixels inside the level."""
    p = np.asarray(g, np.uint8).astype(np.int64)
    ix, iy = np.zeros_like(p), np.zeros_like(p)
    ix[:, 1:-1] = p[:, 2:] - p[:, :-2]
    iy[1:-1, :] = p[2:, :] - p[:-2, :]
    ys, xs = np.asarray(ys, np.int64), np.asarray(xs, np.int64)
    a, b, c = (np.zeros(len(ys), np.int64) for _ in range(3))
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            u, v = ix[ys + dy, xs + dx], iy[ys + dy, xs + dx]
            a += u * u
            b += u * v
            c += v * v
    return (25 * (a * c - b * b) - (a + c) * (a + c)) >> 16


def orientation(g, ys, xs):
    p = np.asarray(g, np.uint8).astype(np.int64)
    ys, xs = np.asarray(ys, np.int64), np.asarray(xs, np.int64)
    patch = p[ys[:, None] + DISC_V[None, :], xs[:, None] + DISC_U[None, :]]
    m10, m01 = (patch * DISC_U[None, :]).sum(axis=1), (patch * DISC_V[None, :]).sum(axis=1)
    return np.argmax(m10[:, None] * CX[None, :] + m01[:, None] * CY[None, :], axis=1).astype(np.int32)  # the first maximum: smallest b


def rotated_patterns():
    """(36, 256, 4) int64: px, py, qx, qy of the base pattern turned by 2 pi b / 36, rotated here and not taken from the package."""
    base = np.asarray(pattern()).astype(np.float64)
    out = np.zeros((BINS, base.shape[0], 4), np.int64)
    for b in range(BINS):
        c, s = np.cos(2.0 * np.pi * b / BINS), np.sin(2.0 * np.pi * b / BINS)
        for k in (0, 2):
            out[b, :, k] = np.rint(base[:, k] * c - base[:, k + 1] * s)
            out[b, :, k + 1] = np.rint(base[:, k] * s + base[:, k + 1] * c)
    return out


_ROT = None


def describe(B, ys, xs, bins):
    global _ROT
    if _ROT is None:
        _ROT = rotated_patterns()
    B = np.asarray(B, np.uint8)
    ys, xs = np.asarray(ys, np.int64), np.asarray(xs, np.int64)
    t = _ROT[np.asarray(bins, np.int64)]  # (n, 256, 4)
    bits = B[ys[:, None] + t[:, :, 1], xs[:, None] + t[:, :, 0]] < B[ys[:, None] + t[:, :, 3], xs[:, None] + t[:, :, 2]]
    return np.packbits(bits, axis=1, bitorder="little").reshape(len(ys), 32)


def detect(img, mask=None, nfeatures=500, nlevels=8, scale=1.2, fast_threshold=20, upright=False):
    """-> dict of level, x, y, bin (int32), R (int64), descriptors (n, 32) u8, and level_sizes.  upright=True is the WRONG variant with
    every bin forced to 0, kept for the test that shows orientation earns its place."""
    img = np.asarray(img, np.uint8)
    h0, w0 = img.shape[:2]
    levels = pyramid(grey(img), nlevels, scale)
    quota = quotas(nfeatures, scale, len(levels))
    out = {k: [] for k in ("level", "x", "y", "bin", "R", "descriptors")}
    for l, g in enumerate(levels):
        hl, wl = g.shape
        ys, xs = candidates(g, fast_threshold)
        if mask is not None:
            keep = np.asarray(mask)[((2 * ys + 1) * h0) // (2 * hl), ((2 * xs + 1) * w0) // (2 * wl)] != 0
            ys, xs = ys[keep], xs[keep]
        R = response(g, ys, xs)
        order = np.lexsort((xs, ys, -R))[:quota[l]]
        ys, xs, R = ys[order], xs[order], R[order]
        bins = np.zeros(len(ys), np.int32) if upright else orientation(g, ys, xs)
        out["level"].append(np.full(len(ys), l, np.int32))
        out["x"].append(xs.astype(np.int32))
        out["y"].append(ys.astype(np.int32))
        out["bin"].append(bins)
        out["R"].append(R.astype(np.int64))
        out["descriptors"].append(describe(blur(g), ys, xs, bins))
    res = {k: (np.concatenate(v) if v else np.zeros((0, 32) if k == "descriptors" else 0, np.uint8 if k == "descriptors" else
                                                     (np.int64 if k == "R" else np.int32))) for k, v in out.items()}
    res["level_sizes"] = [(g.shape[1], g.shape[0]) for g in levels]
    return res
