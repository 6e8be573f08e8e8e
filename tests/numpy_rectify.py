"""The contract of lens rectification (stx_rectify, stitching_amd.rectify): plain numpy.  The device equals `rectify` byte for byte
(tests/test_gpu_rectify.py), and `stitching_amd.LensMap` makes the nodes that `brown_nodes`, `fisheye_nodes` and `maps_nodes` make.

Two halves.

The lens grid (host, float64, once per rig).  For a destination image W x H the map is held at nodes every CELL = 16 destination
pixels: nx = (W + 15) // 16 + 1, ny = (H + 15) // 16 + 1, node (i, j) at destination pixel (16 i, 16 j), the nodes past the right and
bottom edge included.  A node holds the source coordinate (sx, sy) of its pixel in Q6 as int32: rint(s * 64), clipped to
[-16384 * 64, 32767 * 64]; a coordinate that is not finite is refused.  The coordinates come from the Brown model (OpenCV's order
k1, k2, p1, p2[, k3[, k4, k5, k6]]; no tilt, no thin prism), the Kannala-Brandt fisheye model (four coefficients over theta =
atan(r)), or a full-resolution float map (sampled at the nodes; past the last column or row it is extrapolated linearly from the last
two, a single column or row is repeated).

Per pixel (device, integer only).  For destination pixel (x, y), ax = x & 15, ay = y & 15 and the nodes N00 N10 / N01 N11 of its cell,
per coordinate, in int32:

    S = (16 - ay) * ((16 - ax) * N00 + ax * N10) + ay * ((16 - ax) * N01 + ax * N11)      Q14, |S| < 2^30
    q = (S + 256) >> 9                                                                  arithmetic shift: Q5, floor
    i = q >> 5,  f = q & 31

The taps are (ix, iy), (ix + 1, iy), (ix, iy + 1), (ix + 1, iy + 1); with border "constant" a tap outside the source reads 0, with
"replicate" its indices are clamped.  Per channel

    out = (w00 p00 + w10 p10 + w01 p01 + w11 p11 + 512) >> 10,   w00 = (32 - fx)(32 - fy), w10 = fx (32 - fy), w01 = (32 - fx) fy, w11 = fx fy

and the mask is 255 where all four taps lie inside the source, 0 elsewhere.

How far q / 32 is from B, the float64 bilinear interpolation of the UNROUNDED node coordinates (`quantisation_bound`): a node is
within 1/2 of a Q6 unit, 1/128 px, of its coordinate, and a convex combination of nodes no further; S / 2^14 is that combination
exactly; q = floor(S / 2^9 + 1/2) is within 1/2 of a Q5 unit, 1/64 px, of it.  Together 1/128 + 1/64 = 3/128 px.
"""
import numpy as np

CELL = 16
Q6_MIN, Q6_MAX = -16384 * 64, 32767 * 64
BORDERS = ("constant", "replicate")


def node_counts(w, h):
    return (w + CELL - 1) // CELL + 1, (h + CELL - 1) // CELL + 1


def node_pixels(w, h):
    """destination coordinates (x, y) of the nodes as float64 arrays [ny, nx]"""
    nx, ny = node_counts(w, h)
    return np.meshgrid(np.arange(nx, dtype=np.float64) * CELL, np.arange(ny, dtype=np.float64) * CELL)


def quantise(sx, sy):
    """float64 source coordinates [ny, nx] -> int32 nodes [ny, nx, 2] in Q6"""
    s = np.stack([np.asarray(sx, np.float64), np.asarray(sy, np.float64)], axis=-1)
    if not np.all(np.isfinite(s)):
        raise ValueError("a source coordinate is not finite")
    return np.clip(np.rint(s * 64.0), Q6_MIN, Q6_MAX).astype(np.int32)


def _k4(K):
    K = np.asarray(K, np.float64)
    return K[0, 0], K[1, 1], K[0, 2], K[1, 2]


def brown_source(K, dist, new_K, u, v):
    """The exact Brown model: destination pixel (u, v) of the pinhole camera new_K -> source coordinate (float64)."""
    d = np.zeros(8)
    dist = np.asarray(dist, np.float64).ravel()
    d[:dist.size] = dist
    k1, k2, p1, p2, k3, k4, k5, k6 = d
    fx, fy, cx, cy = _k4(K)
    nfx, nfy, ncx, ncy = _k4(new_K)
    x, y = (np.asarray(u, np.float64) - ncx) / nfx, (np.asarray(v, np.float64) - ncy) / nfy
    r2 = x * x + y * y
    kr = (1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))) / (1.0 + r2 * (k4 + r2 * (k5 + r2 * k6)))
    xd = x * kr + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
    yd = y * kr + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
    return fx * xd + cx, fy * yd + cy


def fisheye_source(K, D, new_K, u, v):
    """The exact Kannala-Brandt model: theta_d = theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8), theta = atan(r)."""
    k1, k2, k3, k4 = np.asarray(D, np.float64).ravel()
    fx, fy, cx, cy = _k4(K)
    nfx, nfy, ncx, ncy = _k4(new_K)
    x, y = (np.asarray(u, np.float64) - ncx) / nfx, (np.asarray(v, np.float64) - ncy) / nfy
    r = np.sqrt(x * x + y * y)
    th = np.arctan(r)
    t2 = th * th
    thd = th * (1.0 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4))))
    scale = np.where(r > 1e-12, thd / np.maximum(r, 1e-12), 1.0)
    return fx * x * scale + cx, fy * y * scale + cy


def brown_nodes(K, dist, new_K, dst_size):
    w, h = dst_size
    return quantise(*brown_source(K, dist, new_K, *node_pixels(w, h)))


def fisheye_nodes(K, D, new_K, dst_size):
    w, h = dst_size
    return quantise(*fisheye_source(K, D, new_K, *node_pixels(w, h)))


def _sample_extrapolated(m, cx, cy):
    """m [H, W] at integer coordinates cy [ny], cx [nx], linearly extrapolated past the last row / column (a single one is repeated)"""
    m = np.asarray(m, np.float64)

    def along(a, c, axis):
        n = a.shape[axis]
        inside = np.take(a, np.minimum(c, n - 1), axis=axis)
        if n == 1:
            return inside
        last, step = np.take(a, [n - 1], axis=axis), np.take(a, [n - 1], axis=axis) - np.take(a, [n - 2], axis=axis)
        shape = [1, 1]
        shape[axis] = c.size
        over = np.maximum(c - (n - 1), 0).astype(np.float64).reshape(shape)
        return np.where(over > 0, last + over * step, inside)

    return along(along(m, cx, 1), cy, 0)


def maps_nodes(map_x, map_y):
    """full-resolution float maps [H, W] (as cv2.initUndistortRectifyMap returns them) -> nodes"""
    h, w = np.asarray(map_x).shape
    nx, ny = node_counts(w, h)
    cx, cy = np.arange(nx) * CELL, np.arange(ny) * CELL
    return quantise(_sample_extrapolated(map_x, cx, cy), _sample_extrapolated(map_y, cx, cy))


def interpolate(nodes, dst_size):
    """(e): nodes [ny, nx, 2] -> the Q5 coordinates q [H, W, 2] (int32) of every destination pixel"""
    w, h = dst_size
    nodes = np.asarray(nodes)
    if nodes.dtype != np.int32 or nodes.shape != node_counts(w, h)[::-1] + (2,):
        raise ValueError(f"nodes of a {w} x {h} destination are int32 of shape {node_counts(w, h)[::-1] + (2,)}")
    y, x = np.arange(h, dtype=np.int32)[:, None], np.arange(w, dtype=np.int32)[None, :]
    ax, ay, i, j = (x & 15)[..., None], (y & 15)[..., None], x >> 4, y >> 4
    n00, n10, n01, n11 = nodes[j, i], nodes[j, i + 1], nodes[j + 1, i], nodes[j + 1, i + 1]
    s = (16 - ay) * ((16 - ax) * n00 + ax * n10) + ay * ((16 - ax) * n01 + ax * n11)
    assert s.dtype == np.int32
    return (s + 256) >> 9


def rectify(src, nodes, dst_size, border="constant"):
    """(e) - (h): u8 source [sh, sw] or [sh, sw, 3] -> (image [H, W(, 3)] u8, mask [H, W] u8)"""
    if border not in BORDERS:
        raise ValueError(f"unknown border {border!r}")
    src = np.asarray(src)
    if src.dtype != np.uint8 or src.ndim not in (2, 3) or (src.ndim == 3 and src.shape[2] != 3):
        raise ValueError("the source is u8 with 1 or 3 channels")
    sh, sw = src.shape[:2]
    q = interpolate(nodes, dst_size)
    ix, iy, fx, fy = q[..., 0] >> 5, q[..., 1] >> 5, q[..., 0] & 31, q[..., 1] & 31
    acc = np.full(q.shape[:2] + src.shape[2:], 512, np.int32)
    valid = np.ones(q.shape[:2], bool)
    for dx, dy, wgt in ((0, 0, (32 - fx) * (32 - fy)), (1, 0, fx * (32 - fy)), (0, 1, (32 - fx) * fy), (1, 1, fx * fy)):
        tx, ty = ix + dx, iy + dy
        inside = (tx >= 0) & (tx < sw) & (ty >= 0) & (ty < sh)
        p = src[np.clip(ty, 0, sh - 1), np.clip(tx, 0, sw - 1)].astype(np.int32)
        if border == "constant":
            p = np.where(inside if src.ndim == 2 else inside[..., None], p, 0)
        acc += (wgt if src.ndim == 2 else wgt[..., None]) * p
        valid &= inside
    return (acc >> 10).astype(np.uint8), np.where(valid, 255, 0).astype(np.uint8)


def float_bilinear(sx, sy, dst_size):
    """B of the docstring: the float64 bilinear interpolation of unrounded node coordinates sx, sy [ny, nx] -> [H, W, 2]"""
    w, h = dst_size
    y, x = np.arange(h)[:, None], np.arange(w)[None, :]
    tx, ty, i, j = (x & 15) / 16.0, (y & 15) / 16.0, x >> 4, y >> 4
    out = []
    for s in (np.asarray(sx, np.float64), np.asarray(sy, np.float64)):
        out.append((1 - ty) * ((1 - tx) * s[j, i] + tx * s[j, i + 1]) + ty * ((1 - tx) * s[j + 1, i] + tx * s[j + 1, i + 1]))
    return np.stack(out, axis=-1)


QUANTISATION_BOUND = 1.0 / 128.0 + 1.0 / 64.0
