"""The contract of the warp through the lens (stx_warp_lens_batch, Warper.warp_images_through_lenses): plain numpy.  A DISTORTED frame
goes to the panorama in one resampling: the warp's own fp32 backward map into the rectified (pinhole) frame, then the camera's lens grid
(tests/numpy_rectify.py: the nodes of a `LensMap`), then four taps of the distorted frame.  The device equals `lens_warp` byte for byte
(tests/test_gpu_lens_warp.py).

Inputs: src u8 [sh, sw, 3], the distorted frame; nodes int32 [ny, nx, 2] in Q6 for a rectified size (W, H), one every 16 rectified pixels
(numpy_rectify.node_counts); xmap, ymap fp32 [dh, dw], the backward map into the rectified frame (numpy_warper.map_backward).

Per destination pixel, integer only after (a):

 (a) sx = cvRound(32 x), sy = cvRound(32 y), as cv::remap forms its 1/32-px positions (round half to even; NaN, infinities and anything
     outside int32 give INT_MIN).
 (b) qx = clip(sx, 0, 32 (W - 1)), qy = clip(sy, 0, 32 (H - 1)): a replicate border in the pinhole domain.
 (c) cell i = qx >> 9, j = qy >> 9 (16 pixels of 32 units); position in the cell ax = qx & 511, ay = qy & 511.  The nodes N[j .. j + 1]
     [i .. i + 1] always exist: i <= (W - 1) / 16 and nx = (W + 15) / 16 + 1.
 (d) per coordinate, in int32 (|N| <= 2^21, so every product sum below is at most 512 * 2^21 = 2^30 in magnitude):
         L0 = ((512 - ax) N00 + ax N10 + 256) >> 9         Q6, along the upper edge of the cell
         L1 = ((512 - ax) N01 + ax N11 + 256) >> 9         Q6, along the lower edge
         q  = ((512 - ay) L0 + ay L1 + 512) >> 10          Q5; arithmetic shifts: floor
 (e) ix = q >> 5, f = q & 31 per axis; the four taps (ix, iy), (ix + 1, iy), (ix, iy + 1), (ix + 1, iy + 1) are read at indices CLAMPED
     into the source, always: a constant border would put the lens's black wedges into the pyramids.
 (f) per channel out = (w00 p00 + w10 p10 + w01 p01 + w11 p11 + 512) >> 10, w00 = (32 - fx)(32 - fy), w10 = fx (32 - fy),
     w01 = (32 - fx) fy, w11 = fx fy: the rectify kernel's blend.

Accuracy (`QUANTISATION_BOUND`): |q / 32 - B| <= 1/32 px, B the float64 bilinear interpolation of the UNROUNDED node coordinates at the
point (qx / 32, qy / 32).  A node is within 1/2 Q6 unit = 1/128 px of its coordinate, and so is any convex combination of nodes; L is
floor(exact + 1/2) in Q6, another 1/128 px, and the combination of L0 and L1 carries no more than that; q is floor(exact / 2 + 1/2) in Q5,
within 1/2 Q5 unit = 1/64 px.  1/128 + 1/128 + 1/64 = 1/32.

With identity nodes (N = 64 * pixel) L = 2 (32 * 16 i + ax) exactly and q is the clipped position itself, so the result is remap's
wherever remap's own taps are the clamped ones: cv::remap's Q15 weights at 5 fractional bits are 32 a b exactly, and
(sum 32 a b p + 16384) >> 15 == (sum a b p + 512) >> 10.  tests/test_lens_warp_contract.py states how far that reaches.
"""
import numpy as np

from . import numpy_rectify as nr
from . import numpy_warper as nw

QUANTISATION_BOUND = 1.0 / 32.0
INT_MIN = -2 ** 31


def positions(xmap, ymap, dst_size):
    """(a), (b): the clipped 1/32-px positions (qx, qy) in the rectified frame, int32 [dh, dw]"""
    w, h = dst_size
    with np.errstate(over="ignore", invalid="ignore"):
        sx, sy = nw._cv_round(np.asarray(xmap, np.float32) * nw.F(32)), nw._cv_round(np.asarray(ymap, np.float32) * nw.F(32))
    return np.clip(sx, 0, 32 * (w - 1)).astype(np.int32), np.clip(sy, 0, 32 * (h - 1)).astype(np.int32)


def through_lens(nodes, qx, qy, dst_size, stages=None):
    """(c), (d): positions in the rectified frame -> the Q5 coordinates q [dh, dw, 2] (int32) in the distorted frame.  `stages`, a list,
    receives every intermediate (for the test of their width)."""
    w, h = dst_size
    nodes = np.asarray(nodes)
    if nodes.dtype != np.int32 or nodes.shape != nr.node_counts(w, h)[::-1] + (2,):
        raise ValueError(f"nodes of a {w} x {h} rectified frame are int32 of shape {nr.node_counts(w, h)[::-1] + (2,)}")
    qx, qy = np.asarray(qx), np.asarray(qy)
    assert qx.dtype == np.int32 and qy.dtype == np.int32
    i, j, ax, ay = qx >> 9, qy >> 9, (qx & 511)[..., None], (qy & 511)[..., None]
    n00, n10, n01, n11 = nodes[j, i], nodes[j, i + 1], nodes[j + 1, i], nodes[j + 1, i + 1]
    s0 = (512 - ax) * n00 + ax * n10 + 256
    s1 = (512 - ax) * n01 + ax * n11 + 256
    l0, l1 = s0 >> 9, s1 >> 9
    s = (512 - ay) * l0 + ay * l1 + 512
    q = s >> 10
    for a in (s0, s1, l0, l1, s, q):
        assert a.dtype == np.int32
    if stages is not None:
        stages.extend([s0, s1, l0, l1, s, q])
    return q


def sample_clamped(src, q):
    """(e), (f): Q5 coordinates [.., 2] -> u8 [.., 3] from taps at clamped indices"""
    src = np.asarray(src)
    if src.dtype != np.uint8 or src.ndim != 3 or src.shape[2] != 3:
        raise ValueError("the source is u8 with 3 channels")
    sh, sw = src.shape[:2]
    ix, iy, fx, fy = q[..., 0] >> 5, q[..., 1] >> 5, q[..., 0] & 31, q[..., 1] & 31
    acc = np.full(q.shape[:-1] + (3,), 512, np.int32)
    for dx, dy, wgt in ((0, 0, (32 - fx) * (32 - fy)), (1, 0, fx * (32 - fy)), (0, 1, (32 - fx) * fy), (1, 1, fx * fy)):
        p = src[np.clip(iy + dy, 0, sh - 1), np.clip(ix + dx, 0, sw - 1)].astype(np.int32)
        acc += wgt[..., None] * p
    assert acc.dtype == np.int32
    return (acc >> 10).astype(np.uint8)


def lens_warp(src, nodes, dst_size, xmap, ymap):
    """The whole contract: -> u8 [dh, dw, 3]"""
    qx, qy = positions(xmap, ymap, dst_size)
    return sample_clamped(src, through_lens(nodes, qx, qy, dst_size))


def float_bilinear_at(sx, sy, qx, qy):
    """B of the docstring: the float64 bilinear interpolation of unrounded node coordinates sx, sy [ny, nx] at (qx / 32, qy / 32)"""
    i, j, tx, ty = qx >> 9, qy >> 9, (qx & 511) / 512.0, (qy & 511) / 512.0
    out = []
    for s in (np.asarray(sx, np.float64), np.asarray(sy, np.float64)):
        out.append((1 - ty) * ((1 - tx) * s[j, i] + tx * s[j, i + 1]) + ty * ((1 - tx) * s[j + 1, i] + tx * s[j + 1, i + 1]))
    return np.stack(out, axis=-1)
