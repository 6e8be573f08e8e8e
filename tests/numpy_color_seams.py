"""The colour-aware seam finder of this project in numpy: the contract `stitching_amd.ColorSeamEstimator` is tested against, byte for byte.

This is the project's OWN finder.  It is NOT OpenCV's DpSeamFinder ("dp_color" / "dp_colorgrad": flood fills, contour walking and a
component-by-component dynamic programme) and does not claim those names: it is pairwise, integer only, one dynamic programme per
overlapping pair.  Pair order and "each pair sees the masks as the earlier pairs left them" are PairwiseSeamFinder::run's, as for
"voronoi" (tests/numpy_seams.py: overlap_roi, pairs).

One pair (i, j), i < j, with overlap roi = (x, y, w, h), u8 BGR images I_k (read, never written) and u8 masks m_k:
  collision   both(p) = m_i(p) != 0 and m_j(p) != 0 for p in roi.  Only pixels of `both` are ever written.
  cost        c(p) = sum over the channels of (I_i(p) - I_j(p))^2 where both(p), 0 elsewhere: an int32 of at most 3 * 255^2 = 195 075.
  orientation the doubled centres 2 * corner + size of the two images: |dx| >= |dy| -> a VERTICAL seam (one cut column per roi row: the
              seam axis is y, the cross axis x), else a HORIZONTAL one (the same rule on the transposed roi).  The FIRST image is the one
              with the smaller doubled centre on the cross axis (a tie: i), the other the SECOND.
  dp          r along the seam axis (0 <= r < L), t along the cross axis (0 <= t < W):  A(0, t) = c(0, t),
              A(r, t) = c(r, t) + min(A(r-1, t), A(r-1, t-1), A(r-1, t+1)), neighbours out of range left out; on equal values the first
              in that order wins (straight, then t-1, then t+1).  u32 accumulators.
  seam        the end point is the smallest t that minimises A(L-1, t); the recorded choices walked back give s(r) for every r.
  apply       a `both` pixel at (r, t): t < s(r) -> the first image keeps it, the second's mask is zeroed there; t >= s(r) -> the second
              keeps it, the first's mask is zeroed.  Kept values keep their value (254 stays 254); pixels outside `both` are untouched.

Consequences (tests/test_color_seams.py):
  * every pixel keeps at least one owner it had before: the union of the masks on the panorama is unchanged by find();
  * after all pairs no panorama pixel inside any pair's roi is held by both images of that pair (a later pair only zeroes).

Limit: L <= MAX_SEAM_LENGTH = 16 384, so that the u32 accumulators cannot overflow (16 384 * 195 075 < 2^32).  The device also caps W
(ColorSeamEstimator.MAX_CROSS_EXTENT: its accumulator rows live in LDS); this file does not.
"""

import numpy as np

from tests.numpy_seams import overlap_roi, pairs  # noqa: F401  (re-exported: the pair list is the voronoi finder's)

MAX_COST = 3 * 255 * 255
MAX_SEAM_LENGTH = 16384
assert MAX_SEAM_LENGTH * MAX_COST < 2 ** 32


def orientation(ci, si, cj, sj):
    """-> (vertical, first_is_i) from corners (x, y) and sizes (w, h) of images i and j."""
    dx = (2 * ci[0] + si[0]) - (2 * cj[0] + sj[0])
    dy = (2 * ci[1] + si[1]) - (2 * cj[1] + sj[1])
    vertical = abs(dx) >= abs(dy)
    return vertical, (dx if vertical else dy) <= 0


def pair_cost(img_i, ci, mask_i, img_j, cj, mask_j, roi):
    """-> (both (h, w) bool, c (h, w) int32) over the roi."""
    x, y, w, h = roi
    win = lambda a, c: a[y - c[1]:y - c[1] + h, x - c[0]:x - c[0] + w]  # noqa: E731
    both = (win(mask_i, ci) != 0) & (win(mask_j, cj) != 0)
    d = win(img_i, ci).astype(np.int32) - win(img_j, cj).astype(np.int32)
    return both, np.where(both, (d * d).sum(axis=2), 0).astype(np.int32)


def dp_seam(c):
    """c: (L, W) costs, r along axis 0.  -> s (L,) int32, the cut position per r."""
    c = np.asarray(c, np.int64)
    L, W = c.shape
    if L > MAX_SEAM_LENGTH:
        raise ValueError(f"seam length {L} > {MAX_SEAM_LENGTH}")
    big = np.int64(1) << 40
    step = np.zeros((L, W), np.int8)  # t of the chosen neighbour in row r-1, minus t
    A = c[0].copy()
    for r in range(1, L):
        best = A.copy()
        left = np.concatenate(([big], A[:-1]))
        right = np.concatenate((A[1:], [big]))
        m = left < best
        best[m], step[r][m] = left[m], -1
        m = right < best
        best[m], step[r][m] = right[m], 1
        A = c[r] + best
    assert A.max() < 2 ** 32
    t = int(np.argmin(A))  # the first of the minima
    s = np.zeros(L, np.int32)
    s[L - 1] = t
    for r in range(L - 1, 0, -1):
        t += int(step[r][t])
        s[r - 1] = t
    return s


def seam_in_pair(imgs, masks, corners, i, j, roi):
    """-> (both, second_keeps (h, w) bool: True where t >= s(r), vertical, first_is_i, s)"""
    sz = lambda k: (masks[k].shape[1], masks[k].shape[0])  # noqa: E731
    both, c = pair_cost(imgs[i], corners[i], masks[i], imgs[j], corners[j], masks[j], roi)
    vertical, first_is_i = orientation(corners[i], sz(i), corners[j], sz(j))
    s = dp_seam(c if vertical else c.T)
    L, W = (c.shape if vertical else c.T.shape)
    second = np.arange(W)[None, :] >= s[:, None]
    return both, (second if vertical else second.T), vertical, first_is_i, s


def find_in_pair(imgs, masks, corners, i, j, roi):
    """One pair, in place on `masks`."""
    x, y, w, h = roi
    both, second_keeps, _, first_is_i, _ = seam_in_pair(imgs, masks, corners, i, j, roi)
    first, second = (i, j) if first_is_i else (j, i)
    win = lambda k: masks[k][y - corners[k][1]:y - corners[k][1] + h, x - corners[k][0]:x - corners[k][0] + w]  # noqa: E731
    win(first)[both & second_keeps] = 0
    win(second)[both & ~second_keeps] = 0


def find(imgs, corners, masks):
    """All pairs in run()'s order on copies of `masks` (2-D u8 arrays); imgs: u8 (h, w, 3) arrays of the masks' sizes.  -> new masks."""
    out = [np.array(m, np.uint8, copy=True) for m in masks]
    imgs = [np.asarray(a) for a in imgs]
    corners = [tuple(int(v) for v in c) for c in corners]
    for k, (a, m) in enumerate(zip(imgs, out)):
        if a.dtype != np.uint8 or a.shape != m.shape + (3,):
            raise ValueError(f"image {k}: expected u8 {m.shape + (3,)}, got {a.dtype} {a.shape}")
    sizes = [(m.shape[1], m.shape[0]) for m in out]
    for i, j, roi in pairs(corners, sizes):
        find_in_pair(imgs, out, corners, i, j, roi)
    return out
