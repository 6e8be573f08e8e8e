"""Restatement of the "voronoi" and "no" seam finders (SeamFinder::find, OpenCV 4.x modules/stitching/src/seam_finders.cpp:
PairwiseSeamFinder::run, VoronoiSeamFinder::findInPair, NoSeamFinder) in numpy: the contract `stitching_amd.SeamEstimator` is tested
against.

Written from recollection of OpenCV (no OpenCV source or build is at hand): fidelity to real OpenCV is unpinned, as for the rest of the
oracle.

Pairs (i, j), i < j, run in index order; each sees the masks as the earlier pairs left them.  For a pair whose rectangles overlap in
`roi`, the masks are cut with a gap of 10 pixels around it (0 outside an image), the pixels both masks hold are taken out, and the L1
distance to the nearest remaining pixel of each mask is compared: where image i's is strictly smaller, mask j is zeroed, elsewhere
mask i.  Only pixels of `roi` are written.  Kept values keep their value (254 stays 254).
"""

import numpy as np

GAP = 10
DIST_SAT = 8192  # distanceTransform(DIST_L1, 3)'s fixed point saturates at 8192.0f (csrc/stx_blend.hip, distance transform)
KINDS = ("voronoi", "no")


def overlap_roi(c1, s1, c2, s2):
    """PairwiseSeamFinder's overlapRoi: corners (x, y), sizes (w, h) -> the intersection (x, y, w, h) in panorama coordinates or None."""
    x0, y0 = max(c1[0], c2[0]), max(c1[1], c2[1])
    x1, y1 = min(c1[0] + s1[0], c2[0] + s2[0]), min(c1[1] + s1[1], c2[1] + s2[1])
    if x0 < x1 and y0 < y1:
        return (x0, y0, x1 - x0, y1 - y0)
    return None


def pairs(corners, sizes):
    """run()'s pairs in order: [(i, j, roi)]."""
    out = []
    n = len(sizes)
    for i in range(n - 1):
        for j in range(i + 1, n):
            roi = overlap_roi(corners[i], sizes[i], corners[j], sizes[j])
            if roi is not None:
                out.append((i, j, roi))
    return out


def l1_distance(src):
    """distanceTransform(src == 0, DIST_L1, 3) of a 2-D bool array `src` (True: a source pixel): min(city-block distance to the nearest
    source, 8192) as int32; 8192 everywhere when there is no source.

    Row sweeps, then column sweeps over the row distances g:
      left   l(x) = x - (last source column <= x)     right  r(x) = (first source column >= x) - x      g = min(l, r)
      down   a(y) = min(g(y), a(y - 1) + 1)          up     f(y) = min(a(y), f(y + 1) + 1)
    The recurrences are written in their closed forms (running max / min along the axis).  Clamping g before the column sweeps
    gives the same result as clamping at the end: both sweeps only add non-negative amounts and take minima."""
    src = np.asarray(src, bool)
    h, w = src.shape
    big = 1 << 28
    xs = np.arange(w, dtype=np.int64)[None, :]
    last = np.maximum.accumulate(np.where(src, xs, -big), axis=1)
    first = np.minimum.accumulate(np.where(src, xs, 2 * big)[:, ::-1], axis=1)[:, ::-1]
    g = np.minimum(np.minimum(xs - last, first - xs), DIST_SAT)
    ys = np.arange(h, dtype=np.int64)[:, None]
    a = ys + np.minimum.accumulate(g - ys, axis=0)
    f = -ys + np.minimum.accumulate((a + ys)[::-1], axis=0)[::-1]
    return np.minimum(f, DIST_SAT).astype(np.int32)


def cut(mask, corner, x0, y0, w, h):
    """The h x w window at panorama (x0, y0) of `mask` placed at `corner`; pixels outside the image read as 0."""
    out = np.zeros((h, w), np.uint8)
    mh, mw = mask.shape
    ox, oy = x0 - corner[0], y0 - corner[1]
    sx0, sy0, sx1, sy1 = max(ox, 0), max(oy, 0), min(ox + w, mw), min(oy + h, mh)
    if sx0 < sx1 and sy0 < sy1:
        out[sy0 - oy:sy1 - oy, sx0 - ox:sx1 - ox] = mask[sy0:sy1, sx0:sx1]
    return out


def seam_in_pair(m1, c1, m2, c2, roi):
    """VoronoiSeamFinder::findInPair's decision over `roi`: a bool (h, w) array, True where mask j is zeroed (dist1 < dist2), False
    where mask i is."""
    x, y, w, h = roi
    s1 = cut(m1, c1, x - GAP, y - GAP, w + 2 * GAP, h + 2 * GAP)
    s2 = cut(m2, c2, x - GAP, y - GAP, w + 2 * GAP, h + 2 * GAP)
    collision = (s1 != 0) & (s2 != 0)
    unique1 = (s1 != 0) & ~collision
    unique2 = (s2 != 0) & ~collision
    d1, d2 = l1_distance(unique1), l1_distance(unique2)
    return (d1 < d2)[GAP:GAP + h, GAP:GAP + w]


def find_in_pair(masks, corners, i, j, roi):
    """One pair, in place on `masks` (a list of 2-D u8 arrays)."""
    x, y, w, h = roi
    seam = seam_in_pair(masks[i], corners[i], masks[j], corners[j], roi)
    (xi, yi), (xj, yj) = corners[i], corners[j]
    ri = masks[i][y - yi:y - yi + h, x - xi:x - xi + w]
    rj = masks[j][y - yj:y - yj + h, x - xj:x - xj + w]
    rj[seam] = 0
    ri[~seam] = 0


def find(kind, corners, masks, sizes=None):
    """SeamFinder::find on copies of `masks` (2-D u8 arrays); sizes (w, h) default to the masks' (OpenCV takes them from the images).
    -> new list of masks."""
    if kind not in KINDS:
        raise ValueError(kind)
    out = [np.array(m, np.uint8, copy=True) for m in masks]
    corners = [tuple(int(v) for v in c) for c in corners]
    if kind == "no" or len(out) == 0:
        return out
    sizes = [(m.shape[1], m.shape[0]) for m in out] if sizes is None else [tuple(s) for s in sizes]
    for i, j, roi in pairs(corners, sizes):
        find_in_pair(out, corners, i, j, roi)
    return out
