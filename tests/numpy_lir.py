"""Restatement of the reference's Cropper arithmetic (stitching/cropper.py) without OpenCV or largestinteriorrectangle: the contract
of stitching_amd.cropper and csrc/stx_crop.hip.

single_contour(mask): findContours' check `hierarchy.shape == (1, 1, 4) and all == -1` (cropper.py:96-100) as counts.  OpenCV 4.x
  frames the image with zeros, takes nonzero pixels as 8-connected foreground and zeros as 4-connected background; the hierarchy is one
  entry exactly when the foreground is one component and the framed background one component (no holes).  -> (components, holes).
lir(mask): the largest axis-aligned rectangle of `mask > 0` as (x, y, w, h); ties: smallest y, then smallest x, then largest w; an
  all-false mask gives (0, 0, 0, 0).  The row-by-row DP (height / left / right per column), fast enough for full-resolution masks.
lir_spans(mask): the same rule as largestinteriorrectangle's lir_basis computes it (adjacencies, per-cell span staircases, first
  maxima): slow, for small masks; it pins the tie rule.  The reference calls the contour variant lir(grid, contour), which returns the
  same area; which of several equal-area rectangles it picks is unpinned.
crop_plan(corners, sizes, lir, aspect): Cropper.prepare's rectangle arithmetic and what crop_img / crop_rois make of it.
"""
import numpy as np
from scipy import ndimage


def single_contour(mask):
    """-> (8-connected components of the nonzero pixels, 4-connected components of the zeros of the zero-framed mask that do not
    reach the frame)."""
    m = np.asarray(mask) != 0
    _, fg = ndimage.label(m, structure=np.ones((3, 3), bool))
    framed = np.pad(~m, 1, constant_values=True)
    _, bg = ndimage.label(framed)  # the default structure is the 4-neighbourhood
    return int(fg), int(bg) - 1


def _better(a, b):
    """a = (area, y, x, w) beats b by the tie rule"""
    if a[0] != b[0]:
        return a[0] > b[0]
    if a[1] != b[1]:
        return a[1] < b[1]
    if a[2] != b[2]:
        return a[2] < b[2]
    return a[3] > b[3]


def lir(mask):
    g = np.asarray(mask) > 0
    H, W = g.shape
    height = np.zeros(W, np.int64)
    left = np.zeros(W, np.int64)
    right = np.full(W, W, np.int64)
    xs = np.arange(W, dtype=np.int64)
    best = (0, 0, 0, 0, 0)  # area, y, x, w, h
    for y in range(H):
        r = g[y]
        height = np.where(r, height + 1, 0)
        run_left = np.maximum.accumulate(np.where(r, 0, xs + 1))  # one past the last false cell at or before x
        run_right = np.minimum.accumulate(np.where(r, W, xs)[::-1])[::-1]  # the first false cell at or after x
        left = np.where(r, np.maximum(left, run_left), 0)
        right = np.where(r, np.minimum(right, run_right), W)
        area = height * (right - left)
        top = area.max() if W else 0
        if top == 0 or top < best[0]:
            continue
        # candidates of this row: rectangles with bottom row y, height height[x], over [left[x], right[x])
        idx = np.flatnonzero(area == top)
        ys, x0s, ws = y - height[idx] + 1, left[idx], right[idx] - left[idx]
        order = np.lexsort((-ws, x0s, ys))
        k = idx[order[0]]
        cand = (int(top), int(y - height[k] + 1), int(left[k]), int(right[k] - left[k]), int(height[k]))
        if _better(cand[:4], best[:4]):
            best = cand
    if best[0] == 0:
        return (0, 0, 0, 0)
    return (best[2], best[1], best[3], best[4])


def lir_spans(mask):
    """largestinteriorrectangle's lir_basis, step by step."""
    g = np.asarray(mask) > 0
    H, W = g.shape
    h_adj = np.zeros((H, W), np.int64)  # run of true cells to the right
    v_adj = np.zeros((H, W), np.int64)  # run of true cells downward
    for y in range(H):
        span = 0
        for x in range(W - 1, -1, -1):
            span = span + 1 if g[y, x] else 0
            h_adj[y, x] = span
    for x in range(W):
        span = 0
        for y in range(H - 1, -1, -1):
            span = span + 1 if g[y, x] else 0
            v_adj[y, x] = span
    span_map = np.zeros((H, W, 2), np.int64)
    for y, x in zip(*g.nonzero()):
        col = h_adj[y:, x]
        n = int(np.flatnonzero(col == 0)[0]) if np.any(col == 0) else len(col)
        h_vec = np.unique(np.minimum.accumulate(col[:n]))[::-1]  # widths, widest first
        row = v_adj[y, x:]
        n = int(np.flatnonzero(row == 0)[0]) if np.any(row == 0) else len(row)
        v_vec = np.unique(np.minimum.accumulate(row[:n]))[::-1]  # heights, tallest first
        spans = np.stack((h_vec, v_vec[::-1]), axis=1)  # (width, height): widest with shortest
        areas = spans[:, 0] * spans[:, 1]
        span_map[y, x] = spans[np.flatnonzero(areas == areas.max())[0]]
    areas = span_map[:, :, 0] * span_map[:, :, 1]
    if areas.max() == 0:
        return (0, 0, 0, 0)
    ys, xs = np.nonzero(areas == areas.max())
    y, x = int(ys[0]), int(xs[0])
    return (x, y, int(span_map[y, x, 0]), int(span_map[y, x, 1]))


def brute_force(mask):
    """every rectangle, the tie rule by enumeration (small masks)."""
    g = np.asarray(mask) > 0
    H, W = g.shape
    best = (0, 0, 0, 0)
    rect = (0, 0, 0, 0)
    for y0 in range(H):
        ok = np.ones(W, bool)
        for y1 in range(y0, H):
            ok &= g[y1]
            c = np.concatenate([[0], np.cumsum(ok)])
            x0, x1 = np.meshgrid(np.arange(W), np.arange(W), indexing="ij")
            full = (x1 >= x0) & (c[x1 + 1] - c[x0] == x1 - x0 + 1)
            if not full.any():
                continue
            h = y1 - y0 + 1
            for a, b in zip(*np.nonzero(full)):
                cand = (int((b - a + 1) * h), y0, int(a), int(b - a + 1))
                if _better(cand, best):
                    best, rect = cand, (int(a), y0, int(b - a + 1), h)
    return rect


# ---- the reference's rectangle arithmetic (cropper.py:107-151, Rectangle.times)

def times(r, aspect):
    return tuple(int(round(i * aspect)) for i in r)


def zero_center_corners(corners):
    mx = min(c[0] for c in corners)
    my = min(c[1] for c in corners)
    return [(x - mx, y - my) for x, y in corners]


def overlap(r1, r2):
    x1, y1 = max(r1[0], r2[0]), max(r1[1], r2[1])
    x2, y2 = min(r1[0] + r1[2], r2[0] + r2[2]), min(r1[1] + r1[3], r2[1] + r2[3])
    if x2 < x1 or y2 < y1:
        raise ValueError("Rectangles do not overlap!")
    return (x1, y1, x2 - x1, y2 - y1)


def intersection(r, o):
    return (abs(o[0] - r[0]), abs(o[1] - r[1]), o[2], o[3])


def crop_plan(corners, sizes, lir, aspect=1):
    """-> dict: "overlaps", "intersections" (prepare), "crops" (the rectangles crop_img cuts at `aspect`), "corners" / "sizes"
    (crop_rois at `aspect`)."""
    zc = zero_center_corners(corners)
    rects = [(c[0], c[1], s[0], s[1]) for c, s in zip(zc, sizes)]
    overlaps = [overlap(r, tuple(lir)) for r in rects]
    inters = [intersection(r, o) for r, o in zip(rects, overlaps)]
    scaled = [times(o, aspect) for o in overlaps]
    return {
        "overlaps": overlaps,
        "intersections": inters,
        "crops": [times(i, aspect) for i in inters],
        "corners": zero_center_corners([(r[0], r[1]) for r in scaled]),
        "sizes": [(r[2], r[3]) for r in scaled],
    }


def crop(img, r):
    """Cropper.crop_rectangle: numpy slicing (clips like the reference)"""
    return img[r[1]:r[1] + r[3], r[0]:r[0] + r[2]]
