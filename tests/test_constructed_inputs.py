"""The constructed input families (tests/constructed_inputs.py) without a GPU: every builder's stated facts hold against the numpy
contracts, and each family tells the contract from a plausibly wrong variant of it.

The variants below are restatements with ONE mistake each, of the kind a kernel can carry unnoticed; they live here, are numpy only
and are never imported by the product.  For every variant at least one constructed family gives a result that differs from the
contract's — that is the evidence that tests/test_gpu_constructed_inputs.py would fail on such a kernel — and the inputs the GPU suite
already had (the seeded noise of test_gpu_color_seams.py and test_gpu_cropper.py rebuilt with the same seeds, the cheap warped cases of
test_gpu_seam_estimation.py through the oracle's warper, with their images and panorama masks) are run through the same variants:

  variant                                          existing inputs that tell it from the contract
  colour seam, accumulators compared as int32      none (noise stays below 2^31: about 5e8 at L = 16384; nor the warped cases)
  colour seam, walk-back reaching 62 columns       none (noise seams wander a few columns; at most 70 rows; nor the warped cases)
  colour seam, ties t + 1 before t - 1             many: the 3-level images of test_two_images were made for it; fork_pair is kept as
                                                   the case where the tie provably lies on the seam
  voronoi, carry between 256-pixel steps dropped   "saturation" (one source, three rows); none of the small warped cases (their windows
                                                   stay within one step).  ragged and far_source add many sources, none, and a carry
                                                   over two steps
  LIR, walks stop at the chunk border              most noise up to 777 wide (chunks of 1 .. 4 bars) and the uniform 5000 x 3 and
  LIR, walks cross at most 3 chunk borders         3 x 6000 masks of test_tie_heavy_and_uniform_masks — the latter on the global-scratch
                                                   path (chunks of 24 bars, every walk crosses every chunk); NOT the 5200-wide noise and
                                                   its views.  So both paths were separated before, on bars that are all EQUAL; the
                                                   families add monotone runs and staircases of many values, on both pointer paths and
                                                   at W = 4864 / 4865
  contours, background 8-connected                 many (sparse noise has diagonal background neighbours); diagonal_mask(complement)
                                                   is kept for its exact count
Nothing here provokes a fault: these are host computations."""
import itertools
import os
import re

import numpy as np
import pytest
from scipy import ndimage

from stitching_amd import _lib, synthetic
from stitching_amd.seam_estimation import schedule
from tests import constructed_inputs as CI
from tests import numpy_color_seams as ZC
from tests import numpy_lir as ZL
from tests import numpy_seams as ZS
from tests import test_gpu_color_seams as GC
from tests import test_gpu_cropper as GL


CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "stitching_amd", "csrc")


def _constexpr(source, name):
    """the value of `constexpr int NAME = <integer or product of integers and earlier names>;` in a kernel source"""
    text = open(os.path.join(CSRC, source)).read()
    m = re.search(r"constexpr\s+int\s+%s\s*=\s*([^;]+);" % name, text)
    assert m, (source, name)
    value = 1
    for factor in m.group(1).split("*"):
        factor = factor.strip()
        value *= int(factor) if factor.isdigit() else _constexpr(source, factor)
    return value


def test_the_kernels_constants_are_the_ones_the_families_are_shaped_around():
    assert CI.ROW_STEP == _constexpr("stx_seams.hip", "SEAM_STEP") and _constexpr("stx_seams.hip", "SEAM_PX") == 4
    assert CI.COL_BATCH == _constexpr("stx_seams.hip", "SEAM_BATCH")
    assert CI.LIR_LANES == _constexpr("stx_crop.hip", "CROP_WG")
    assert CI.LIR_LDS_MAX_W == _constexpr("stx_crop.hip", "CROP_LDS_MAX_W")
    assert CI.LIR_ROWS_GRID == _constexpr("stx_crop.hip", "CROP_ROWS_GRID")
    assert CI.BACK == _constexpr("stx_color_seams.hip", "CS_BACK") and CI.SEAM_LANES == _constexpr("stx_color_seams.hip", "CS_WG")
    assert CI.MAX_SEAM_LENGTH == ZC.MAX_SEAM_LENGTH == _lib.COLOR_SEAM_MAX_LENGTH and CI.MAX_COST == ZC.MAX_COST and CI.GAP == ZS.GAP
    # the shapes lie around them
    assert {rw + 2 * CI.GAP for rw in CI.RAGGED_RW} >= {k * CI.ROW_STEP + d for k in (1, 2) for d in (-1, 0, 1)}
    assert {CI.COL_BATCH + d for d in (-1, 0, 1)} <= set(CI.RAGGED_RH)
    assert {CI.LIR_LDS_MAX_W, CI.LIR_LDS_MAX_W + 1, CI.LIR_LANES + 1} <= set(CI.HISTOGRAM_W)
    assert {k * CI.BACK + d for k in (1, 2) for d in (0, 1, 2)} <= set(CI.ZIGZAG_L) and {CI.BACK, CI.BACK + 1, CI.SEAM_LANES + 1} <= set(CI.ZIGZAG_W)


def _sizes(masks):
    return [(m.shape[1], m.shape[0]) for m in masks]


def _one_pair(corners, imgs, masks):
    (i, j, roi), = ZC.pairs(corners, _sizes(masks))
    return (roi,) + ZC.seam_in_pair(imgs, masks, corners, i, j, roi)


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------------------------------------------------
# the variants: one mistake each
# ---------------------------------------------------------------------------------------------------------------------------------
def variant_dp_seam(c, signed=False, right_first=False, reach=CI.BACK - 1):
    """numpy_color_seams.dp_seam with: accumulators compared as int32 (the out-of-range sentinel INT32_MAX) | the neighbour t + 1 tried
    before t - 1 | a walk back whose 64-row window holds choices only up to `reach` columns from where the step started (beyond it a
    stale 0, "straight", is read)"""
    c = np.asarray(c, np.int64)
    L, W = c.shape
    key = (lambda a: ((a + 2 ** 31) % 2 ** 32) - 2 ** 31) if signed else (lambda a: a)
    big = np.int64(2 ** 31 - 1) if signed else np.int64(1) << 40
    step = np.zeros((L, W), np.int8)
    A = c[0].copy()
    for r in range(1, L):
        best = A.copy()
        left = np.concatenate(([big], A[:-1]))
        right = np.concatenate((A[1:], [big]))
        for cand, d in ((right, 1), (left, -1)) if right_first else ((left, -1), (right, 1)):
            m = key(cand) < key(best)
            best[m], step[r][m] = cand[m], d
        A = c[r] + best
    t = int(np.argmin(key(A)))
    s = np.zeros(L, np.int32)
    s[L - 1] = t
    r_hi = L - 1
    while r_hi > 0:
        n, s_hi = min(CI.BACK, r_hi), t
        for q in range(n):
            t += int(step[r_hi - q][t]) if abs(t - s_hi) <= min(q, reach) else 0
            s[r_hi - q - 1] = t
        r_hi -= n
    return s


def variant_color_find(imgs, corners, masks, **kw):
    """numpy_color_seams.find with variant_dp_seam"""
    out = [np.array(m, np.uint8, copy=True) for m in masks]
    corners = [tuple(int(v) for v in c) for c in corners]
    sizes = _sizes(out)
    for i, j, roi in ZC.pairs(corners, sizes):
        x, y, w, h = roi
        both, c = ZC.pair_cost(imgs[i], corners[i], out[i], imgs[j], corners[j], out[j], roi)
        vertical, first_is_i = ZC.orientation(corners[i], sizes[i], corners[j], sizes[j])
        s = variant_dp_seam(c if vertical else c.T, **kw)
        second = np.arange(c.shape[1] if vertical else c.shape[0])[None, :] >= s[:, None]
        second = second if vertical else second.T
        first, last = (i, j) if first_is_i else (j, i)
        win = lambda k: out[k][y - corners[k][1]:y - corners[k][1] + h, x - corners[k][0]:x - corners[k][0] + w]  # noqa: E731
        win(first)[both & second] = 0
        win(last)[both & ~second] = 0
    return out


COLOR_VARIANTS = {"int32": {"signed": True}, "reach62": {"reach": CI.BACK - 2}, "right_first": {"right_first": True}}


def l1_distance_no_carry(src):
    """numpy_seams.l1_distance whose row sweeps forget the nearest source at every 256-pixel step of the window"""
    src = np.asarray(src, bool)
    h, w = src.shape
    g = np.full((h, w), ZS.DIST_SAT, np.int64)
    for x0 in range(0, w, CI.ROW_STEP):
        blk = src[:, x0:x0 + CI.ROW_STEP]
        xs = np.arange(blk.shape[1], dtype=np.int64)[None, :]
        last = np.maximum.accumulate(np.where(blk, xs, -(1 << 28)), axis=1)
        first = np.minimum.accumulate(np.where(blk, xs, 1 << 29)[:, ::-1], axis=1)[:, ::-1]
        g[:, x0:x0 + CI.ROW_STEP] = np.minimum(np.minimum(xs - last, first - xs), ZS.DIST_SAT)
    ys = np.arange(h, dtype=np.int64)[:, None]
    a = ys + np.minimum.accumulate(g - ys, axis=0)
    f = -ys + np.minimum.accumulate((a + ys)[::-1], axis=0)[::-1]
    return np.minimum(f, ZS.DIST_SAT).astype(np.int32)


def voronoi_find(corners, masks, distance):
    """numpy_seams.find("voronoi") with the distance transform `distance`"""
    out = [np.array(m, np.uint8, copy=True) for m in masks]
    corners = [tuple(int(v) for v in c) for c in corners]
    g = ZS.GAP
    for i, j, (x, y, w, h) in ZS.pairs(corners, _sizes(out)):
        s1 = ZS.cut(out[i], corners[i], x - g, y - g, w + 2 * g, h + 2 * g)
        s2 = ZS.cut(out[j], corners[j], x - g, y - g, w + 2 * g, h + 2 * g)
        both = (s1 != 0) & (s2 != 0)
        seam = (distance((s1 != 0) & ~both) < distance((s2 != 0) & ~both))[g:g + h, g:g + w]
        (xi, yi), (xj, yj) = corners[i], corners[j]
        out[j][y - yj:y - yj + h, x - xj:x - xj + w][seam] = 0
        out[i][y - yi:y - yi + h, x - xi:x - xi + w][~seam] = 0
    return out


def bars(mask):
    """-> v, left, right: the row stage's histogram rows and every bar's nearest strictly smaller bars"""
    v = CI.down_runs(mask)
    return (v,) + CI.nearest_smaller(v)


def lir_chunked(mask, hops=None, given=None):
    """The row stage of csrc/stx_crop.hip restated: bar x of row y spans (left, right), its nearest strictly smaller bars, and gives the
    rectangle of height v(y, x); the best by the tie rule.  hops None: the exact walks (this equals numpy_lir.lir, asserted below).
    hops k: a walk that leaves its lane's chunk of ceil(W / 256) bars crosses at most k further chunk borders and stops there."""
    v, lf, rt = given or bars(mask)
    H, W = v.shape
    if hops is not None:
        c = -(-W // CI.LIR_LANES)
        start = (np.arange(W) // c) * c
        lf = np.maximum(np.maximum(lf, (start - 1 - hops * c)[None, :]), -1)
        rt = np.minimum(np.minimum(rt, (start + c + hops * c)[None, :]), W)
    x0, w = lf + 1, rt - lf - 1
    area = v * w
    top = int(area.max())
    if top == 0:
        return (0, 0, 0, 0)
    ys, xs = np.nonzero(area == top)
    k = np.lexsort((-w[ys, xs], x0[ys, xs], ys))[0]
    y, x = ys[k], xs[k]
    return (int(x0[y, x]), int(y), int(w[y, x]), int(v[y, x]))


def lir_variants(mask):
    """-> (exact, walks stopping at the chunk border, walks crossing at most three more borders)"""
    given = bars(mask)
    return tuple(lir_chunked(mask, hops, given) for hops in (None, 0, 3))


def contours_bg8(mask):
    """numpy_lir.single_contour with the background taken as 8-connected too"""
    m = np.asarray(mask) != 0
    eight = np.ones((3, 3), bool)
    _, fg = ndimage.label(m, structure=eight)
    _, bg = ndimage.label(np.pad(~m, 1, constant_values=True), structure=eight)
    return int(fg), int(bg) - 1


# ---------------------------------------------------------------------------------------------------------------------------------
# colour seams: the builders' facts
# ---------------------------------------------------------------------------------------------------------------------------------
def test_zigzag_cover_is_pairwise_and_holds_the_named_rows():
    cases = CI.zigzag_cover()
    assert {(L, W) for L, W, _, _ in cases} >= {(L, 70) for L in CI.ZIGZAG_L} | {(200, W) for W in CI.ZIGZAG_W}
    for a, b in itertools.combinations(range(4), 2):
        seen = {(c[a], c[b]) for c in cases}
        assert seen == set(itertools.product({c[a] for c in cases}, {c[b] for c in cases})), (a, b)
    assert {c[0] for c in cases} == set(CI.ZIGZAG_L) and {c[1] for c in cases} == set(CI.ZIGZAG_W)
    # over the family a walk-back step starts with the seam on t = 0 and on t = W - 1, at the seam's end and at a later boundary
    starts = set()
    for L, W, _, first_is_j in cases:
        t = CI.zigzag_valley(L, W, anchor_high=first_is_j)
        starts |= {("low" if t[r] == 0 else "high", r == L - 1) for r, *_ in CI.window_drifts(t) if W > 3 and t[r] in (0, W - 1)}
    assert starts == set(itertools.product(("low", "high"), (True, False)))


@pytest.mark.parametrize("L", CI.ZIGZAG_L)
def test_zigzag_seam_is_the_valley_and_spans_the_window(L):
    for case in (c for c in CI.zigzag_cover() if c[0] == L):
        _, W, transpose, first_is_j = case
        corners, imgs, masks, f = CI.zigzag_pair(*case)
        roi, both, _, vertical, first_is_i, s = _one_pair(corners, imgs, masks)
        assert roi == f["roi"] and both.all()
        assert (vertical, first_is_i) == (not transpose, not first_is_j) == (f["vertical"], f["first_is_i"])
        t = f["valley"]
        assert np.array_equal(s, t), case
        assert np.all(np.abs(np.diff(t)) == 1) and t.min() >= 0 and t.max() < W
        # a walk-back window (from L - 1 in steps of 64) in which the seam drifts the window's full reach, or the whole width
        assert f["drift"] == max(d[2] for d in CI.window_drifts(s)) == min(CI.BACK - 1, W - 1), case
        if L > CI.BACK:  # with 65 rows or more a full step exists: the choice at the window's outermost column is read
            assert f["reach"] == min(CI.BACK - 1, W - 1)
        # the walk starts on a border; both are touched wherever L rows can span the W columns
        assert t[L - 1] == (W - 1 if first_is_j else 0)
        assert f["touches"] == (True, True) if L >= W else any(f["touches"])


def test_zigzag_shapes_of_the_issue():
    for (L, W), drift in (((200, 70), 63), ((333, 300), 63), ((150, 2), 1)):
        corners, imgs, masks, f = CI.zigzag_pair(L, W)
        assert np.array_equal(_one_pair(corners, imgs, masks)[5], f["valley"]) and f["drift"] == drift and f["touches"] == (True, True)


@pytest.mark.parametrize("W,jog", ((3, 0), (5, 0), (3, -1), (5, 1)))
def test_saturated_pair_straddles_2_31(W, jog):
    corners, imgs, masks, f = CI.saturated_pair(W, jog)
    roi, both, _, vertical, first_is_i, s = _one_pair(corners, imgs, masks)
    assert roi == f["roi"] == (3, 0, W, CI.MAX_SEAM_LENGTH) and both.all() and vertical and first_is_i
    _, c = ZC.pair_cost(imgs[0], corners[0], masks[0], imgs[1], corners[1], masks[1], roi)
    L, tc = f["L"], f["cheap"]
    # the columns' costs are constant (but for the jog's last row), one cheap and the rest black against white
    assert np.all(c[:L - 1] == c[0]) and c[0, tc] == f["c"] and np.all(np.delete(c[0], tc) == ZC.MAX_COST)
    assert ZC.MAX_COST * L == 3196108800 > 2 ** 31
    # from the column sums: the seam's accumulator ends below 2^31, its neighbour's lies at or above it in the row that is compared
    along = int(c[np.arange(L), f["seam"]].sum())
    assert along == f["seam_sum"] < 2 ** 31 <= f["neighbour_sum"] < 2 ** 32
    n_row, n_col = f["neighbour_row"], (tc + jog if jog else (tc - 1 if tc else tc + 1))  # the cheapest way into the neighbour
    assert int(c[:n_row, tc].sum()) + int(c[n_row, n_col]) == f["neighbour_sum"]
    assert int(c[:, tc].sum()) >= along and all(int(c[:, t].sum()) > 2 ** 31 for t in range(W) if t != tc)
    # the contract's seam lies in the cheap column (the jog: up to the last row, where it steps onto the free cell)
    assert np.array_equal(s, f["seam"]) and np.all(s[:L - 1] == tc) and s[L - 1] == tc + jog


def test_fork_pair_has_the_tie_on_the_seam():
    for transpose in (False, True):
        corners, imgs, masks, f = CI.fork_pair(transpose)
        roi, both, _, vertical, _, s = _one_pair(corners, imgs, masks)
        assert vertical == (not transpose) and np.array_equal(s, f["seam"])
        _, c = ZC.pair_cost(imgs[0], corners[0], masks[0], imgs[1], corners[1], masks[1], roi)
        c = c if vertical else c.T
        assert c[:4].sum() == 0 and c[4].tolist() == [0, 0, ZC.MAX_COST, 0, 0] and c[5].tolist() == [ZC.MAX_COST] * 2 + [0] + [ZC.MAX_COST] * 2


def test_mixed_level_schedule_and_empty_collisions():
    corners, imgs, masks, f = CI.mixed_level()
    sizes = _sizes(masks)
    pairs, levels = schedule(corners, sizes)
    assert [tuple(int(v) for v in p) for p in pairs] == f["pairs"] == [(i, j) + roi for i, j, roi in ZC.pairs(corners, sizes)]
    assert levels.tolist() == f["levels"] and int(levels.max()) + 1 == f["nlevels"]
    # level 0: one launch serves a 600-wide pair, a 3-wide one of 300 rows and a horizontal one
    geo = []
    for i, j, roi in ZC.pairs(corners, sizes):
        vertical, _ = ZC.orientation(corners[i], sizes[i], corners[j], sizes[j])
        geo.append(((roi[3], roi[2]) if vertical else (roi[2], roi[3]), vertical))
    assert [g[0] for g in geo] == f["LW"] and [g[1] for g in geo] == f["vertical"]
    assert [g[0] for g, l in zip(geo, levels) if l == 0] == [(5, 600), (300, 3), (40, 20)]
    # rows without `both` (cost 0 across the row) in the long pair, and a pair without `both` altogether
    want = [np.array(m, copy=True) for m in masks]
    for k, (i, j, roi) in enumerate(ZC.pairs(corners, sizes)):
        both, c = ZC.pair_cost(imgs[i], corners[i], want[i], imgs[j], corners[j], want[j], roi)
        if k == f["zero_cost_rows"][0]:
            rows = f["zero_cost_rows"][1]
            assert not both[rows].any() and not c[rows].any() and both[:rows.start].any() and both[rows.stop:].any()
        assert both.any() == (k != f["empty_both"])
        ZC.find_in_pair(imgs, want, corners, i, j, roi)
    assert _same(want, ZC.find(imgs, corners, masks)) and not _same(want, masks)


# ---------------------------------------------------------------------------------------------------------------------------------
# voronoi: the builders' facts
# ---------------------------------------------------------------------------------------------------------------------------------
def _uniques(corners, masks):
    (i, j, (x, y, w, h)), = ZS.pairs(corners, _sizes(masks))
    g = ZS.GAP
    s1 = ZS.cut(masks[i], corners[i], x - g, y - g, w + 2 * g, h + 2 * g)
    s2 = ZS.cut(masks[j], corners[j], x - g, y - g, w + 2 * g, h + 2 * g)
    both = (s1 != 0) & (s2 != 0)
    return (x, y, w, h), (s1 != 0) & ~both, (s2 != 0) & ~both


@pytest.mark.parametrize("rw", CI.RAGGED_RW)
def test_ragged_pair_windows_and_gap_sources(rw):
    assert rw + 2 * ZS.GAP in (255, 256, 257, 511, 512, 513, 620) and CI.GAP == ZS.GAP
    many = [0, 0]
    for rh, density in itertools.product(CI.RAGGED_RH, CI.RAGGED_DENSITY):
        corners, _, masks, f = CI.ragged_pair(rw, rh, density, 0)
        roi, u1, u2 = _uniques(corners, masks)
        assert roi == f["roi"] and roi[2:] == (rw, rh) and u1.shape == (rh + 2 * ZS.GAP, rw + 2 * ZS.GAP) == f["window"][::-1]
        assert {int(v) for m in masks for v in np.unique(m)} <= {0, 1, 254, 255}
        g = ZS.GAP
        gap = np.ones(u1.shape, bool)
        gap[g:g + rh, g:g + rw] = False
        assert (u1 & gap).any() and (u2 & gap).any()  # both images reach past the roi: sources in the gap
        # a roi row with no source of either image anywhere in the window, between rows that have some
        assert (f["blank_row"] is None) == (rh < 4)
        if f["blank_row"] is not None:
            y = f["blank_row"]
            assert g <= y < g + rh and not u1[y].any() and not u2[y].any() and (u1[y - 1] | u2[y - 1]).any() and (u1[y + 1] | u2[y + 1]).any()
        for k, u in enumerate((u1, u2)):  # several sources within one lane's 4 pixels
            many[k] += int((u[:, :u.shape[1] // 4 * 4].reshape(u.shape[0], -1, 4).sum(axis=2) >= 2).sum())
    assert min(many) > 0


def test_far_source_pair():
    corners, _, masks, f = CI.far_source_pair()
    roi, u1, u2 = _uniques(corners, masks)
    assert roi == f["roi"] and u1.shape[::-1] == f["window"] and u1.shape[1] > 2 * CI.ROW_STEP
    g, (rw, rh) = ZS.GAP, roi[2:]
    cols = np.arange(g, g + rw)
    for row in range(u1.shape[0]):
        got = {1: np.flatnonzero(u1[row]).tolist(), 2: np.flatnonzero(u2[row]).tolist()}
        if row in f["sources"]:
            who, col = f["sources"][row]
            assert got[who] == [col] and got[3 - who] == [], row
        else:
            assert got == {1: [], 2: []}, row  # no source at all
    for who in (1, 2):  # both images have a row whose only source is more than two steps (512 columns) from a roi pixel, on either side
        far = [np.abs(cols - col).max() for r, (w_, col) in f["sources"].items() if w_ == who and g <= col < g + rw]
        assert len(far) == 2 and min(far) > 2 * CI.ROW_STEP
    assert f["sources"][g + 9] == (1, 2) and 2 < g  # a source in the gap only
    # the row distance the contract sees there, before the column sweeps: a single row is its own distance transform
    d = ZS.l1_distance(u1[g + 2:g + 3])[0]
    assert d[g + rw - 1] == rw - 2 > 2 * CI.ROW_STEP


def test_tie_pair_ties_on_a_whole_column():
    corners, _, masks, f = CI.tie_pair()
    roi, u1, u2 = _uniques(corners, masks)
    assert np.array_equal(u2, u1[:, ::-1]) and u1.any()
    g = ZS.GAP
    d1, d2 = ZS.l1_distance(u1)[g:-g, g:-g], ZS.l1_distance(u2)[g:-g, g:-g]
    k = f["tie_column"]
    assert np.array_equal(d1[:, k], d2[:, k]) and d1[:, k].max() < ZS.DIST_SAT
    assert (d1 < d2).any() and (d2 < d1).any()
    want = ZS.find("voronoi", corners, masks)
    assert not want[0][:, k].any() and np.array_equal(want[1][:, k], masks[1][:, k])  # a tie zeroes mask i


# ---------------------------------------------------------------------------------------------------------------------------------
# largest interior rectangle: the builders' facts
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CI.PROFILES)
def test_histogram_masks_have_far_nearest_smaller_bars(name):
    for W, anchor in itertools.product(CI.HISTOGRAM_W, ("bottom", "top")):
        mask, f = CI.histogram_mask(name, W, anchor=anchor)
        h = f["profile"]
        assert mask.shape == (CI.HISTOGRAM_H, W) and h.min() >= 1 and h.max() <= CI.HISTOGRAM_H
        assert np.array_equal(np.count_nonzero(mask, axis=0), h)
        assert f["chunk"] == -(-W // 256) and f["in_lds"] == (W <= 4864)
        # a walk longer than three chunks.  Staircases and tents (and the standing valley) have such walks that END AT A SMALLER BAR;
        # in the comb, the sawtooth and the hanging valley smaller bars are near, and the long walks are those of the lowest bars,
        # which find none and run to the row's end across every chunk
        real = name in ("ascending", "descending", "tent") or (name, anchor) == ("valley", "bottom")
        assert CI.farthest_smaller(mask, real=real) > 3 * f["chunk"], (name, W, anchor)
        assert ZL.single_contour(mask) == (1, 0)
    if name in ("ascending", "descending"):  # hanging bars: every row is the whole staircase, 40 distinct values
        v = CI.down_runs(CI.histogram_mask(name, 700, anchor="top")[0])
        assert len(np.unique(v[0])) == CI.HISTOGRAM_H
        assert ZL.lir(CI.histogram_mask("ascending", 700)[0]) == (350, 19, 350, 21)
        assert ZL.lir(CI.histogram_mask("ascending", 5200)[0]) == (2600, 19, 2600, 21)


def test_notched_mask():
    mask, f = CI.notched_mask()
    assert mask.shape == (2100, 4865) and f["grid_stride"] and not f["in_lds"] and f["notches"] == 22
    ys, xs = np.nonzero(mask == 0)
    assert len(ys) == f["notches"] and np.all(np.diff(ys) == 97) and xs.min() > 0 and xs.max() < 4864 and ys.min() > 0 and ys.max() < 2099
    assert ZL.single_contour(mask) == (1, f["notches"])
    # rows of the whole mask as the kernel sees them, the one above the first notch among them: every bar of that row is
    # H - y high but the notch's column, the only smaller bar, thousands of columns from most
    assert CI.farthest_smaller(mask, rows=[0, int(ys[0]) - 1, int(ys[-1]) - 1], real=True) > 100 * f["chunk"]


def test_contour_masks_counts():
    for (mask, f), shape in ((CI.spiral_mask(), (401, 401)), (CI.spiral_mask(closed=True), (401, 401)), (CI.serpentine_mask(), (400, 400)),
                             (CI.rings_mask(50, 201), (201, 201)), (CI.rings_mask(50, 198), (198, 198)), (CI.rings_mask(50, 197), (197, 197)),
                             (CI.diagonal_mask(), (300, 300)), (CI.diagonal_mask(complement=True), (300, 300))):
        assert mask.shape == shape and max(shape) <= 600
        assert ZL.single_contour(mask) == f["counts"], (shape, f["counts"])
        if "length" in f:  # one pixel wide and 1e4 .. 1e5 long
            assert 10 ** 4 <= f["length"] == np.count_nonzero(mask) - (1 if f["counts"] == (1, 1) else 0) <= 10 ** 5
    assert CI.rings_mask(50, 201)[1]["counts"] == (50, 50) and CI.rings_mask(50, 198)[1]["counts"] == (50, 49)
    assert CI.diagonal_mask(complement=True)[1]["counts"] == (1, 298)


# ---------------------------------------------------------------------------------------------------------------------------------
# sensitivity: the families against the variants, and the inputs the GPU suite had before
# ---------------------------------------------------------------------------------------------------------------------------------
def _existing_color_inputs():
    """test_gpu_color_seams.py's seeded noise: test_two_images, test_every_columns_per_lane_kernel and the longest seam of
    test_limits_are_refused_and_the_context_stays_usable, with the same seeds and the same order of draws"""
    for cross, transpose in itertools.product(GC.CROSS, (False, True)):
        rng = np.random.default_rng(cross + 1000 * transpose)
        for length in GC.LENGTHS:
            corners, sizes = GC._side_by_side(cross, length, transpose)
            for levels in (256, 3):
                yield ("two_images", cross, transpose, length, levels), corners, GC._images(rng, sizes, levels), GC._masks(rng, sizes)
            yield ("two_images", cross, transpose, length, "j"), corners[::-1], GC._images(rng, sizes[::-1]), GC._masks(rng, sizes[::-1], 1.0)
    for cross in (300, 1000, 2000, 4000):
        rng = np.random.default_rng(cross)
        corners, sizes = GC._side_by_side(cross, 70, False)
        yield ("columns_per_lane", cross), corners, GC._images(rng, sizes, 3), GC._masks(rng, sizes)
    rng = np.random.default_rng(4)  # test_limits_...: its draws before the longest seam's
    for sizes, levels in (([(9, 5), (8, 5)], 256), ([(_lib.COLOR_SEAM_MAX_CROSS, 2)] * 2, 3)):
        GC._images(rng, sizes, levels), GC._masks(rng, sizes)
    sizes = [(1, ZC.MAX_SEAM_LENGTH)] * 2
    yield ("longest",), [(0, 0), (0, 0)], GC._images(rng, sizes), GC._masks(rng, sizes)


def test_color_seam_variants_are_told_apart_by_the_families_not_by_the_old_noise(oracle):
    separated = {k: [] for k in COLOR_VARIANTS}
    for name, corners, imgs, masks in _cheap_warped(oracle):  # smooth synthetic frames: few ties, short seams, small sums
        want = ZC.find(imgs, corners, masks)
        assert [k for k, kw in COLOR_VARIANTS.items() if not _same(variant_color_find(imgs, corners, masks, **kw), want)] == [], name
    for key, corners, imgs, masks in _existing_color_inputs():
        want = ZC.find(imgs, corners, masks)
        for name, kw in COLOR_VARIANTS.items():
            if not _same(variant_color_find(imgs, corners, masks, **kw), want):
                separated[name].append(key)
    assert separated["int32"] == [] and separated["reach62"] == []
    assert len(separated["right_first"]) > 0  # the old inputs already tell the tie order; fork_pair stays as the provable case

    def differs(name, corners, imgs, masks, *_):
        return not _same(variant_color_find(imgs, corners, masks, **COLOR_VARIANTS[name]), ZC.find(imgs, corners, masks))

    # accumulators above 2^31: the final arg-min (jog 0) and the comparison on the seam (jog -1: right < best, jog +1: left < best)
    for W, jog in ((3, 0), (5, 0), (3, -1), (5, 1)):
        assert differs("int32", *CI.saturated_pair(W, jog)), (W, jog)
    # the window's full reach: every zigzag of 65 rows or more and 64 columns or more; 64 rows never walk a full step
    for L, W, transpose, first_is_j in CI.zigzag_cover():
        assert differs("reach62", *CI.zigzag_pair(L, W, transpose, first_is_j)) == (L > CI.BACK and W >= CI.BACK), (L, W)
        assert not differs("int32", *CI.zigzag_pair(L, W, transpose, first_is_j))
    for transpose in (False, True):
        assert differs("right_first", *CI.fork_pair(transpose))
    assert not any(differs(name, *CI.mixed_level()) for name in ("int32", "reach62"))  # mixed_level aims at the launch, not at these


def _cheap_warped(oracle):
    """test_gpu_seam_estimation.py's small warped cases and config 2's ring at low resolution (test_gpu_cropper.py's _low(2)) through
    the oracle's warper (bit-exact with the device's: test_gpu_parity.py).  -> name, corners, warped images, warped masks"""
    for name, wtype, n, w, h in (("n2_cyl", "cylindrical", 2, 192, 144), ("n3_sph", "spherical", 3, 192, 144),
                                 ("n4_affine", "affine", 4, 160, 120), ("config2_low", "spherical", 8, GL.LW, GL.LH)):
        if name == "config2_low":
            cams = synthetic.ring_cameras(n, w, h, focal_factor=0.75)
        elif wtype == "affine":
            cams = synthetic.affine_scan_cameras(n, w, h)
        else:
            cams = synthetic.ring_cameras(n, w, h, focal_factor=0.75, span_deg=min(340.0, 45.0 * n))
        wp = oracle.Warper(wtype)
        wp.set_scale(cams)
        imgs = [np.asarray(a) for a in wp.warp_images(synthetic.make_frames(range(n), w, h), cams, 1)]
        masks = [np.asarray(m) for m in wp.create_and_warp_masks([(w, h)] * n, cams, 1)]
        corners, _ = wp.warp_rois([(w, h)] * n, cams, 1)
        yield name, [tuple(int(v) for v in c) for c in corners], imgs, masks


def _panorama_mask(corners, masks):
    """the union of the masks on the panorama (what Cropper.estimate_panorama_mask hands the cropper)"""
    x0, y0 = min(c[0] for c in corners), min(c[1] for c in corners)
    x1 = max(c[0] + m.shape[1] for c, m in zip(corners, masks))
    y1 = max(c[1] + m.shape[0] for c, m in zip(corners, masks))
    pano = np.zeros((y1 - y0, x1 - x0), np.uint8)
    for c, m in zip(corners, masks):
        pano[c[1] - y0:c[1] - y0 + m.shape[0], c[0] - x0:c[0] - x0 + m.shape[1]] |= m
    return pano


def test_voronoi_carry_variant(oracle):
    for x in (5, 300, 700):  # one source in a row of three steps: the variant forgets it beyond its own step
        src = np.zeros((1, 720), bool)
        src[0, x] = True
        step = np.arange(720) // CI.ROW_STEP == x // CI.ROW_STEP
        assert np.array_equal(l1_distance_no_carry(src)[0] == ZS.l1_distance(src)[0], step)
    separated = []
    for name, corners, _, masks in _cheap_warped(oracle):
        want = ZS.find("voronoi", corners, masks)
        assert _same(voronoi_find(corners, masks, ZS.l1_distance), want)
        if not _same(voronoi_find(corners, masks, l1_distance_no_carry), want):
            separated.append(name)
    w = 9000  # "saturation"
    a, b = np.full((3, w), 255, np.uint8), np.full((3, w), 255, np.uint8)
    b[:, 0] = 0
    if not _same(voronoi_find([(0, 0), (0, 0)], [a, b], l1_distance_no_carry), ZS.find("voronoi", [(0, 0), (0, 0)], [a, b])):
        separated.append("saturation")
    # the old suite tells this variant on one source and three rows; the warped rois (at most 254 wide) never leave one step
    assert separated == ["saturation"]
    corners, _, masks, _ = CI.far_source_pair()
    assert not _same(voronoi_find(corners, masks, l1_distance_no_carry), ZS.find("voronoi", corners, masks))
    told = 0
    for rw, rh in itertools.product((493, 600), CI.RAGGED_RH):
        corners, _, masks, _ = CI.ragged_pair(rw, rh, 0.1, 0)
        want = ZS.find("voronoi", corners, masks)
        assert _same(voronoi_find(corners, masks, ZS.l1_distance), want)
        told += not _same(voronoi_find(corners, masks, l1_distance_no_carry), want)
    assert told > 0


def _existing_lir_inputs():
    """test_gpu_cropper.py's seeded noise (test_random_masks), the 300 x 5200 mask of test_views_and_pitched_buffers with its views,
    and the masks of test_tie_heavy_and_uniform_masks that are wider than a chunk or than LDS holds"""
    for hw in GL.SIZES:
        rng = np.random.default_rng(hash(hw) % 2 ** 32)
        for p in (0.05, 0.5, 0.9, 0.995):
            yield (hw, p), np.where(rng.random(hw) < p, 255, 0).astype(np.uint8)
        yield (hw, "grey"), (rng.random(hw) < 0.97).astype(np.uint8) * rng.integers(1, 256, hw, dtype=np.uint8)
    rng = np.random.default_rng(11)
    big = np.where(rng.random((300, 5200)) < 0.93, 255, 0).astype(np.uint8)
    yield ((300, 5200), 0.93), big
    for y0, y1, x0, x1 in ((7, 250, 3, 200), (1, 2, 5, 4990), (30, 290, 100, 5199)):
        yield ((y1 - y0, x1 - x0), "view"), big[y0:y1, x0:x1]
    yield ((5000, 3), "uniform"), np.full((5000, 3), 1, np.uint8)
    yield ((3, 6000), "uniform"), np.full((3, 6000), 1, np.uint8)


def test_lir_walk_variants(oracle):
    """Both variants WERE told apart before, on either pointer path: masks up to 256 wide have chunks of ONE bar, where every walk
    crosses chunks; the uniform 3 x 6000 mask lies on the global-scratch path and every one of its walks crosses every chunk; warped
    panorama masks are blobs far wider than a chunk.  What those inputs share is that the bars a long walk passes are all EQUAL
    (full columns), or the walk is short (noise).  The families add long walks over monotone runs and staircases of many values, on
    both paths and at W = 4864 / 4865 — and they tell both variants too, which is asserted here."""
    stop_at_border, three_hops = [], []
    for key, mask in _existing_lir_inputs():
        if mask.size > 2 * 10 ** 6 and key[1] not in (0.5, 0.995):  # of the 4097 x 777 masks two densities are enough here
            continue
        want = ZL.lir(mask)
        exact, v0, v3 = lir_variants(mask)
        assert exact == want, key
        stop_at_border += [key] * (v0 != want)
        three_hops += [key] * (v3 != want)
    assert set(three_hops) <= set(stop_at_border)
    # wider than LDS holds: the uniform mask tells both, the 1 x 4985 view the border variant, the 5200-wide noise and its other view none
    assert [k for k in stop_at_border if k[0][1] > CI.LIR_LDS_MAX_W] == [((1, 4985), "view"), ((3, 6000), "uniform")]
    assert [k for k in three_hops if k[0][1] > CI.LIR_LDS_MAX_W] == [((3, 6000), "uniform")]
    assert ((5000, 3), "uniform") in stop_at_border and ((5000, 3), "uniform") not in three_hops  # three chunks of one bar
    assert any(k[0][1] <= CI.LIR_LDS_MAX_W for k in three_hops)
    for name, corners, _, masks in _cheap_warped(oracle):  # the low-resolution panorama masks: every one tells both variants
        pano = _panorama_mask(corners, masks)
        exact, v0, v3 = lir_variants(pano)
        assert exact == ZL.lir(pano) and v0 != exact and v3 != exact and pano.shape[1] <= CI.LIR_LDS_MAX_W, name
    for name, W, anchor in itertools.product(CI.PROFILES, CI.HISTOGRAM_W, ("bottom", "top")):
        mask, _ = CI.histogram_mask(name, W, anchor=anchor)
        exact, v0, v3 = lir_variants(mask)
        assert exact == ZL.lir(mask)
        if name in ("ascending", "descending", "tent") or (name in ("comb", "sawtooth") and W >= 700):
            assert v0 != exact and v3 != exact, (name, W, anchor)  # at every width, on both pointer paths
    notched, _ = CI.notched_mask()
    exact, v0, v3 = lir_variants(notched[:300])
    assert exact == ZL.lir(notched[:300]) and v0 != exact and v3 != exact


def test_contour_variant_background_8_connected():
    told = [key for key, mask in _existing_lir_inputs() if mask.size <= 300 * 300 and contours_bg8(mask) != ZL.single_contour(mask)]
    assert told  # sparse noise already tells it; the complement of the diagonal does so with an exact count
    mask, f = CI.diagonal_mask(complement=True)
    assert ZL.single_contour(mask) == f["counts"] == (1, 298) and contours_bg8(mask) == (1, 1)
    for mask, f in (CI.spiral_mask(), CI.spiral_mask(closed=True), CI.serpentine_mask(), CI.rings_mask(50, 201)):
        assert contours_bg8(mask) == ZL.single_contour(mask) == f["counts"]  # corridors one pixel wide are 4-connected: no difference
