"""The constructed exposure families (tests/constructed_exposures.py) without a GPU: the constants they are shaped around are the ones
in the sources, every family's stated facts hold against the CPU contracts (tests/numpy_exposure.py for the estimation; the oracle's
gain_apply / block_gain_apply / resize_linear_f32 for the apply), and each family tells the contract from a plausibly wrong variant.

The variants are restatements with ONE mistake each, of the kind the kernels and the plan can carry unnoticed; they live here or in
the constructed module, are numpy only and are never imported by the product:

  variant                                                        family that tells it from the contract
  b's read offset taken from a's                                 E2 placements (wherever the two offsets differ)
  blocks of bl pixels instead of ceil(w / ceil(w / bl))          E3 block grids (wherever bw != bl)
  a mask of 254, or any non-zero mask, counts                    E4 mask levels
  the sequential sum | a contiguous run per lane                 E5 tree order
  half away from zero | half up | truncation                     A1 ties
  an out-of-range product saturates to 255                       A2 int-range edge
  a row table covering the first ceil(w / 256) * 256 rows only   A3 geometry (h > 256 >= w)
Nothing here provokes a fault: these are host computations."""
import functools
import os
import re

import numpy as np
import pytest

from oracle import oracle as O
from tests import constructed_exposures as CE
from tests import numpy_exposure as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stitching_amd", "csrc")


def _src(name, where=CSRC):
    return open(os.path.join(where, name)).read()


def _int(pattern, text):
    m = re.search(pattern, text)
    assert m, pattern
    return int(m.group(1))


def test_the_kernels_constants_are_the_ones_the_families_are_shaped_around():
    exp, exp_host, gain = _src("stx_exposure.hip"), _src("stx_exposure_host.cpp"), _src("stx_gain.hip")
    py = _src("exposure_error_compensator.py", os.path.join(ROOT, "stitching_amd"))
    assert CE.EXP_WG == _int(r"constexpr\s+int\s+EXP_WG\s*=\s*(\d+)\s*;", exp)
    assert len(re.findall(r"__launch_bounds__\(EXP_WG\)", exp)) == 2 and re.search(r"const int cnt = min\(EXP_WG, n - base\);", exp)
    assert re.search(r"for \(int s = EXP_WG / 2; s > 0; s >>= 1\) \{  // fixed pairing: lane t adds lane t \+ s", exp)
    assert CE.BLOCK_MUL_GRID == _int(r"const int gx = std::min\((\d+), std::max\(1, \(max_pixels \+ EXP_WG - 1\) / EXP_WG\)\);", exp)
    m = re.search(r"constexpr\s+int\s+EXP_SQRT_N\s*=\s*3 \* (\d+) \* (\d+) \+ 1\s*;", exp_host)
    assert m and CE.EXP_SQRT_N == 3 * int(m.group(1)) * int(m.group(2)) + 1 == 3 * 255 * 255 + 1
    assert CE.GAIN_BATCH == _int(r"constexpr\s+int\s+GAIN_BATCH\s*=\s*(\d+)\s*;", gain)
    assert re.findall(r"const int x4 = \(blockIdx\.x \* 64 \+ \(threadIdx\.x & 63\)\) \* (\d);", gain) == [str(CE.PIXEL_GROUP)] * 2
    assert CE.GAIN4_ROWS == _int(r"const int y = blockIdx\.y \* (\d+) \+ wv \* 4 \+ j;", gain)
    assert CE.GAIN4_ROWS == _int(r"const dim3 grid\(\(mw \+ 255\) / 256, \(mh \+ 15\) / (\d+), m\);", gain)
    assert CE.GAIN_ROWS_WG == _int(r"const int i = blockIdx\.x \* (\d+) \+ threadIdx\.x;", gain)
    assert CE.GAIN_ROWS_WG == _int(r"const dim3 grid\(\(mt \+ 255\) / (\d+), mgh \+ 1, m\);", gain)
    assert re.search(r"mt = std::max\(mt, std::max\(B\.k\[i\]\.w, B\.k\[i\]\.h\)\);", gain)  # block row 0 writes the per-row table
    assert CE.BOUNDED_BELOW == float(re.search(r"np\.abs\(g\)\.max\(initial=0\.0\) < ([0-9.e]+)\)", py).group(1))
    assert CE.BOUNDED_BELOW < float(CE.INT_EDGE_F32) == 8421504.0 < CE.INT_EDGE < 8421505.0
    assert re.search(r"if \(!FAST\) v = v < 2147483648\.f \? v : 0\.f;", gain)
    # rows that are not dword-aligned take the per-byte path of gain_apply_kernel
    assert re.search(r"K\.dwords = \(\(uintptr_t\)img->ptr & 3\) == 0 && \(img->stride & 3\) == 0;", gain)
    assert re.search(r"if \(P\.dwords && x4 \+ 4 <= P\.w\) \{", gain)
    # the shapes lie around them
    assert {CE.EXP_WG * k + d for k in (1, 2) for d in (-1, 0, 1)} | {1, 2, 4 * CE.EXP_WG + 1} <= set(CE.JOB_SIZES)
    ws, hs = {g[0] for g in CE.GEOMETRY}, {g[1] for g in CE.GEOMETRY}
    assert {1, 2, 3, 4, 5} | {CE.GAIN_ROWS_WG + d for d in (-1, 0, 1)} <= ws and {1, 2 * CE.GAIN4_ROWS + 1} | {CE.GAIN4_ROWS + d for d in (-1, 0, 1)} <= hs
    assert sum(h > CE.GAIN_ROWS_WG >= w for w, h, _, _ in CE.GEOMETRY) == 2 and {w % CE.PIXEL_GROUP for w in CE.TIE_WIDTHS} == {0, 1, 2, 3}
    px = CE.between_feeds("small_and_large").facts["pixels"]
    assert px[0] <= CE.EXP_WG and px[1] > CE.BLOCK_MUL_GRID * CE.EXP_WG
    assert CE.KINDS == X.KINDS


# ---------------------------------------------------------------------------------------------------------------------------------
# the contract of the estimation
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _feed(builder, args, kind, nr_feeds=1, bl=None):
    """(scene, gains, the first feed's jobs, units) by the restatement: once per case"""
    s = getattr(CE, builder)(*args)
    gains, first, units = X.feed(kind, s.corners, s.imgs, s.masks, nr_feeds, bl or s.bl, want_stats=True)
    return s, gains, first, units


def _by_image_pair(first, units):
    """the jobs summed per pair of images.  Blocks partition their image: the jobs of the blocks of i and j partition the overlap of
    i and j, and the jobs of the blocks of i with themselves partition image i"""
    out = {}
    for (a, b), (c, sa, sb) in first.items():
        t = out.setdefault((units[a][0], units[b][0]), [0, np.zeros(len(sa)), np.zeros(len(sb))])
        t[0] += c
        t[1] += np.asarray(sa, np.float64)
        t[2] += np.asarray(sb, np.float64)
    return out


def _check_coded_pairs(s, first, units):
    """channel kinds: the contract's integer sums are the construction's, per image pair"""
    got = _by_image_pair(first, units)
    assert set(got) == set(s.facts["pairs"])
    for (i, j), (c, sa, sb) in s.facts["pairs"].items():
        assert got[(i, j)][0] == c and tuple(got[(i, j)][1]) == sa and tuple(got[(i, j)][2]) == sb, (i, j)


@pytest.mark.parametrize("layout", CE.LAYOUTS)
@pytest.mark.parametrize("n", CE.JOB_SIZES)
def test_job_sizes(n, layout):
    for mode in CE.MASK_MODES:
        s = CE.job_sizes(n, layout, mode)
        f = s.facts
        assert f["w"] * f["h"] == n and f["pairs"][(0, 1)][0] == f["c"] == {"full": n, "first_chunk_off": max(0, n - CE.EXP_WG),
                                                                            "last_chunk_off": n - f["last_chunk"]}[mode]
        assert 1 <= f["last_chunk"] <= CE.EXP_WG and (f["chunks"] - 1) * CE.EXP_WG + f["last_chunk"] == n
        for kind in X.KINDS:
            _, gains, first, units = _feed("job_sizes", (n, layout, mode), kind)
            assert len(units) == 2 and set(first) == {(0, 0), (0, 1), (1, 1)}  # one block per image for the block kinds
            c, sa, sb = first[(0, 1)]
            assert c == f["c"]
            if kind.startswith("channel"):
                _check_coded_pairs(s, first, units)
            if c == 0:
                assert all((g == 1).all() for g in gains)


@pytest.mark.parametrize("which", CE.PLACEMENTS)
def test_placements(which):
    s = CE.placements(which)
    f = s.facts
    touching = which.startswith("touch")
    assert (f["overlap"] is None) == touching
    assert f["overlap"] == {"inside": (9, 7), "identical": (23, 17), "column": (1, 17), "row": (23, 1), "pixel": (1, 1),
                            "negative": (13, 8)}.get(which)
    for kind in X.KINDS:
        _, gains, first, units = _feed("placements", (which,), kind)
        cross = [k for k in first if units[k[0]][0] != units[k[1]][0]]
        if touching:  # no pair job, both units skipped, gains exactly 1
            assert not cross and all((g == 1).all() for g in gains)
            assert all(X.stats_matrices(len(units), first, 0)[2])
            continue
        assert cross
        if kind.startswith("channel"):
            _check_coded_pairs(s, first, units)
    if touching:
        return
    # the variant: b read at a's offset (clamped into b)
    (ox, oy), (bx, by) = f["offsets"]
    w, h = f["overlap"]
    b = s.imgs[1]
    yy, xx = np.mgrid[0:h, 0:w]
    wrong = b[np.minimum(yy + oy, b.shape[0] - 1), np.minimum(xx + ox, b.shape[1] - 1)].reshape(-1, 3).astype(np.int64).sum(axis=0)
    assert (tuple(int(v) for v in wrong) == f["pairs"][(0, 1)][2]) == ((ox, oy) == (bx, by)) == (which == "identical")
    if which == "inside":  # the block kinds: a pair whose two read offsets are both non-zero and unequal
        _, _, first, units = _feed("placements", (which,), "channel_blocks")
        ua = next(k for k, u in enumerate(units) if u[:3] == (0, 8, 12))  # a's blocks are 8 x 6, b's 5 x 7
        ub = next(k for k, u in enumerate(units) if u[:3] == (1, 5, 0))
        assert (ua, ub) in first and first[(ua, ub)][0] == 4 * 1  # global (14, 15) .. (18, 16): a read at (9, 12), b at (5, 6)


def _units_bw_is_bl(sizes, bl):
    return [(i, x, y, min(x + bl, w), min(y + bl, h)) for i, (w, h) in enumerate(sizes) for y in range(0, h, bl) for x in range(0, w, bl)]


@pytest.mark.parametrize("which", CE.BLOCK_GRIDS)
def test_block_grids(which):
    s = CE.block_grids(which)
    f = s.facts
    assert [X.block_grid(w, h, s.bl) for w, h in s.sizes] == f["grids"]
    _, gains, first, units = _feed("block_grids", (which,), "channel_blocks")
    assert len(units) == f["units"] and [g.shape[:2] for g in gains] == [(g[1], g[0]) for g in f["grids"]]
    cross = [k for k in first if units[k[0]][0] != units[k[1]][0]]
    assert len(cross) == f["cross_pairs"] and len(first) == f["units"] + f["cross_pairs"]
    bpw = f["grids"][0][0]
    meets = {}
    for a, _ in cross:
        meets[(a % bpw, a // bpw)] = meets.get((a % bpw, a // bpw), 0) + 1
    assert meets == f["meets"]
    assert {"33_32": lambda: f["grids"][0][2] == 17, "50_8": lambda: f["grids"][0][2] == 8 and 50 % 8 == 2,
            "50_12": lambda: f["grids"][0][2] == 10, "bl1": lambda: f["units"] == 60, "bl_large": lambda: f["units"] == 2,
            "aligned": lambda: set(meets.values()) == {1}, "off_by_one": lambda: max(meets.values()) == 4 and meets[(3, 2)] == 4,
            "two_sizes": lambda: f["grids"][0][2:] != f["grids"][1][2:]}[which]()
    _check_coded_pairs(s, first, units)
    # the variant: blocks of bl pixels
    wrong = _units_bw_is_bl(s.sizes, s.bl)
    assert (wrong != [tuple(u) for u in units]) == f["cut_differs"] == (which in ("33_32", "50_8", "50_12", "two_sizes"))
    if f["cut_differs"]:
        jobs, _ = X.pair_stats(s.corners, s.imgs, s.masks, wrong, (0, 1, 2))
        assert jobs != first


@pytest.mark.parametrize("which", CE.VALUES)
def test_values(which):
    s = CE.values(which)
    f = s.facts
    if which in ("white", "black"):
        assert f["table_index"] == (CE.EXP_SQRT_N - 1 if which == "white" else 0)
        _, gains, first, units = _feed("values", (which,), "gain")
        c, sa, sb = first[(0, 1)]
        N, I, skip = X.stats_matrices(2, first, 0)
        assert c == f["c"] == 12 * 9 and sa[0] == sb[0] == X.seq_sum(np.full(c, f["norm"])) and not skip.any()
        assert I[0, 1] == I[1, 0] and abs(I[0, 1] - f["norm"]) <= 1e-12 * f["norm"]
        assert all(np.abs(g - 1).max() < 1e-12 for g in gains)  # equal intensities: nothing to compensate
        return
    if which == "mask_levels":
        _, _, first, units = _feed("values", (which,), "channel")
        assert first[(0, 1)][0] == f["c"] < f["c_if_254_counts"] < f["c_if_nonzero_counts"]
        _check_coded_pairs(s, first, units)
        return
    for kind in ("gain", "channel"):
        _, gains, first, units = _feed("values", (which,), kind)
        assert f["empty_pair"] in first and {k: first[k][0] for k in f["c"]} == f["c"]
        N, I, skip = X.stats_matrices(3, first, 0)
        assert N[0, 1] == 1 and I[0, 1] == 0 and I[1, 0] == 0 and not skip.any()
        assert all(np.isfinite(g).all() for g in gains) and not all((g == 1).all() for g in gains)


def test_tree_order():
    """the order exposure_stats_kernel documents for the "gain" kind differs in bits from the sequential sum and from a contiguous run
    per lane, and stays within the 1e-12 the project compares it at"""
    scenes = [CE.job_sizes(n, "square") for n in CE.JOB_SIZES] + [CE.tree_large()]
    differs_seq = differs_run = 0
    for s in scenes:
        key = ("tree_large", ()) if s is scenes[-1] else ("job_sizes", (s.facts["n"], "square"))
        first = _feed(*key, "gain")[2]
        for (i, j), (c, *vals) in CE.norm_jobs(s).items():
            assert c == first[(i, j)][0] and [X.seq_sum(v) for v in vals] == [first[(i, j)][1][0], first[(i, j)][2][0]]  # the contract's
            for v in vals:
                t, q, r = CE.tree_sum(v), X.seq_sum(v), CE.tree_sum_contiguous(v)
                assert abs(t - q) <= 1e-12 * abs(q)
                differs_seq += t != q
                differs_run += t != r
    assert differs_seq >= 1 and differs_run >= 1
    big = CE.norm_jobs(scenes[-1])[(0, 1)][1]
    assert big.size == 102000 and CE.tree_sum(big) != X.seq_sum(big)
    assert CE.tree_sum([]) == 0.0 and CE.tree_sum([1.5]) == 1.5 and CE.tree_sum(np.arange(1000.0)) == 499500.0


def _first_feed_unit_gains(kind, s):
    _, _, first, units = _feed(*s, kind)
    planes = 3 if kind.startswith("channel") else 1
    g = np.array([X.single_feed_gains(*X.stats_matrices(len(units), first, p)) for p in range(planes)])
    return g, units


@pytest.mark.parametrize("which", CE.BETWEEN_FEEDS)
def test_between_feeds(which):
    s = CE.between_feeds(which)
    kinds = ("gain", "channel") if which == "tails" else X.KINDS
    for kind in kinds:
        g, units = _first_feed_unit_gains(kind, ("between_feeds", (which,)))
        assert np.abs(g - 1).max() > 0.2  # the first feed's gains are far from 1
        saturating = 0
        for u, (i, x0, y0, x1, y1) in enumerate(units):
            saturating += int((s.imgs[i][y0:y1, x0:x1].astype(np.float32) * g[:, u].astype(np.float32)[None, None, :] > 255.5).sum())
        assert saturating >= 1
        one, two, three = (_feed("between_feeds", (which,), kind, k)[1] for k in (1, 2, 3))
        assert any(not np.array_equal(a, b) for a, b in zip(one, two)) and any(not np.array_equal(a, b) for a, b in zip(two, three))
    if which != "tails":
        assert all(bw != s.bl for bw, _ in s.facts["block_sizes"][-1:])


@pytest.mark.parametrize("grid", CE.FILTER_GRIDS)
def test_filter_shapes(grid):
    for kind in ("gain_blocks", "channel_blocks"):
        s, gains, _, units = _feed("filter_shapes", (grid,), kind)
        assert [g.shape[:2] for g in gains] == [grid, grid] and len(units) == 2 * grid[0] * grid[1]
        g, _ = _first_feed_unit_gains(kind, ("filter_shapes", (grid,)))
        raw = g[:, :grid[0] * grid[1]].astype(np.float32).reshape(-1, *grid).transpose(1, 2, 0)
        raw = raw if kind == "channel_blocks" else raw[..., 0]
        assert np.array_equal(gains[0], X.filter_gain_map(raw))
        assert np.array_equal(gains[0], raw) == (grid == (1, 1))  # a 1-long axis stays; longer ones are smoothed
        if grid[0] == 1 and grid[1] > 1:  # the only pass is the horizontal one, twice
            assert np.array_equal(gains[0], X._smooth_axis(X._smooth_axis(raw, 1), 1))
        if grid == (2, 2):  # reflection at length 2: 0.5 c + 0.25 (o + o), the other element twice
            o = raw[:, ::-1]
            assert np.array_equal(X._smooth_axis(raw, 1), (np.float32(0.5) * raw + np.float32(0.25) * (o + o)).astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------------------------
# the apply families
# ---------------------------------------------------------------------------------------------------------------------------------
def _count(a, b):
    return int(np.count_nonzero(a != b))


def test_interp_gains_is_the_oracles_resize():
    for w, h, gw, gh in CE.GEOMETRY + ((64, 32, 8, 4), (25, 15, 5, 3)):
        _, gmap = CE.geometry(w, h, gw, gh)
        want = O.resize_linear_f32(gmap, (w, h)) if (gw, gh) != (w, h) else gmap
        assert np.array_equal(CE.interp_gains(gmap, w, h)[..., 0].view(np.uint32), np.asarray(want).view(np.uint32)), (w, h, gw, gh)
    fw, fh, gw, gh = CE.SUB_FULL
    _, gmap = CE.geometry(fw, fh, gw, gh)
    full = CE.interp_gains(gmap, fw, fh)
    for x0, y0, w, h in CE.SUB_RECTS:
        assert np.array_equal(CE.interp_gains(gmap, w, h, (fw, fh, x0, y0)), full[y0:y0 + h, x0:x0 + w])


@pytest.mark.parametrize("channels", (1, 3))
def test_ties_blocks(channels):
    img, gmap, f = CE.ties(channels)
    CE.assert_tie_facts(f)
    assert 0.4 < f["admits_tie"] < 0.6
    want = O.block_gain_apply(img, gmap)
    p = CE.products(img, CE.interp_gains(gmap, img.shape[1], img.shape[0]))
    assert np.array_equal(want, CE.saturate(p))
    assert _count(want, CE.saturate(p, CE.half_up)) >= f["ties_down"] and _count(want, CE.saturate(p, CE.half_away)) >= f["ties_down"]
    assert _count(want, CE.saturate(p, np.trunc)) >= f["ties_up"]


@pytest.mark.parametrize("w", CE.TIE_WIDTHS)
def test_ties_scalar_ramp(w):
    img, f = CE.tie_ramp(w)
    assert f["all_values"] and f["odd_bytes"] >= 300
    for g in CE.TIE_SCALARS + (CE.TIE_SCALARS,):
        want = O.gain_apply(img, g)
        p = CE.products(img, g)
        assert np.array_equal(want, CE.saturate(p))
        for wrong in (CE.half_up, CE.half_away, np.trunc):
            assert _count(want, CE.saturate(p, wrong)) >= 50


@pytest.mark.parametrize("channels", (1, 3))
@pytest.mark.parametrize("which", CE.EDGE_MAPS)
def test_int_edge(which, channels):
    img, gmap, f = CE.int_edge(which, channels)
    assert f["bounded"] == (which == "below_bound")
    want = O.block_gain_apply(img, gmap)
    p = CE.products(img, CE.interp_gains(gmap, img.shape[1], img.shape[0]))
    assert np.array_equal(want, CE.saturate(p))
    c = CE.EDGE_BLOCK // 2
    if which == "edge":
        assert f["at_or_above_2_31"] >= 1 and f["largest_below_2_31"] >= 1
        with np.errstate(invalid="ignore"):
            to_255 = np.where(p >= 2.0 ** 31, 255, CE.saturate(p))
        assert _count(want, to_255) == f["at_or_above_2_31"]  # the variant: such a product saturates to 255
        if channels == 1:  # 255 x 8421504 = 2^31 - 128 -> 255; 255 x 8421503 -> 255; 255 x 8421505 rounds to 2^31 -> INT_MIN -> 0
            assert [want[c, c + 10 * k].tolist() for k in range(3)] == [[255, 255, 0], [255, 255, 0], [0, 255, 0]]
    if which == "inf":
        assert f["zero_times_inf"] and f["nan_products"] >= 1
        if channels == 1:
            assert want[c, c].tolist() == [0, 0, 0]  # inf, inf, and 0 x inf = NaN: all INT_MIN
    if which == "nan":
        assert f["nan_products"] >= 3 and (channels == 3 or want[c, c].tolist() == [0, 0, 0])
    if which == "below_bound" and channels == 1:  # 7999999.5, -0.0, -3, a subnormal
        assert [want[c, c + 10 * k].tolist() for k in range(3)] == [[255, 255, 0], [0, 0, 0], [0, 0, 0]] and want[2 * CE.EDGE_BLOCK + c, c].tolist() == [0, 0, 0]


@pytest.mark.parametrize("channels", (1, 3))
def test_geometry(channels):
    for w, h, gw, gh in CE.GEOMETRY:
        img, gmap = CE.geometry(w, h, gw, gh, channels)
        want = O.block_gain_apply(img, gmap)
        assert np.array_equal(want, CE.saturate(CE.products(img, CE.interp_gains(gmap, w, h)))), (w, h, gw, gh)
        assert np.array_equal(want, CE.stale_row_table(img, gmap)) == (not h > CE.GAIN_ROWS_WG >= w), (w, h)
    fw, fh, gw, gh = CE.SUB_FULL
    img, gmap = CE.geometry(fw, fh, gw, gh, channels)
    want = O.block_gain_apply(img, gmap)
    for x0, y0, w, h in CE.SUB_RECTS:
        cut = img[y0:y0 + h, x0:x0 + w]
        assert np.array_equal(CE.saturate(CE.products(cut, CE.interp_gains(gmap, w, h, (fw, fh, x0, y0)))), want[y0:y0 + h, x0:x0 + w])
    imgs, maps, f = CE.unbounded_in_second_launch()
    assert f["bounded"] == [bool(np.abs(m).max() < CE.BOUNDED_BELOW) for m in maps] and f["bounded"].index(False) >= CE.GAIN_BATCH
