"""The constructed resize families (tests/constructed_resizes.py) without a GPU: the numpy contract (tests/numpy_resize.py) equals the
CPU oracle on all of them, every family's stated facts hold, `expected_path` reaches each of its six answers, the constants it rests on
are the sources' own, and the LDS window the one-launch kernel stages fits the host's bound over a sweep of sizes and tile starts.

The variants below restate the contract with ONE mistake each, of the kind a kernel can carry unnoticed; they are numpy only and never
imported by the product.  For every variant at least one family gives a result that differs from the contract's, and every family
tells at least one variant: the evidence that tests/test_gpu_constructed_resizes.py would fail on such a kernel.

Three mistakes one might list change no byte and therefore have no variant here: `o + 1` not clamped to the last column or row (its
weight is 0 wherever the clamp acts: it is a question of reading past the image, which the 0xff frames of view_offsets and the
unchanged-parent checks on the device look at), the interior flag ignored on the last row (with coeff1 = 0 the blend
(h0 * 256 + 2^15) >> 16 is the edge form (h0 + 128) >> 8), and a tail that writes or keeps a byte too many (it lands in row padding);
a tail that is a byte SHORT is visible and stands in for it.  Nothing here provokes a fault: these are host computations."""
import math
import os
import re

import numpy as np
import pytest

from tests import constructed_resizes as CR
from tests import numpy_resize as NR

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "stitching_amd", "csrc")


def _text(source):
    return open(os.path.join(CSRC, source)).read()


def _constexpr(source, name):
    """the value of NAME in `constexpr int ... NAME = <integer or product of integers and earlier names> [,;]` of a source"""
    m = re.search(r"constexpr\s+int\s+(?:[^;]*?,\s*)?%s\s*=\s*([^;,]+)[;,]" % name, _text(source))
    assert m, (source, name)
    value = 1
    for factor in m.group(1).split("*"):
        factor = factor.strip()
        value *= int(factor) if factor.isdigit() else _constexpr(source, factor)
    return value


def test_the_sources_constants_are_the_ones_expected_path_rests_on():
    hip, host = "stx_resize.hip", "stx_resize_host.cpp"
    assert (CR.SEAM1_COLS, CR.SEAM1_ROWS) == (_constexpr(hip, "SEAM1_COLS"), _constexpr(hip, "SEAM1_ROWS")) == (8, 8)
    assert (CR.TILE_W, CR.TILE_H) == (_constexpr(hip, "SEAM1_TW"), _constexpr(hip, "SEAM1_TH")) == (512, 32)
    assert CR.SEAM_BATCH == _constexpr(hip, "SEAM_BATCH") == 16 and CR.SEAM_ROWS == _constexpr(hip, "SEAM_ROWS") == 16
    assert (CR.RESIZE_TW, CR.RESIZE_TH) == (_constexpr("stx_internal.h", "STX_RESIZE_TW"), _constexpr("stx_internal.h", "STX_RESIZE_TH"))
    m = re.search(r"lds\s*>\s*\((\d+)u\s*<<\s*(\d+)\)", _text(hip))
    assert m and int(m.group(1)) << int(m.group(2)) == CR.LDS_BUDGET
    # the window bound, the alignment tests and the pitch of the library's own images, as the host writes them
    assert "std::min(seams[i]->w, (int)std::ceil(SEAM1_TW * xs) + 3) + 2" in _text(hip)
    assert "std::min(seams[i]->h, (int)std::ceil(SEAM1_TH * ys) + 3)" in _text(hip)
    assert "((uintptr_t)m->ptr & 7) || (m->stride & 7) || w8 > m->stride" in _text(hip)
    assert "((uintptr_t)m->ptr & 3) == 0 && (m->stride & 3) == 0 && (size_t)((m->w + 3) & ~3) <= m->stride" in _text(host)
    m = re.search(r"b->stride = align_up\(align_up\(\(size_t\)w, (\d+)\) \* c \* stx_elem_bytes\(elem\), (\d+)\);", _text("stx_image_host.cpp"))
    assert m and (int(m.group(1)), int(m.group(2))) == (8, CR.BUF_PITCH)
    assert [CR.buf_pitch(w) for w in (1, 8, 57, 64, 65)] == [64, 64, 64, 64, 128] and CR.buf_pitch(22, 3) == 128
    # the shapes lie around them
    assert set(CR.CHUNK_COUNTS) == {CR.SEAM_BATCH, CR.SEAM_BATCH + 1, 2 * CR.SEAM_BATCH + 1}
    assert {w % 4 for w in CR.VIEW_WIDTHS} == {0, 1, 2, 3} and {w % 8 for w in CR.VIEW_WIDTHS} == set(range(8))
    assert {h > CR.SEAM1_ROWS for h in CR.VIEW_HEIGHTS} == {h > 4 * CR.SEAM_ROWS for h in CR.VIEW_HEIGHTS} == {False, True}


# ---------------------------------------------------------------------------------------------------------------------------------
# the contract equals the oracle
# ---------------------------------------------------------------------------------------------------------------------------------
def _oracle_case(oracle, c):
    out = []
    for i, (low, f) in enumerate(zip(c["lows"], c["finals"])):
        if c["sub"] is None:
            out.append(oracle.seam_resize(low, f.array))
        else:  # the rectangle of the whole result: the final mask outside the rectangle does not matter
            fw, fh, x0, y0 = c["sub"][i]
            full = np.zeros((fh, fw), np.uint8)
            full[y0:y0 + f.h, x0:x0 + f.w] = f.array
            out.append(oracle.seam_resize(low, full)[y0:y0 + f.h, x0:x0 + f.w])
    return out


def _differing(a, b):
    assert len(a) == len(b) and all(x.shape == y.shape and x.dtype == y.dtype for x, y in zip(a, b))
    return sum(int(np.count_nonzero(x != y)) for x, y in zip(a, b))


@pytest.mark.parametrize("family", sorted(CR.SEAM_FAMILIES))
def test_contract_equals_the_oracle_on_every_seam_family(oracle, family):
    for c in CR.SEAM_FAMILIES[family]():
        assert _differing(CR.want(c), _oracle_case(oracle, c)) == 0, c["name"]
        for low in c["lows"]:
            assert np.array_equal(NR.dilate3x3(low), oracle.dilate3x3(low))


def test_contract_equals_the_oracle_on_the_image_families(oracle):
    for name, srcs, sizes, _ in CR.image_batches():
        for s, size in zip(srcs, sizes):
            a = CR.source_array(s)
            assert np.array_equal(NR.resize_linear_exact(a, size), oracle.resize_linear_exact(a, size)), (name, a.shape, size)
    for kind in ("ties", "knife_edges"):
        for src_n, dst_n, col, axis in CR.coefficient_cases(kind):
            for ch in (1, 3):
                img, size = CR.coefficient_image(src_n, dst_n, col, axis, ch)
                assert np.array_equal(NR.resize_linear_exact(img, size), oracle.resize_linear_exact(img, size))


def test_contract_on_the_known_answers(oracle):
    """the known answers of test_next_rows.py"""
    a = (np.arange(12).reshape(3, 4) * 20).astype(np.uint8)
    assert np.array_equal(NR.resize_linear_exact(a, (4, 3)), a)
    assert NR.resize_linear_exact(a, (8, 3))[0].tolist() == [0, 5, 15, 25, 35, 45, 55, 60]
    assert NR.resize_linear_exact(a, (2, 2)).tolist() == [[30, 70], [150, 190]]
    assert NR.resize_linear_exact(np.array([[7]], np.uint8), (3, 2)).tolist() == [[7, 7, 7], [7, 7, 7]]
    assert (NR.resize_linear_exact(np.full((5, 7, 3), 200, np.uint8), (13, 9)) == 200).all()
    m = np.zeros((5, 5), np.uint8)
    m[2, 2] = 255
    d = NR.dilate3x3(m)
    assert d[1:4, 1:4].all() and d.sum() == 9 * 255 and np.array_equal(d, oracle.dilate3x3(m))
    for size in ((4, 3), (8, 3), (2, 2), (13, 9), (1, 1)):
        assert np.array_equal(NR.resize_linear_exact(a, size), oracle.resize_linear_exact(a, size))


# ---------------------------------------------------------------------------------------------------------------------------------
# facts and paths
# ---------------------------------------------------------------------------------------------------------------------------------
def test_every_path_is_reached_and_every_family_states_its_path():
    reached = {}
    for family, make in CR.SEAM_FAMILIES.items():
        for c in make():
            p = CR.expected_path(c)
            assert p == c["facts"]["path"], (c["name"], p)
            assert sum(CR.expected_counts(c)) == len(c["lows"])
            reached.setdefault(p, set()).add(family)
            for f in c["finals"]:  # destinations stay small
                assert f.w * f.h <= 4096 * 64 + 4096 and min(f.w, f.h) <= 80 and max(f.w, f.h) <= 4096, c["name"]
    assert set(reached) == set(CR.PATHS)
    assert reached["per_image_fallback"] == reached["aligned_copy_then_lds"] == {"view_offsets"}
    assert {"batch_chunks", "sub_tables", "lds_budget", "ties", "knife_edges"} <= reached["tables_batch"]
    assert {"ties", "knife_edges", "borders", "view_offsets"} <= reached["single_4px"] & reached["single_1px"]


def test_view_offsets_facts():
    cases = CR.view_offsets()
    singles = [c for c in cases if not c["batch"]]
    assert {(c["facts"]["x0"], c["facts"]["width"]) for c in singles} == {(x, w) for xs in CR.VIEW_X0.values() for x in xs for w in CR.VIEW_WIDTHS}
    for c in cases:
        for f in c["finals"]:
            if not f.whole:  # everything outside the view is 0xff, and there is something to its right and below it
                outside = np.ones(f.parent.shape, bool)
                outside[f.y:f.y + f.h, f.x:f.x + f.w] = False
                assert (f.parent[outside] == 0xff).all() and f.parent.shape[1] > f.x + f.w and f.parent.shape[0] > f.y + f.h
                assert (f.array != 0xff).any()
    mixed = next(c for c in cases if c["name"] == "one odd view among aligned")
    assert CR.image_paths(mixed) == mixed["facts"]["image_paths"] and CR.expected_counts(mixed) == [4, 0, 0, 1]
    assert all(CR.expected_path(CR.single(mixed, i)) == p for i, p in enumerate(mixed["facts"]["image_paths"]))
    # in a batch of odd views every image takes the per-pixel kernel; with sub all are copied and take the LDS kernel
    odd = next(c for c in cases if c["name"] == "views x0=5 batch")
    assert CR.expected_counts(odd) == [0, 0, 0, len(CR.VIEW_WIDTHS)]
    assert CR.expected_counts(next(c for c in cases if c["name"] == "views x0=5 batch sub")) == [len(CR.VIEW_WIDTHS), 0, 0, 0]


def test_lds_budget_facts():
    cases = CR.lds_budget()
    by = {c["name"]: c for c in cases}
    assert by["budget 700x50->350x25"]["facts"]["lds_bytes"] == (52 + 50) * 704 > CR.LDS_BUDGET
    assert by["budget 520x40->520x40"]["facts"]["lds_bytes"] == (37 + 35) * 520 <= CR.LDS_BUDGET
    fits, over = CR.budget_edge()
    assert over == fits - 1 < 700
    assert by[f"budget 700x40->{fits}x40"]["facts"]["lds_bytes"] <= CR.LDS_BUDGET < by[f"budget 700x40->{over}x40"]["facts"]["lds_bytes"]
    for c in cases:
        assert c["facts"]["lds_bytes"] == CR.lds_bytes(c)
        if c["batch"]:  # the other images of the batch would fit on their own
            assert c["facts"]["lds_bytes"] > CR.LDS_BUDGET
            assert any(CR.expected_path(CR.single(c, i)) == "lds" for i in range(len(c["lows"])))


def test_window_reach_facts():
    cases = CR.window_reach()
    by = {c["name"]: c["facts"] for c in cases}
    assert by["reach cols 60->166"]["window"] == by["reach cols 60->166"]["bound"] == 60
    for c in cases[:-1]:
        f, (low,), (fin,) = c["facts"], c["lows"], c["finals"]
        src_n, dst_n = (low.shape[1], fin.w) if f["axis"] == "x" else (low.shape[0], fin.h)
        tile, step = (CR.TILE_W, 4) if f["axis"] == "x" else (CR.TILE_H, 1)
        got, _, bound = CR.reach(src_n, dst_n, tile, step)
        assert (got, bound) == (f["window"], f["bound"]) and got <= bound
    assert sum(c["facts"]["window"] == c["facts"]["bound"] for c in cases[:-1]) >= 8
    assert {c["facts"]["bound"] - c["facts"]["window"] for c in cases[:-1] if "tiles" in c["name"]} == {1}
    assert cases[-1]["facts"]["phases"] == len(cases[-1]["lows"]) == 12  # twelve rectangles, twelve different (x, y) phases


def test_batch_chunks_and_sub_tables_facts():
    for c in CR.batch_chunks():
        f = c["facts"]
        assert len(c["lows"]) == f["n"] and f["chunks"] == (1 if f["n"] == CR.SEAM_BATCH else f["n"] // CR.SEAM_BATCH + 1)
        assert (f["largest"] >= CR.SEAM_BATCH) == (f["n"] > CR.SEAM_BATCH)
        sizes = [(x.w, x.h) for x in c["finals"]]
        assert len(set(sizes)) > len(sizes) // 2
        assert any(w > CR.TILE_W and h > CR.TILE_H for w, h in sizes) and any(w < 256 and h < CR.TILE_H for w, h in sizes)
        # a chunk indexed from 0 instead of `base` shows in the largest image, the first of the second chunk
        good, bad = CR.want(c), _without_base(c)
        assert (f["n"] > CR.SEAM_BATCH) == (not np.array_equal(good[f["largest"]], bad[f["largest"]])) == (_differing(good, bad) > 0)
    views, over = CR.sub_tables()
    assert {q[2] for q in views["sub"]} >= {0, 4, 52} and {q[3] for q in views["sub"]} >= {0, 1, views["sub"][0][1] - 1}
    assert all(f.w % 4 for f in views["finals"][:-1]) and all(f.x == 4 for f in views["finals"])
    k = views["facts"]["ends_on_corner"]
    fw, fh, x0, y0 = views["sub"][k]
    assert (x0 + views["finals"][k].w, y0 + views["finals"][k].h) == (fw, fh)
    assert all(f.whole for f in over["finals"]) and over["facts"]["lds_bytes"] > CR.LDS_BUDGET


def test_borders_facts():
    for c in CR.borders():
        (low,), f = c["lows"], c["facts"]
        if "dilated" in f:
            want = np.zeros_like(low)
            want[f["dilated"]] = 255
            assert np.array_equal(NR.dilate3x3(low), want) and np.count_nonzero(low) == 1
        if f.get("all_255"):
            assert (NR.dilate3x3(low) == 255).all() and (low == 0).sum() == 1
        if "values" in f:
            assert set(np.unique(CR.want(c)[0]).tolist()) == f["values"]
    shapes = {(c["lows"][0].shape, (c["finals"][0].h, c["finals"][0].w)) for c in CR.borders()}
    assert {s for s, _ in shapes} >= {(1, 7), (7, 1), (1, 1), (2, 2)} and ((5, 6), (1, 1)) in shapes


def test_ties_and_knife_edges_facts():
    assert len(CR.tie_columns(2, 512)) == 512 - 2 * 128  # every interior column of 2 -> 512
    assert [len(CR.tie_columns(s, d)) > 0 for s, d in CR.TIES] == [True] * len(CR.TIES)
    for s, d, col in CR.KNIVES:
        assert col in CR.knife_columns(s, d), (s, d, col)
    more = CR.more_knives()
    assert len(more) == 3 and not set(more) & set(CR.KNIVES)
    for s, d, col in list(CR.KNIVES) + more:  # one fused operation changes the weight by one 256th; half-up rounding does too
        a, b = NR.coeff(col, s, d), CR.fused_coeff(col, s, d)
        assert a[0] == b[0] and abs(a[1] - b[1]) == 1, (s, d, col)
    for kind, other in (("ties", CR.half_up_coeff), ("knife_edges", CR.fused_coeff)):
        for src_n, dst_n, col, axis in CR.coefficient_cases(kind):
            for ch in (1, 3):  # the image: the named column (row) lies between a 0 and a 255 and its byte tells the two evaluations apart
                img, size = CR.coefficient_image(src_n, dst_n, col, axis, ch)
                good = NR.resize_linear_exact(img, size)
                cx = NR.coeffs(img.shape[1], size[0], one=other if axis == "x" else NR.coeff)
                cy = NR.coeffs(img.shape[0], size[1], one=other if axis == "y" else NR.coeff)
                bad = NR.resize_with(img, cx, cy)
                line = (good != bad).reshape(good.shape[0], good.shape[1], -1).any(axis=2)
                assert (line[2, col] if axis == "x" else line[col, 2]), (kind, src_n, dst_n, col, axis)
        for c in CR.coefficient_masks(kind):
            f = c["facts"]
            assert f["visible"] == (f["src"] >= 3)
            if f["visible"]:
                assert not np.array_equal(CR.want(c)[0], _with_coeff(other)(c["lows"][0], c["finals"][0].array)), c["name"]


# ---------------------------------------------------------------------------------------------------------------------------------
# the variants: one mistake each
# ---------------------------------------------------------------------------------------------------------------------------------
def _pieces(low, final, sub):
    h, w = final.shape
    fw, fh, x0, y0 = (w, h, 0, 0) if sub is None else sub
    return np.asarray(low, np.uint8), w, h, fw, fh, x0, y0


def _with_coeff(one):
    def f(low, final, sub=None):
        low, w, h, fw, fh, x0, y0 = _pieces(low, final, sub)
        return NR.resize_with(NR.dilate3x3(low), NR.coeffs(low.shape[1], fw, x0, w, one=one), NR.coeffs(low.shape[0], fh, y0, h, one=one)) & final
    return f


def _with_dilate(dilate):
    def f(low, final, sub=None):
        low, w, h, fw, fh, x0, y0 = _pieces(low, final, sub)
        return NR.resize_with(dilate(low), NR.coeffs(low.shape[1], fw, x0, w), NR.coeffs(low.shape[0], fh, y0, h)) & final
    return f


def _dilate_outside_255(m):
    h, w = m.shape
    p = np.pad(m, 1, constant_values=255)
    return np.max([p[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)], axis=0)


def _dilate_wrapping(m):
    """x - 1 and x + 1 taken in the flat array: the row's end reads the next row's start"""
    h, w = m.shape
    flat = np.concatenate(([0], m.ravel(), [0]))
    rows = np.maximum(np.maximum(flat[:-2], flat[1:-1]), flat[2:]).reshape(h, w)
    p = np.pad(rows, ((1, 1), (0, 0)))
    return np.maximum(np.maximum(p[:-2], p[1:-1]), p[2:])


def _dilate_after(low, final, sub=None):
    low, w, h, fw, fh, x0, y0 = _pieces(low, final, sub)
    full = NR.dilate3x3(NR.resize_linear_exact(low, (fw, fh)))
    return full[y0:y0 + h, x0:x0 + w] & final


def _with_and(op):
    return lambda low, final, sub=None: op(NR.seam_resize(low, np.full(final.shape, 255, np.uint8), sub), final)


def _sub_dropped(low, final, sub=None):
    return NR.seam_resize(low, final, None if sub is None else (sub[0], sub[1], 0, 0))


def _sub_on_source(low, final, sub=None):
    """the rectangle's offset added to the source offsets instead of the destination index"""
    low, w, h, fw, fh, x0, y0 = _pieces(low, final, sub)
    cx, cy = NR.coeffs(low.shape[1], fw, 0, w), NR.coeffs(low.shape[0], fh, 0, h)
    cx = (np.minimum(cx[0] + x0, low.shape[1] - 1),) + cx[1:]
    cy = (np.minimum(cy[0] + y0, low.shape[0] - 1),) + cy[1:]
    return NR.resize_with(NR.dilate3x3(low), cx, cy) & final


def _tail_short(low, final, sub=None):
    """the last byte of a row whose width is no multiple of 4 is not written"""
    r = NR.seam_resize(low, final, sub)
    if r.shape[1] % 4:
        r[:, -1] = 0
    return r


def _without_base(c):
    """image i of a batch served with the low mask of image i mod 16"""
    lows = [c["lows"][i % CR.SEAM_BATCH] for i in range(len(c["lows"]))]
    return CR.want(dict(c, lows=lows))


VARIANTS = {
    "half_up": _with_coeff(CR.half_up_coeff),
    "fused": _with_coeff(CR.fused_coeff),
    "dilate_outside_255": _with_dilate(_dilate_outside_255),
    "dilate_wraps": _with_dilate(_dilate_wrapping),
    "dilate_after": _dilate_after,
    "min_for_and": _with_and(np.minimum),
    "logical_and": _with_and(lambda r, m: np.where(m != 0, r, 0).astype(np.uint8)),
    "sub_dropped": _sub_dropped,
    "sub_on_source": _sub_on_source,
    "tail_short": _tail_short,
}


def test_every_variant_is_told_by_a_family_and_every_family_tells_one():
    told = {v: set() for v in list(VARIANTS) + ["without_base"]}
    for family, make in CR.SEAM_FAMILIES.items():
        for c in make():
            good = CR.want(c)
            for name, fn in VARIANTS.items():
                if family not in told[name] and _differing(good, CR.want(c, fn)):
                    told[name].add(family)
            if _differing(good, _without_base(c)):
                told["without_base"].add(family)
    assert all(told.values()), told
    assert set().union(*told.values()) == set(CR.SEAM_FAMILIES)
    assert "ties" in told["half_up"] and "knife_edges" in told["fused"] and "borders" in told["dilate_outside_255"] & told["dilate_wraps"]
    assert told["without_base"] == {"batch_chunks"}  # no other family passes more than 16 masks
    assert {"sub_tables", "view_offsets", "window_reach"} <= told["sub_dropped"] & told["sub_on_source"]
    assert "borders" in told["min_for_and"] & told["logical_and"] and "view_offsets" in told["tail_short"]
    # the sizes the suite had (random masks enlarged 5 .. 40 times) do not land on the ties: neither rounding nor contraction shows
    rng = np.random.default_rng(17)
    for (sw, sh), (dw, dh) in (((73, 54), (803, 601)), ((91, 68), (640, 480)), ((10, 133), (97, 1201)), ((240, 7), (1200, 37))):
        low, fin = CR.low_mask(rng, sh, sw), np.full((dh, dw), 255, np.uint8)
        assert np.array_equal(VARIANTS["fused"](low, fin), NR.seam_resize(low, fin)), (sw, dw)


# ---------------------------------------------------------------------------------------------------------------------------------
# the LDS window fits the host's bound
# ---------------------------------------------------------------------------------------------------------------------------------
def _offsets(src_n, dst_n):
    """numpy_resize.coeff's offsets for a whole axis at once (the same two roundings per index)"""
    scale = 1.0 / (float(dst_n) / float(src_n))
    f = scale * (np.arange(dst_n, dtype=np.float64) + 0.5) - 0.5
    return np.clip(np.floor(f).astype(np.int64), 0, src_n - 1)


def test_window_bound_sweep():
    """Every source size 1 .. 700, destinations 1 .. 6000 (the integer factors up to 40 and the integer reductions up to 8, each +-1,
    and a seeded sample) and every tile start (columns: multiples of 4 — tile starts are multiples of 512 plus a rectangle's x0; rows:
    any): the window the kernel stages is never larger than min(src, ceil(tile * scale) + 3).  The bound is attained: wherever one tile
    spans the whole source the window IS the source and the `min` holds — 60 -> 166 is named — so the clamp cannot be loosened to
    anything smaller.  Where the ceil side holds, the widest window leaves exactly one column spare."""
    rng = np.random.default_rng(0)
    for src_n, dst_n in ((1, 1), (1, 9), (2, 512), (3, 1280), (60, 166), (700, 350), (13, 6000)):
        assert _offsets(src_n, dst_n).tolist() == [NR.coeff(v, src_n, dst_n)[0] for v in range(dst_n)]
    for tile, step in ((CR.TILE_W, 4), (CR.TILE_H, 1)):
        least, least_ceil, named = None, None, None
        for src_n in range(1, 701):
            dsts = {k * src_n + d for k in range(1, 41) for d in (-1, 0, 1)} | {src_n // k + d for k in range(2, 9) for d in (-1, 0, 1)}
            dsts |= {int(v) for v in rng.integers(1, 6001, 8)} | ({166} if src_n == 60 else set())
            for dst_n in sorted(d for d in dsts if 1 <= d <= 6000):
                o = _offsets(src_n, dst_n)
                first = np.arange(0, dst_n, step)
                last = np.minimum(first + tile, dst_n) - 1
                window = np.minimum(o[last] + 1, src_n - 1) - o[first] + 1
                k = int(np.argmax(window))
                bound = CR.window_bound(src_n, dst_n, tile)
                margin = bound - int(window[k])
                assert margin >= 0, (tile, src_n, dst_n, int(first[k]))
                if bound < src_n and (least_ceil is None or margin < least_ceil[0]):
                    least_ceil = (margin, src_n, dst_n, int(first[k]))
                if least is None or margin < least[0]:
                    least = (margin, src_n, dst_n, int(first[k]))
                if (src_n, dst_n) == (60, 166):
                    named = (margin, int(window[k]), bound)
        assert least[0] == 0, least
        assert named == (0, 60, 60) if tile == CR.TILE_W else named == (1, 14, 15)
        assert least_ceil[0] == 1, least_ceil
    # the same through the kernel's own restatement, one index at a time
    assert CR.reach(60, 166, CR.TILE_W, 4) == (60, 0, 60)
    assert CR.tile_window(7, 1544, 264, CR.TILE_W) == 5 and CR.window_bound(7, 1544, CR.TILE_W) == 6
    assert math.ceil(CR.TILE_W * (1.0 / (166.0 / 60.0))) + 3 == 189
