"""pyrUp in the packed lanes of the gathers combines the three window rows before it filters the columns (up_patch_pk_math and
up_patch_pks_math of csrc/stx_blend_fast.hip).  This file restates the two helpers in numpy as the device runs them — 32-bit registers,
v_perm_b32 / v_alignbit_b32 on them, and wrapping 16-bit arithmetic with one array element per register half — and compares every output
with the int32 pyrUp of tests/numpy_blenders.py on windows at every edge, at the value extremes and at the +-500 limit of the int16 form.
The selectors are read from the source, so a changed selector is tested, not a remembered one.  No GPU."""
import os
import re

import numpy as np
import pytest

from tests import numpy_blenders as NB

SRC = open(os.path.join(os.path.dirname(__file__), "..", "stitching_amd", "csrc", "stx_blend_fast.hip")).read()
TAP_LIMIT = 500


def _body(name):
    return SRC[SRC.index(name):SRC.index("return s;", SRC.index(name))]


def _selectors(fn):
    """up_sel / up_sel_u8 -> {(left, right): (a0, a2)} from the source text"""
    body = _body("STX_DEV UpSel %s(bool left_edge, bool right_edge)" % fn)
    a0 = re.search(r"s\.a0 = left_edge \? (0x[0-9a-f]+)u : (0x[0-9a-f]+)u;", body)
    a2 = re.search(r"s\.a2 = right_edge \? (0x[0-9a-f]+)u : (0x[0-9a-f]+)u;", body)
    return {(l, r): (int(a0.group(1 if l else 2), 16), int(a2.group(1 if r else 2), 16)) for l in (False, True) for r in (False, True)}


SEL_U8, SEL_S16 = _selectors("up_sel_u8"), _selectors("up_sel")
A1_U8 = 0x0c020c01  # the middle pair register of a byte window: perm(d1, d1)


# ---------------------------------------------------------------------------------------------------------------------------------
# the device's operations on uint32 arrays (one element per lane) and on (..., 2) 16-bit arrays (one element per register half)
# ---------------------------------------------------------------------------------------------------------------------------------
def perm(hi, lo, sel):
    """v_perm_b32: selector byte i picks byte 0 .. 3 of `lo`, 4 .. 7 of `hi`, 0x0c gives 0"""
    src = [(lo >> np.uint32(8 * i)) & np.uint32(255) for i in range(4)] + [(hi >> np.uint32(8 * i)) & np.uint32(255) for i in range(4)]
    out = np.zeros_like(lo)
    for i in range(4):
        s = (sel >> (8 * i)) & 255
        assert s < 8 or s == 0x0c
        if s < 8:
            out |= src[s] << np.uint32(8 * i)
    return out


def alignbit16(hi, lo):
    """v_alignbit_b32(hi, lo, 16)"""
    return (lo >> np.uint32(16)) | (hi << np.uint32(16))


def halves(reg, dtype):
    return np.stack([reg & np.uint32(0xffff), reg >> np.uint32(16)], -1).astype(np.uint16).view(dtype)


def between(hi, lo):
    """up_between on halves: (lo's high half, hi's low half)"""
    return np.stack([lo[..., 1], hi[..., 0]], -1)


def columns(e, o, dtype):
    """up_patch_columns: -> up[2][4] as (N, 2, 4, 2), and the largest |intermediate| of the unwrapped sums"""
    k = lambda v: dtype(v)
    eB, oB = [between(e[1], e[0]), between(e[2], e[1])], [between(o[1], o[0]), between(o[2], o[1])]
    up = [[None] * 4, [None] * 4]
    wide = []
    for q in range(2):
        he, ho = e[q] + eB[q] * k(6) + e[q + 1], eB[q] + e[q + 1]
        hv, hq = o[q] + oB[q] * k(6) + o[q + 1], oB[q] + o[q + 1]
        wide.append(np.abs(e[q].astype(np.int64) + 6 * eB[q].astype(np.int64) + e[q + 1].astype(np.int64)).max())
        assert he.dtype == dtype and ho.dtype == dtype
        up[0][q], up[0][2 + q], up[1][q], up[1][2 + q] = he >> k(6), ho >> k(4), hv >> k(4), hq >> k(2)
    return np.stack([np.stack(r, 1) for r in up], 1), max(wide)


def rows_first(A, dtype):
    """the vertical stage on the pair registers A[row][j] (halves) -> VE[j], VO[j] with the rounding constants folded in"""
    k = lambda v: dtype(v)
    e = [A[1][j] * k(6) + A[0][j] + A[2][j] + k(4) for j in range(3)]
    o = [A[1][j] + A[2][j] + k(1) for j in range(3)]
    return e, o


def up_patch_pk_math(w, sel):
    """w[row][dword]: uint32 arrays, the 12-byte windows plane[cx - 4 .. cx + 7] -> (up (N, 2, 4, 2) uint16, max VE, max HE(VE))"""
    A = [[halves(perm(w[r][1], w[r][0], sel[0]), np.uint16), halves(perm(w[r][1], w[r][1], A1_U8), np.uint16),
          halves(perm(w[r][2], w[r][1], sel[1]), np.uint16)] for r in range(3)]
    e, o = rows_first(A, np.uint16)
    up, he = columns(e, o, np.uint16)
    return up, max(int(v.max()) for v in e), int(he)


def up_patch_pks_math(w, sel):
    """w[row][dword]: the 16-byte windows (x,c0) (c1,c2) (c3,c4) (c5,x) -> (accepted (N,), up (N, 2, 4, 2) int16, max |VE|, max |HE(VE)|)"""
    regs = [[perm(w[r][1], w[r][0], sel[0]), alignbit16(w[r][2], w[r][1]), perm(w[r][3], w[r][2], sel[1])] for r in range(3)]
    worst = np.zeros(regs[0][0].shape + (2,), np.uint16)
    for r in range(3):
        for j in range(3):
            worst = np.maximum(worst, halves(regs[r][j], np.uint16) + np.uint16(TAP_LIMIT))
    ok = (np.minimum(worst, np.uint16(2 * TAP_LIMIT)) == worst).all(axis=-1)
    A = [[halves(regs[r][j], np.int16) for j in range(3)] for r in range(3)]
    e, o = rows_first(A, np.int16)
    up, he = columns(e, o, np.int16)
    return ok, up, max(int(np.abs(v.astype(np.int64)).max()) for v in e), int(he)


def pixels(up):
    """(N, 2, 4, 2) in the pair order (0,2) (4,6) (1,3) (5,7) -> (N, 2, 8)"""
    out = np.zeros(up.shape[:2] + (8,), np.int64)
    for q, (a, b) in enumerate(((0, 2), (4, 6), (1, 3), (5, 7))):
        out[:, :, a], out[:, :, b] = up[:, :, q, 0], up[:, :, q, 1]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# windows of a coarse plane as the loads return them
# ---------------------------------------------------------------------------------------------------------------------------------
def up_idx_s(i, n):
    return min(abs(i), n - 1)


def lanes_of(plane):
    """every 8 x 2 patch of pyrUp(plane): [(cx, cy)], cx a multiple of 4"""
    ch, cw = plane.shape
    assert cw % 4 == 0
    return [(cx, cy) for cy in range(ch) for cx in range(0, cw, 4)]


def windows(plane, junk):
    """plane (ch, cw) u8 or int16 -> (w[row][dword] uint32 over the lanes, left (N,), right (N,)): the three rows by the row rule, each
    read from 4 bytes in front of sample cx (u8: 12 bytes, int16: 16 bytes) out of rows padded with `junk` in front and behind"""
    ch, cw = plane.shape
    pad = np.concatenate([junk[:, :8].astype(plane.dtype), plane, junk[:, 8:24].astype(plane.dtype)], axis=1)
    raw = np.ascontiguousarray(pad).view(np.uint8).reshape(ch, -1)
    size, nd = plane.dtype.itemsize, 3 if plane.dtype == np.uint8 else 4
    w = [[[] for _ in range(nd)] for _ in range(3)]
    for cx, cy in lanes_of(plane):
        for r, row in enumerate((up_idx_s(cy - 1, ch), cy, up_idx_s(cy + 1, ch))):
            start = (8 + cx) * size - 4
            d = raw[row, start:start + 4 * nd].copy().view("<u4")
            for i in range(nd):
                w[r][i].append(d[i])
    cxs = np.array([cx for cx, _ in lanes_of(plane)])
    return [[np.array(v, np.uint32) for v in row] for row in w], cxs == 0, cxs + 4 >= cw


def reference(plane):
    """the int32 pyrUp of tests/numpy_blenders.py, per lane (N, 2, 8)"""
    up = NB.pyr_up_16s(plane.astype(np.int16)).astype(np.int64)
    return np.stack([up[2 * cy:2 * cy + 2, 2 * cx:2 * cx + 8] for cx, cy in lanes_of(plane)])


def run_u8(plane, junk):
    w, left, right = windows(plane, junk)
    out = np.zeros((len(left), 2, 8), np.int64)
    ve = he = 0
    for key, sel in SEL_U8.items():
        m = (left == key[0]) & (right == key[1])
        if m.any():
            up, a, b = up_patch_pk_math([[d[m] for d in row] for row in w], sel)
            out[m], ve, he = pixels(up), max(ve, a), max(he, b)
    return out, ve, he


def run_s16(plane, junk):
    w, left, right = windows(plane, junk)
    out, ok = np.zeros((len(left), 2, 8), np.int64), np.zeros(len(left), bool)
    ve = he = 0
    for key, sel in SEL_S16.items():
        m = (left == key[0]) & (right == key[1])
        if m.any():
            good, up, a, b = up_patch_pks_math([[d[m] for d in row] for row in w], sel)
            out[m], ok[m], ve, he = pixels(up), good, max(ve, a), max(he, b)
    return ok, out, ve, he


# coarse sizes: 4 columns = one lane that is the first and the last of its row; 8 = a left and a right lane; 12, 20 = lanes at neither edge;
# heights 1, 2 (the row clamp) and odd ones
SHAPES = [(1, 4), (2, 4), (3, 4), (1, 8), (2, 8), (5, 8), (1, 12), (2, 12), (7, 20)]


def _junk(ch, dtype, seed=1):
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        return rng.integers(0, 256, (ch, 24)).astype(np.uint8)
    return rng.choice(np.array([-32768, -20000, 20000, 32767], np.int16), (ch, 24))


def test_the_selectors_cover_every_edge_combination():
    combos = set()
    for ch, cw in SHAPES:
        _, left, right = windows(np.zeros((ch, cw), np.uint8), _junk(ch, np.uint8))
        combos |= set(zip(left.tolist(), right.tolist()))
    assert combos == {(False, False), (True, False), (False, True), (True, True)}
    assert len(set(SEL_U8.values())) == 4 and len(set(SEL_S16.values())) == 4


@pytest.mark.parametrize("ch,cw", SHAPES)
@pytest.mark.parametrize("fill", ("zeros", "full", "columns", "rows", "checker", "random", "random_extremes"))
def test_u8_windows_equal_the_int32_pyrup(ch, cw, fill):
    rng = np.random.default_rng(ch * 100 + cw)
    yy, xx = np.mgrid[0:ch, 0:cw]
    plane = {"zeros": np.zeros((ch, cw)), "full": np.full((ch, cw), 255), "columns": 255 * (xx & 1), "rows": 255 * (yy & 1),
             "checker": 255 * ((xx + yy) & 1), "random": rng.integers(0, 256, (ch, cw)),
             "random_extremes": rng.choice([0, 255], (ch, cw))}[fill].astype(np.uint8)
    for seed in (1, 2):  # what lies in front of and behind a row must not matter
        got, ve, he = run_u8(plane, _junk(ch, np.uint8, seed))
        assert np.array_equal(got, reference(plane))
        assert ve <= 8 * 255 + 4 and he <= 64 * 255 + 32


def test_u8_bounds_are_reached_by_the_all_255_window_and_fit_an_unsigned_half():
    got, ve, he = run_u8(np.full((3, 12), 255, np.uint8), _junk(3, np.uint8))
    assert (ve, he) == (8 * 255 + 4, 64 * 255 + 32) and he == 16352 and he < 1 << 16
    assert (got == 255).all()


@pytest.mark.parametrize("ch,cw", SHAPES)
@pytest.mark.parametrize("fill", ("zeros", "plus", "minus", "columns", "rows", "checker", "random", "random_extremes"))
def test_int16_windows_within_the_limit_equal_the_int32_pyrup(ch, cw, fill):
    rng = np.random.default_rng(ch * 100 + cw + 7)
    yy, xx = np.mgrid[0:ch, 0:cw]
    L = TAP_LIMIT
    plane = {"zeros": np.zeros((ch, cw)), "plus": np.full((ch, cw), L), "minus": np.full((ch, cw), -L), "columns": L - 2 * L * (xx & 1),
             "rows": L - 2 * L * (yy & 1), "checker": L - 2 * L * ((xx + yy) & 1), "random": rng.integers(-L, L + 1, (ch, cw)),
             "random_extremes": rng.choice([-L, L], (ch, cw))}[fill].astype(np.int16)
    for seed in (1, 2):  # the halves outside the selected taps hold values far outside the limit: they are neither summed nor tested
        ok, got, ve, he = run_s16(plane, _junk(ch, np.int16, seed))
        assert ok.all()
        assert np.array_equal(got, reference(plane))
        assert ve <= 8 * L + 4 and he <= 64 * L + 32


def test_int16_bounds_are_reached_by_the_all_500_windows_and_fit_a_signed_half():
    for v, want in ((TAP_LIMIT, (8 * 500 + 4, 64 * 500 + 32)), (-TAP_LIMIT, (8 * 500 - 4, 64 * 500 - 32))):
        ok, got, ve, he = run_s16(np.full((3, 12), v, np.int16), _junk(3, np.int16))
        assert ok.all() and (ve, he) == want and he <= 32032 < 1 << 15
        assert (got == v).all()


@pytest.mark.parametrize("ch,cw", [(1, 4), (2, 8), (5, 12)])
@pytest.mark.parametrize("bad", (-TAP_LIMIT - 1, TAP_LIMIT + 1, -32768, 32767))
def test_a_tap_outside_the_limit_rejects_exactly_the_lanes_that_read_it(ch, cw, bad):
    rng = np.random.default_rng(3)
    base = rng.integers(-TAP_LIMIT, TAP_LIMIT + 1, (ch, cw)).astype(np.int16)
    lanes = lanes_of(base)
    for y in range(ch):
        for x in range(cw):
            plane = base.copy()
            plane[y, x] = bad
            ok, got, _, _ = run_s16(plane, _junk(ch, np.int16))
            reads = []
            for cx, cy in lanes:
                rows = {up_idx_s(cy - 1, ch), cy, up_idx_s(cy + 1, ch)}
                cols = set(range(cx, cx + 4)) | {cx - 1 if cx > 0 else cx + 1, cx + 4 if cx + 4 < cw else cx + 3}
                reads.append(y in rows and x in cols)
            assert ok.tolist() == [not r for r in reads], (y, x)
            assert np.array_equal(got[ok], reference(plane)[ok])


def test_the_limit_is_the_largest_that_keeps_the_sums_inside_int16():
    """64 * 500 + 32 <= 32767 < 64 * 512: the constant in the source is 500 and must not be widened"""
    assert "pk_splat(500)" in SRC and "pk_splat(1000)" in SRC and 64 * TAP_LIMIT + 32 <= 32767 < 64 * 512
    ok, got, _, he = run_s16(np.full((3, 12), 512, np.int16), _junk(3, np.int16))
    assert not ok.any() and he > 32767  # and were it let through, the packed sums would wrap:
    assert not np.array_equal(got, reference(np.full((3, 12), 512, np.int16)))


# ---------------------------------------------------------------------------------------------------------------------------------
# the facts of the scenes tests/test_gpu_pyrup_rows_first.py runs on the device
# ---------------------------------------------------------------------------------------------------------------------------------
from tests import constructed_multiband as CM  # noqa: E402
from tests import pyrup_rows_first_scenes as PS  # noqa: E402


@pytest.mark.parametrize("bands", (3, 4))
def test_scene_edges_facts(bands):
    scene = PS.edges(bands)
    assert scene.B == bands and scene.roi == (0, 0) + PS.EDGE_SIZES[bands] and scene.proi == scene.roi
    assert set(np.unique(PS.coverage(scene)).tolist()) == scene.facts["covering"]
    # the backdrop's feed rectangle is the panorama: its first lane is a left edge (X0 == fx), its last a right edge
    (fx, fy, fw, fh), _ = CM.feed_rect(scene.B, scene.proi, scene.roi[2], scene.roi[3], (0, 0))
    assert (fx, fy, fw, fh) == scene.proi and (fw // 8 - 1) * 4 + 4 >= fw >> 1
    # the tiny image starts and ends inside one lane and one row pair boundary crosses it
    tw, th, tx, ty = PS.TINY
    assert tx // 8 == (tx + tw - 1) // 8 == scene.facts["tiny_lane"] and tx % 8 != 0 and (tx + tw) % 8 != 0 and ty // 2 != (ty + th - 1) // 2
    # 0 and 255 in one 6-sample window of G_1: stripes of 12 columns are 6 samples of G_1 wide
    g1 = NB.pyr_down_16s(scene.feeds[0][0][:, :, 0].astype(np.int16))
    win = np.lib.stride_tricks.sliding_window_view(g1, 6, axis=1)
    assert ((win.min(axis=-1) == 0) & (win.max(axis=-1) == 255)).any()
    # the row rule is met at a wavefront's first and last coarse row only: the coarse planes are even and >= 4 rows high
    for lv in range(0, bands - 2):
        assert (fh >> (lv + 1)) % 2 == 0 and fh >> (lv + 1) >= 4


@pytest.mark.parametrize("grey", (False, True))
@pytest.mark.parametrize("bands", (3, 4))
def test_scene_holes_facts(bands, grey):
    scene = PS.holes(bands, grey)
    h = PS.HOLE_H[bands]
    assert scene.B == bands and scene.roi == (0, 0, PS.HOLE_W, h) and all(scene.binary) != grey
    tiles = set(PS.uncovered_tiles(scene))
    want = {(1, y) for y in range(0, 10, 2)} | {(c, y) for c in (0, 1) for y in range(10, 20, 2)} | {(0, y) for y in range(20, h, 2)}
    assert tiles == want
    assert set(np.unique(PS.coverage(scene)).tolist()) == {0, 1, 2}
    assert CM.expected_launches(scene, adopted=True)[2] == bands - 2  # every packed gather replays
