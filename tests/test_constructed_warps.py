"""The constructed warp cases (tests/constructed_warps.py) without a GPU: the constants they are shaped around are the ones in
csrc/stx_warp.hip, every case's stated facts hold under classify() on the maps of tests/numpy_warper.py, numpy_warper and the oracle
agree to the bit on the maps, the image and the mask of every case, and the families tell the contract from plausibly wrong variants
of it.

The variants are restatements of remap with ONE mistake each, of the kind the sampling paths of warp_fast_kernel can carry unnoticed;
they live here, are numpy only and are never imported by the product:

  variant                                                    family that tells it from the contract
  no int16 saturation of the pixel part                      saturation (and periods: the long sources)
  BORDER_REFLECT_101 taps                                    edge_taps
  round half away from zero in cvRound(32 v)                 phases (its "ties" cases)
  the nearest-neighbour mask with ties rounded up            mask_ties
  truncation toward zero instead of >> 5 below zero          edge_taps
Nothing here provokes a fault: these are host computations."""
import os
import re

import numpy as np
import pytest

from oracle import oracle as O
from tests import constructed_warps as CW
from tests import numpy_warper as NW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP = open(os.path.join(ROOT, "stitching_amd", "csrc", "stx_warp.hip")).read()


def _int(pattern, text=HIP):
    m = re.search(pattern, text)
    assert m, pattern
    return int(m.group(1), 0)


def test_the_kernels_constants_are_the_ones_the_families_are_shaped_around():
    assert _int(r"constexpr\s+int\s+WARP_WAVES\s*=\s*(\d+)\s*;") == 1
    assert re.search(r"constexpr\s+int\s+WARP_FW\s*=\s*64\s*\*\s*WARP_WAVES\s*;", HIP) and CW.LANES == 64
    assert CW.ROWS == _int(r"constexpr\s+int\s+WARP_TH\s*=\s*(\d+)\s*;")
    assert _int(r"constexpr\s+int\s+WARP_IT\s*=\s*(\d+)\s*;") == 1   # one block of WARP_TH rows per wavefront
    assert CW.BATCH == _int(r"constexpr\s+int\s+WARP_BATCH\s*=\s*(\d+)\s*;")
    assert CW.RND_U0 == _int(r"constexpr\s+uint32_t\s+RND_U0\s*=\s*(0x[0-9A-Fa-f]+)u\s*;")
    assert np.array([CW.RND_U0], np.uint32).view(np.float32)[0] == 1.5 * 2 ** 23
    assert re.search(r"const v2f k32 = \{32\.f, 32\.f\}, kmg = \{12582912\.f, 12582912\.f\};", HIP)
    # the chain of the fixed-point model: interior, zone, 2^21, generic; the fp32 models' interior a pixel further in
    assert re.search(r"const uint32_t u_lo = RM == STX_REMAP_Q15 \? RND_U0 : RND_U0 \+ 32u;", HIP)
    assert re.search(r"const bool lane_int = uxmn >= u_lo && uxmx <= ux_int && uymn >= u_lo && uymx <= uy_int;", HIP)
    assert re.search(r"const bool lane_zone = \(uxmn >= ux_zlo\) & \(uxmx <= ux_zhi\) & \(uymn >= uy_zlo\) & \(uymx <= uy_zhi\);", HIP)
    m = re.search(r"ballot_w64\(min\(uxmn, uymn\) < RND_U0 - \(1u << (\d+)\) \|\| max\(uxmx, uymx\) >= RND_U0 \+ \(1u << (\d+)\)\) == 0", HIP)
    assert m and 1 << int(m.group(1)) == 1 << int(m.group(2)) == CW.PERIODIC_LIMIT
    # the division: z_one, then the 2^-60 .. 2^60 test on z and the numerators' test, then fdiv
    m = re.search(r"bool easy = zlo >= (0x[0-9a-f]+) /\* 2\^-60 \*/ && zhi <= (0x[0-9a-f]+) /\* 2\^60 \*/;", HIP)
    assert m and (int(m.group(1), 16), int(m.group(2), 16)) == (CW.Z_MIN_BITS, CW.Z_MAX_BITS)
    assert np.array([CW.Z_MIN_BITS, CW.Z_MAX_BITS], np.uint32).view(np.float32).tolist() == [2.0 ** -60, 2.0 ** 60]
    assert re.search(r"easy = easy && nmax <= 0x1p60f;", HIP) and CW.NUM_MAX == 2.0 ** 60
    assert re.search(r"\* bz <= 0x1p59;", HIP) and CW.NUM_BOUND == 2.0 ** 59
    assert re.search(r"K\.z_one = K\.num_ok && L\.proj\.family == STX_F_PLANE && K\.kr\[6\] == 0\.f && K\.kr\[7\] == 0\.f && K\.c8 == 1\.0f \? 1 : 0;", HIP)
    # the host setup's expressions of the interior, the zone and the mask test, for both axes
    for a, n in (("x", "sw"), ("y", "sh")):
        assert re.search(r"const int z%s_lo = std::max\(-32 \* L\.%s, -32768 \* 32\), z%s_hi = std::min\(64 \* L\.%s - 33, 32767 \* 32 \+ 31\);" % (a, n, a, n), HIP)
        assert re.search(r"K\.u%s_int = RND_U0 \+ \(uint32_t\)\(32 \* \(L\.%s - 1\) - 1\);" % (a, n), HIP)
        assert re.search(r"K\.u%s_zlo = RND_U0 \+ \(uint32_t\)z%s_lo; K\.u%s_zhi = RND_U0 \+ \(uint32_t\)z%s_hi;" % (a, a, a, a), HIP)
        assert re.search(r"K\.m%s32_hi = 32\.f \* \(\(\(L\.%s - 1\) & 1\) \? \(float\)\(L\.%s - 0\.5\) : std::nextafterf\(\(float\)\(L\.%s - 0\.5\), 3\.0e38f\)\);" % (a, n, n, n), HIP)
        assert re.search(r"K\.per_%s = 64 \* L\.%s;" % (a, n), HIP)
    assert re.search(r"return !K\.msrc && K\.sw <= (\d+) && K\.sh <= \1 && K\.sw >= 2 && K\.sh >= 2", HIP).group(1) == str(CW.TUNED_MAX)
    assert (CW.S16_MIN, CW.S16_MAX) == (-32768, 32767)
    # mirror_axis and periodic_axis, statement by statement: mirror_axis() and periodic_axis() below restate exactly these
    for line in (r"int m = max(max(s, -32 - s), 0);", r"m = min(min(m, 64 * n - 32 - m), 32 * (n - 1));", r"const int i = min(m >> 5, n - 2);",
                 r"fp = (uint32_t)(m - (i << 5));",
                 r"const int se = (min(max(s >> 5, -32768), 32767) << 5) | (s & 31);", r"const uint32_t a = (uint32_t)(se + bias);",
                 r"const uint32_t q = (uint32_t)(int)__fmul_rn((float)a, inv_period);", r"uint32_t r = a - __umul24(q, (uint32_t)period);",
                 r"r = min(r, r + (uint32_t)period);", r"r = min(r, r - (uint32_t)period);", r"return (int)r - 32 * n;"):
        assert line in HIP, line
    # ... and the host's period, reciprocal and bias of both axes
    assert "K.inv_x = 1.0f / (float)K.per_x; K.inv_y = 1.0f / (float)K.per_y;" in HIP
    for a, n in (("x", "sw"), ("y", "sh")):
        assert "K.bias_%s = 32 * L.%s + K.per_%s * (((1 << 20) + K.per_%s - 1) / K.per_%s);" % (a, n, a, a, a) in HIP
        assert "mirror_axis(periodic_axis((int)(u%s[j] - RND_U0), %s, per_%s, inv_%s, bias_%s), %s, i%s, f%s);" % (a, n, a, a, a, n, a, a) in HIP
    # and the functions of them
    assert [CW.interior_hi(n) for n in (2, 331)] == [31, 10559] and CW.zone(331) == (-10592, 21151)
    assert CW.zone(16384) == (-524288, 1048543) and CW.zone(16385) == (-524320, 1048575) and CW.zone(32767) == (-1048544, 1048575)
    assert (CW.RECT_W, CW.RECT_H) == (3 * CW.LANES, 2 * CW.ROWS)


# ---------------------------------------------------------------------------------------------------------------------------------
# the two references
# ---------------------------------------------------------------------------------------------------------------------------------
_maps = {}


def maps(case):
    if case.name not in _maps:
        with np.errstate(all="ignore"):
            _maps[case.name] = NW.map_backward(case.warper_type, case.scale, case.K, case.R, case.rect)
    return _maps[case.name]


def numerators(case):
    """(X, Y, Z, k_rinv, T): numerators and denominator of every pixel, every step rounded to fp32 (numpy_warper's arithmetic)"""
    kind, R, T = case.warper_type, case.R, None
    if kind == "affine":
        (R, T), kind = NW.affine_params(R), "plane"
    k_rinv = NW.projector_setup(case.K, R)[0]
    s = np.float32(case.scale)
    x0, y0, w, h = case.rect
    u = (np.arange(x0, x0 + w).astype(np.float32)[None, :] / s) + np.zeros((h, 1), np.float32)
    v = (np.arange(y0, y0 + h).astype(np.float32)[:, None] / s) + np.zeros((1, w), np.float32)
    if kind == "spherical":
        sinv = NW._m(np.sin, NW.PI_F - v)
        x_, y_, z_ = sinv * NW._m(np.sin, u), NW._m(np.cos, NW.PI_F - v), sinv * NW._m(np.cos, u)
    elif kind == "cylindrical":
        x_, y_, z_ = NW._m(np.sin, u), v, NW._m(np.cos, u)
    else:
        t = np.zeros(3, np.float32) if T is None else np.asarray(T, np.float32)
        x_, y_, z_ = u - t[0], v - t[1], np.full_like(u, np.float32(1) - t[2])
    with np.errstate(all="ignore"):
        return tuple(NW._dot3(k_rinv, r, x_, y_, z_) for r in range(3)) + (k_rinv, T)


def division(case):
    X, Y, Z, k_rinv, T = numerators(case)
    kind = "plane" if case.warper_type == "affine" else case.warper_type
    num_ok, z_one = CW.host_flags(kind, case.scale, k_rinv, T, case.rect)
    waves, lanes = CW.classify_division(kind, X, Y, Z, num_ok, z_one)
    return waves, lanes, Z, num_ok


@pytest.mark.parametrize("name", list(CW.CASES))
def test_facts_hold_and_the_references_agree(name):
    case = CW.CASES[name]
    wt, scale, K, R, src, rect, f = case
    xm, ym = maps(case)
    assert xm.shape == (rect[3], rect[2])
    waves, lanes, px = CW.classify(xm, ym, *case.size, case.model)
    if "waves" in f:
        assert np.array_equal(waves, f["waves"]), (waves, f["waves"])
    if "sx" in f:   # the plane construction: the integers the camera's entries give
        assert np.array_equal(lanes, f["lanes"]) and np.array_equal(px, f["pixels"])
        for m, s in ((xm, f["sx"]), (ym, f["sy"])):
            exact = np.abs(s) < 1 << 24   # beyond, fp32 no longer holds every 1/32: the class (generic) is all the family states
            assert np.array_equal(NW._cv_round(m * np.float32(32))[exact], s[exact])
    if "target" in f:   # one sample, everything else further to the near side
        tc, tr = f["target"]
        s = f["sx"] if f["axis"] == "x" else f["sy"]
        nr = tr - 1 if tr else 1   # a neighbouring row: 32 units to the near side
        side = np.sign(s[tr, tc] - s[nr, tc])
        assert s[tr, tc] == f["s_target"] and np.count_nonzero((s - f["s_target"]) * side >= 0) == 1
        if px[tr, tc] != px[nr, tc]:   # 1/32 past a limit that changes the class: one pixel, one wavefront
            assert np.count_nonzero(px == px[tr, tc]) == 1 and np.count_nonzero(waves == px[tr, tc]) == 1
            by, bx = tr // CW.ROWS, tc // CW.LANES
            clamped = bx * CW.LANES + CW.LANES - rect[2] if tc == rect[2] - 1 and rect[2] % CW.LANES else 0
            assert np.count_nonzero(lanes[by, bx] == px[tr, tc]) == 1 + max(clamped, 0)
    if "means" in f:
        assert (waves == f["means"]).all()
    if "pairs" in f:
        for a, b in f["pairs"]:
            assert any(a in l and b in l for l in lanes.reshape(-1, CW.LANES)), (a, b)
    # the division
    dwaves, dlanes, Z, num_ok = division(case)
    if "division" in f:
        assert {CW.DIV_NAMES[c] for c in np.unique(dlanes)} == f["division"], np.unique(dlanes)
    if "num_ok" in f:
        assert num_ok == f["num_ok"]
    if "z" in f:
        signs = "".join(ch for ch, hit in (("-", (Z < 0).any()), ("0", (Z == 0).any()), ("+", (Z > 0).any())) if hit)
        assert signs == f["z"], signs
    if "nonfinite" in f:
        assert (np.isnan(xm).any() if f["nonfinite"] == "nan" else np.isinf(xm).any())
    if "same_maps_as" in f:
        a, b = maps(CW.CASES[f["same_maps_as"]])
        assert np.array_equal(a, xm) and np.array_equal(b, ym)
    # numpy_warper and the oracle, to the bit (NaN == NaN): maps, image (fixed-point model), mask
    ox, oy = O.build_maps(wt, scale, K, R, rect)
    assert np.array_equal(xm, ox, equal_nan=True) and np.array_equal(ym, oy, equal_nan=True)
    ones = np.full(src.shape[:2], 255, np.uint8)
    assert np.array_equal(NW.remap_linear_reflect(src, xm, ym), O.remap_linear(src, ox, oy))
    assert np.array_equal(NW.remap_nearest_constant(ones, xm, ym), O.remap_nearest(ones, ox, oy))


# ---------------------------------------------------------------------------------------------------------------------------------
# what the families reach
# ---------------------------------------------------------------------------------------------------------------------------------
def reach():
    """family -> {class name: wavefronts of that class}, sampling chain and division chain, by classify on numpy_warper's maps"""
    out = {}
    for case in CW.CASES.values():
        d = out.setdefault(case.family, {})
        if not CW.tuned(case):
            d["warp_kernel"] = d.get("warp_kernel", 0) + 1   # images, not wavefronts: the tuned kernel refuses the source
            continue
        waves = CW.classify(*maps(case), *case.size, case.model)[0]
        for c in np.unique(waves):
            key = CW.CLASS_NAMES[c] if case.model == "q15" else case.model + " " + CW.CLASS_NAMES[c]
            d[key] = d.get(key, 0) + int(np.count_nonzero(waves == c))
        dw = division(case)[0]
        for c, nm in enumerate(CW.DIV_NAMES):
            if dw[..., c].any():
                d[nm] = d.get(nm, 0) + int(np.count_nonzero(dw[..., c]))
    return out


def test_every_branch_of_both_chains_is_reached_by_a_named_family():
    r = reach()
    for fam in sorted(r):
        print(fam, dict(sorted(r[fam].items())))
    for fam in ("thresholds", "phases", "affine_thresholds", "affine_phases", "clamped"):
        assert all(r[fam].get(c, 0) > 0 for c in ("interior", "mirror", "periodic", "generic", "z_one")), (fam, r[fam])
    assert r["edge_taps"]["mirror"] > 0 and r["periods"]["periodic"] > 0 and r["periods"]["generic"] > 0
    assert r["saturation"]["periodic"] > 0 and r["saturation"]["mirror"] > 0
    assert all(r["searched"].get(c, 0) > 0 for c in ("interior", "mirror", "periodic", "generic", "easy"))
    assert r["division"]["easy"] > 0 and r["division"]["fdiv"] > 0 and "z_one" not in r["division"]
    for m in ("float", "float_fma"):
        assert all(r[f].get(f"{m} {c}", 0) > 0 for f in ("float_thresholds", "float_edge_taps") for c in ("interior", "other"))
    assert r["refused"] == {"warp_kernel": len(CW.family("refused"))}
    # the searched rectangles: all four classes and every adjacent pair inside one wavefront, for both rotation warpers
    for wt in ("spherical", "cylindrical"):
        cs = [c for c in CW.family("searched") if c.warper_type == wt]
        assert set(np.unique(np.concatenate([c.facts["waves"].ravel() for c in cs]))) == {0, 1, 2, 3}
        assert set().union(*[c.facts["pairs"] for c in cs]) == {(0, 1), (1, 2), (2, 3)}


def test_the_searched_rectangles_lie_around_the_pitched_cameras_roi():
    for c in CW.family("searched"):
        roi = NW.warp_roi(c.warper_type, c.scale, c.K, c.R, c.size)
        assert roi[0] - 512 <= c.rect[0] <= roi[0] + roi[2] + 512 and roi[1] - 128 <= c.rect[1] <= roi[1] + roi[3] + 128
        assert (c.rect[0] - roi[0]) % CW.LANES == 0 and (c.rect[1] - roi[1]) % CW.ROWS == 0


def search(wt, cam=0):
    """The search behind CW.SEARCHED: every 192 x 8 rectangle in steps of one wavefront, 512 columns and 128 rows around the ROI of a
    pitched camera -> {rectangle: (classes of its 2 x 3 wavefronts, adjacent pairs of classes met inside ONE of its wavefronts)}, in
    row-major order of the rectangles"""
    scale, K, R = CW.pitched_camera(cam)
    roi = NW.warp_roi(wt, scale, K, R, CW.PITCHED_SIZE)
    x0, y0 = roi[0] - 512, roi[1] - 128
    w, h = -(-(roi[2] + 1024) // CW.LANES) * CW.LANES, -(-(roi[3] + 256) // CW.ROWS) * CW.ROWS
    with np.errstate(all="ignore"):
        xm, ym = NW.map_backward(wt, scale, K, R, (x0, y0, w, h))
    waves, lanes, _ = CW.classify(xm, ym, *CW.PITCHED_SIZE)
    has = np.stack([(lanes == c).any(axis=2) for c in range(4)])
    both = has[:-1] & has[1:]   # [pair (a, a + 1)][block row][wavefront column]
    out = {}
    for by in range(waves.shape[0] - 1):
        for bx in range(waves.shape[1] - 2):
            pairs = {(a, a + 1) for a in range(3) if both[a, by:by + 2, bx:bx + 3].any()}
            out[(x0 + bx * CW.LANES, y0 + by * CW.ROWS, CW.RECT_W, CW.RECT_H)] = (waves[by:by + 2, bx:bx + 3], pairs)
    return out


@pytest.mark.parametrize("wt", ["spherical", "cylindrical"])
def test_the_search_finds_the_rectangles_written_into_the_file(wt):
    """Per warper CW.SEARCHED holds two of the rectangles the search finds: the first, in row-major order, with a wavefront of every
    class but the interior's and both pairs (mirror, periodic) and (periodic, generic) inside single wavefronts, and the first with
    interior and mirror lanes inside one wavefront"""
    found = search(wt)
    mine = [(rect, waves, pairs) for w, cam, rect, waves, pairs in CW.SEARCHED if w == wt and cam == 0]
    assert len(mine) == 2
    for rect, waves, pairs in mine:
        assert np.array_equal(found[rect][0], waves) and found[rect][1] == set(pairs), (rect, found[rect])
    first_far = next(r for r, (wv, p) in found.items() if {(1, 2), (2, 3)} <= p and {1, 2, 3} <= set(wv.ravel().tolist()))
    first_near = next(r for r, (wv, p) in found.items() if (0, 1) in p and 0 in wv)
    print(wt, "first with (1, 2) and (2, 3):", first_far, "first with (0, 1):", first_near)
    assert [first_far, first_near] == [m[0] for m in mine]


# ---------------------------------------------------------------------------------------------------------------------------------
# the periodic path's quotient estimate
# ---------------------------------------------------------------------------------------------------------------------------------
def quotient_error(s, n):
    """periodic_axis: (first estimate of floor(a / period)) - floor(a / period) for the positions s of an axis of n pixels"""
    f = np.float32
    per = 64 * n
    inv = f(1) / f(per)
    bias = 32 * n + per * (((1 << 20) + per - 1) // per)
    s = np.asarray(s, np.int64)
    a = ((np.clip(s >> 5, CW.S16_MIN, CW.S16_MAX) << 5) | (s & 31)) + bias
    assert a.min() >= 0 and a.max() < 1 << 23   # exact in fp32
    return (a.astype(f) * inv).astype(f).astype(np.int64) - a // per


def test_the_quotient_estimate_and_what_the_periods_family_holds_of_it():
    """Over all |s| < 2^21 the first estimate is never off for the sizes 2, 3, 5, 331, 16 385 and 32 767, so neither correction runs for
    them; for 41 it is one too LOW where the biased position is a multiple of the period (half a period off the origin), which the family's
    "+0-half" case holds in columns 9 to 95.  One too HIGH does not occur for any of them (nor for any other size: the next test): the
    correction for it has no input that reaches it."""
    s = np.arange(-CW.PERIODIC_LIMIT, CW.PERIODIC_LIMIT, dtype=np.int64)
    errs = {n: quotient_error(s, n) for n in CW.PERIOD_N}
    assert all(np.abs(e).max() <= 1 for e in errs.values())
    assert {n for n, e in errs.items() if (e < 0).any()} == {41} and not any((e > 0).any() for e in errs.values())
    held = set()
    for c in CW.family("periods"):
        if c.facts["means"] == CW.PERIODIC:
            e = quotient_error(c.facts["sx" if c.facts["axis"] == "x" else "sy"], c.facts["n"])
            held |= {(c.facts["n"], int(v)) for v in np.unique(e)}
    assert (41, -1) in held and not any(v > 0 for _, v in held)


def test_the_quotient_estimate_of_every_size_the_tuned_kernel_takes():
    """For every n from 2 to 32 767: the first estimate is never one too HIGH, and one too LOW for 4 843 of the sizes, 41 the smallest.
    The biased positions a of an axis are the integers of [bias - 2^20, bias + 2^20) (the pixel part is saturated), and the estimate
    fl(fl(a) fl(1 / period)) does not decrease with a while floor(a / period) steps on the multiples of the period.  So if any a is one
    too low, the multiple of the period at or below it is (or, where that lies outside, the first a of the range); if any a is one too
    high, the a before the next multiple is (or the last of the range).  Those, and the neighbours of the multiples, are evaluated."""
    f = np.float32
    low = []
    for n in range(2, CW.TUNED_MAX + 1):
        per = 64 * n
        bias = 32 * n + per * (((1 << 20) + per - 1) // per)
        first, last = bias - (1 << 20), bias + (1 << 20) - 1
        assert 0 <= first and last < 1 << 23
        m = np.arange(first // per, last // per + 2, dtype=np.int64) * per
        a = np.concatenate([m - 1, m, m + 1, [first, last]])
        a = a[(a >= first) & (a <= last)]
        e = (a.astype(f) * (f(1) / f(per))).astype(f).astype(np.int64) - a // per
        assert -1 <= e.min() and e.max() <= 0, (n, e.min(), e.max())
        if e.min() < 0:
            assert (e[a % per != 0] == 0).all(), n   # only on the multiples themselves
            low.append(n)
    assert (len(low), low[0]) == (4843, 41) and not set(low) & {2, 3, 5, 331, 16385, 32767}


def mirror_axis(s, n):
    """csrc/stx_warp.hip: mirror_axis, in numpy: position -> (base pixel, weight of the pixel to its right, 0 .. 32)"""
    m = np.maximum(np.maximum(s, -32 - s), 0)
    m = np.minimum(np.minimum(m, 64 * n - 32 - m), 32 * (n - 1))
    i = np.minimum(m >> 5, n - 2)
    return i, m - (i << 5)


def periodic_axis(s, n):
    """csrc/stx_warp.hip: periodic_axis, in numpy (the quotient estimate in fp32, corrected one step either way)"""
    f = np.float32
    per = 64 * n
    bias = 32 * n + per * (((1 << 20) + per - 1) // per)
    a = ((np.clip(s >> 5, CW.S16_MIN, CW.S16_MAX) << 5) | (s & 31)) + bias
    q = (a.astype(f) * (f(1) / f(per))).astype(f).astype(np.int64)
    r = (a - q * per) & 0xFFFFFFFF
    r = np.minimum(r, (r + per) & 0xFFFFFFFF)
    r = np.minimum(r, (r - per) & 0xFFFFFFFF)
    return r - 32 * n


def _canonical(p0, w0, p1, w1):
    """two weighted taps as (pixel, weight, other pixel or -1): equal pixels merged, a tap of weight 0 dropped, the smaller pixel first"""
    one = (p0 == p1) | (w1 == 0) | (w0 == 0)
    p = np.where(w0 == 0, p1, p0)
    lo_first = p0 < p1
    return (np.where(one, p, np.minimum(p0, p1)), np.where(one, 32, np.where(lo_first, w0, w1)), np.where(one, -1, np.maximum(p0, p1)))


@pytest.mark.parametrize("n", [2, 41, 331, 16385, 32767])
def test_within_the_limits_the_mirrored_and_the_reduced_position_are_the_contract(n):
    """Inside the zone mirror_axis gives the taps and weights of saturate-then-BORDER_REFLECT, inside +-2^21 mirror_axis of
    periodic_axis does, for every s, with a base pixel inside [0, n - 2]: within the limits classify() and the families are built on,
    the kernel's shortcuts are the contract.  (The zone is not tight: -32 n - 1 would still come out right.)"""
    s = np.arange(-CW.PERIODIC_LIMIT - 64, CW.PERIODIC_LIMIT + 64, dtype=np.int64)
    ix, fx = NW._sat16(s >> 5), s & 31
    want = _canonical(NW._reflect(ix, n), 32 - fx, NW._reflect(ix + 1, n), fx)
    zl, zh = CW.zone(n)

    def same(got, sel):
        return np.array([np.array_equal(g[sel], w[sel]) for g, w in zip(got, want)]).all()

    i, f = mirror_axis(s, n)
    mirrored = _canonical(i, 32 - f, i + 1, f)
    inside = (s >= zl) & (s <= zh)
    assert same(mirrored, inside)
    assert (i[inside] >= 0).all() and (i[inside] <= n - 2).all()
    i, f = mirror_axis(periodic_axis(s, n), n)
    inside = np.abs(s + 0.5) < CW.PERIODIC_LIMIT
    assert same(_canonical(i, 32 - f, i + 1, f), inside)
    assert (i[inside] >= 0).all() and (i[inside] <= n - 2).all() and (f[inside] >= 0).all() and (f[inside] <= 32).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# the variants
# ---------------------------------------------------------------------------------------------------------------------------------
def _reflect101(p, n):
    if n == 1:
        return np.zeros_like(p)
    p = np.mod(p, 2 * n - 2)
    return np.where(p >= n, 2 * n - 2 - p, p)


def variant_linear(src, xmap, ymap, saturate=True, reflect101=False, half_away=False, truncate=False):
    """numpy_warper.remap_linear_reflect with the named mistakes"""
    H, W = src.shape[:2]

    def quantise(m):
        with np.errstate(all="ignore"):
            v = (m * np.float32(32)).astype(np.float64)
            if half_away:
                ok = np.abs(v) < 2.0 ** 31
                s = np.where(ok, np.sign(v) * np.floor(np.abs(np.where(ok, v, 0)) + 0.5), -2.0 ** 31).astype(np.int64)
            else:
                s = NW._cv_round(m * np.float32(32))
        i = np.where(s < 0, -((-s) >> 5), s >> 5) if truncate else s >> 5
        return (NW._sat16(i) if saturate else i), s & 31

    (ix, fx), (iy, fy) = quantise(xmap), quantise(ymap)
    refl = _reflect101 if reflect101 else NW._reflect
    x0, x1, y0, y1 = refl(ix, W), refl(ix + 1, W), refl(iy, H), refl(iy + 1, H)
    w = [(32 - fx) * (32 - fy) * 32, fx * (32 - fy) * 32, (32 - fx) * fy * 32, fx * fy * 32]
    s = src.astype(np.int64)
    acc = sum(wk[..., None] * t for wk, t in zip(w, [s[y0, x0], s[y0, x1], s[y1, x0], s[y1, x1]]))
    return ((acc + 16384) >> 15).astype(np.uint8)


def variant_mask_ties_up(size, xmap, ymap):
    with np.errstate(all="ignore"):
        ix, iy = (NW._sat16(np.where(np.isfinite(m), np.floor(m.astype(np.float64) + 0.5), -2.0 ** 31).astype(np.int64)) for m in (xmap, ymap))
    return np.where((ix >= 0) & (ix < size[0]) & (iy >= 0) & (iy < size[1]), 255, 0).astype(np.uint8)


VARIANTS = {"no_saturation": (dict(saturate=False), "saturation"), "reflect_101": (dict(reflect101=True), "edge_taps"),
            "half_away": (dict(half_away=True), "phases"), "truncate": (dict(truncate=True), "edge_taps"), "mask_ties_up": (None, "mask_ties")}


def caught_by(variant):
    """family -> cases of it in which the variant changes at least one byte (fixed-point cases of the tuned kernel)"""
    kw = VARIANTS[variant][0]
    out = {}
    for c in CW.CASES.values():
        if c.model != "q15":
            continue
        xm, ym = maps(c)
        if kw is None:
            ones = np.full(c.source.shape[:2], 255, np.uint8)
            diff = not np.array_equal(variant_mask_ties_up(c.size, xm, ym), NW.remap_nearest_constant(ones, xm, ym))
        else:
            diff = not np.array_equal(variant_linear(c.source, xm, ym, **kw), NW.remap_linear_reflect(c.source, xm, ym))
        if diff:
            out[c.family] = out.get(c.family, 0) + 1
    return out


def test_the_restatement_without_a_mistake_is_the_contract():
    for fam in ("edge_taps", "saturation", "phases", "division"):
        for c in CW.family(fam):
            xm, ym = maps(c)
            assert np.array_equal(variant_linear(c.source, xm, ym), NW.remap_linear_reflect(c.source, xm, ym)), c.name


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_a_named_family_tells_the_contract_from_the_variant(variant):
    caught = caught_by(variant)
    print(variant, "changes bytes in", dict(sorted(caught.items())))
    fam = VARIANTS[variant][1]
    assert caught.get(fam, 0) > 0, (variant, fam, caught)
    if variant == "half_away":   # the ties cases, on both axes and at every limit that is an integer number of 1/32
        ties = [c for c in CW.family("phases") if c.facts["ties"]]
        hit = [c for c in ties if not np.array_equal(variant_linear(c.source, *maps(c), half_away=True), NW.remap_linear_reflect(c.source, *maps(c)))]
        assert len(hit) >= len(ties) - 4, [c.name for c in ties if c not in hit]   # (beyond 2^22 a tie is no longer a float)
    if variant == "no_saturation":
        assert caught.get("periods", 0) > 0 and caught.get("thresholds", 0) > 0
