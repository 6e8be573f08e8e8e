"""The constructed multi-band families (tests/constructed_multiband.py) without a GPU: the constants they are shaped around are the ones
in the sources, every family's stated facts hold, both CPU references (the oracle's blender handle, OpenCV's algorithm restated in C++,
and tests/numpy_blenders.py) agree on every scene to the byte, classify() counts at least one lane, wavefront or run on every path
of PATHS and puts the limit cases on the side the construction promises, and each family tells the contract from a plausibly wrong
variant.

The variants are restatements of NumpyMultiBand with ONE mistake each, of the kind the packed kernels can carry unnoticed; they live
here, are numpy only and are never imported by the product:

  variant                                                      family that tells it from the contract
  a saturating instead of a wrapping accumulator               accumulator_wrap (150, 255)
  division by n without the 1e-5                               count_edges (exact multiples of the count)
  the product rounded instead of truncated                     occupancy_edges (fractional weights from level 1 on)
  the quotient rounded instead of truncated                    count_edges
  a wrapping instead of a saturating collapse add              launch_matrix ("s16_overshoot": the overshoot scene in int16, 128 times as bright)
  pyrUp's border rule -1 -> 0 instead of -1 -> 1               up_borders
  REFLECT_101 instead of REFLECT around the image              down0_runs
  REFLECT instead of REFLECT_101 in pyrDown                    down0_runs
  a reflected instead of a constant-0 weight border            down0_runs
  weights as m / 256                                           grey_bytes
  a grey byte treated as 255                                   grey_bytes
  images summed in reverse feed order                          feed_order (fp32 weight sums of grey masks)
  mask > 0 instead of > 1e-5                                   NOT distinguishable: the smallest non-zero weight of a u8 mask is 1 / 255
Nothing here provokes a fault: these are host computations."""
import functools
import os
import re

import numpy as np
import pytest
from scipy import ndimage

from oracle import oracle as O
from stitching_amd import _lib
from tests import constructed_multiband as CM
from tests import helpers
from tests import numpy_blenders as NB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stitching_amd", "csrc")


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def _int(pattern, text):
    m = re.search(pattern, text)
    assert m, pattern
    return int(m.group(1))


def test_the_kernels_constants_are_the_ones_the_families_are_shaped_around():
    fast, kern, host, internal = _src("stx_blend_fast.hip"), _src("stx_blend_kernels.h"), _src("stx_blend_host.cpp"), _src("stx_internal.h")
    # the gathers: one wavefront per workgroup, 64 lanes of 8 x 2 patches, tiles of 512 x 2
    assert re.search(r"constexpr int LV_WAVES = 1, LV_TH = 2 \* LV_WAVES, LV_THREADS = 64 \* LV_WAVES;", fast)
    assert CM.TILE_H == CM.STRIP_H == 2 and CM.LANES == 64 and CM.TILE_W == CM.LANES * CM.STRIP_W
    assert len(re.findall(r"const int tile_x = P\.x0 \+ tile_tx \* %d, tile_y = P\.y0 \+ tile_ty \* LV_TH;" % CM.TILE_W, fast)) >= 2
    assert len(re.findall(r"const int X0 = tile_x \+ \(tid & 63\) \* %d, Y0 = tile_y \+ __builtin_amdgcn_readfirstlane\(tid >> 6\) \* 2;" % CM.STRIP_W, fast)) >= 2
    assert re.search(r"KT->tiles = stx_tile_map\(\(K\.x1 - K\.x0 \+ 511\) / 512, \(K\.y1 - K\.y0 \+ LV_TH - 1\) / LV_TH, LV_BAND\);", fast)
    # the level-0 pyrDown
    m = re.search(r"constexpr int DN_TOW = (\d+), DN_TOH = (\d+), DN_ROWS = 2 \* DN_TOH \+ 3;", fast)
    assert m and (int(m.group(1)), int(m.group(2))) == (CM.DN_TOW, CM.DN_TOH) and CM.DN_ROWS == 2 * CM.DN_TOH + 3
    assert re.search(r"const int c0 = 2 \* xo - 2;", fast) and re.search(r"c0 \+ %d < im\.fw && a0 >= 0 && a0 \+ %d < im\.iw" % (CM.RUN - 1, CM.RUN - 1), fast)
    assert re.search(r"if \(s_low >= 0 && s_low \+ %d < im\.iw\)" % (CM.RUN - 1), fast)
    assert re.search(r"const int q = tid & 15, rA = tid >> 4;", fast) and CM.RUN_GROUP == CM.DN_TOW // 4 == 16
    assert re.search(r"mw\[2\] = __builtin_amdgcn_alignbyte\(m\.w, m\.z, ms\) & 0x00ffffffu;", fast)  # byte 11 of a run is masked off
    # the batched branch: wave-uniform, every run of the tile column interior or mirrored, the image NEAR
    assert re.search(r"batched = __builtin_amdgcn_ballot_w64\(col_ok && !\(interior \|\| mirrored\)\) == 0ull;", fast)
    assert re.search(r"bool batched = false;\s*if \(near\) \{", fast) and re.search(r"task < DN_ROWS \* \(DN_TOW / 4\) && !batched; task \+= 256", fast)
    # the collapse and the normalisation tiers
    assert set(re.findall(r"pk_splat\((\d+)\)\);\n", fast[fast.index("STX_DEV bool up_patch_pks_math"):fast.index("STX_DEV bool up_patch_pks(")])) == {str(CM.TAP_LIMIT)}
    assert re.search(r"__builtin_elementwise_min\(worst, pk_splat\(%d\)\)" % (2 * CM.TAP_LIMIT), fast)
    assert re.search(r"if \(!WF && \(anyc & 0xfffefffeu\) == 0u\)", fast) and CM.COUNT_SIGN == 1
    assert re.search(r"else if \(!WF && \(cnt3 & 0xfffcfffcu\) == 0u\)", fast) and CM.COUNT_SHIFT == 2
    assert re.search(r"const bool small = !WF && \(anyc & 0xfff0fff0u\) == 0u;", fast) and CM.COUNT_RCP == 16
    # the image limits
    assert re.search(r"if \(K\.n_images > %d\) return false;" % CM.PACKED_IMAGES, fast)
    assert re.search(r"K\.n_images <= %d && !K\.has_contrib; \}" % CM.COVER_IMAGES, fast)
    assert re.search(r"if \(b->images\.size\(\) > %d \|\| !b->d_gather\) return;" % CM.COVER_IMAGES, host)
    assert re.search(r"if \(K\.num_bands - K\.level < %d\) return false;" % CM.FAST_LEVELS_BELOW, fast)
    assert re.search(r"const bool fuse = nb >= %d && !no_fusion;" % CM.FAST_LEVELS_BELOW, host)
    assert CM.DEFER_SEGS == _int(r"constexpr int STX_DEFER_SEGS = (\d+);", kern)
    assert re.search(r"const unsigned seg = \(unsigned\)tile_tx % \(unsigned\)STX_DEFER_SEGS;", fast)
    assert re.search(r"STX_DEV int occ_pitch\(int lw\) \{ return \(\(\(lw \+ 63\) >> 6\) \+ 3\) & ~3; \}", fast) and CM.OCC_CELL == 64
    assert CM.MAX_BANDS == _int(r"#define STX_MAX_BANDS (\d+)", internal)
    # the host's geometry: the border, the band count, the regions
    assert re.search(r"const int gap = 3 \* \(1 << nb\);", host) and [CM.border(b) for b in (0, 3, 5)] == [3, 24, 96]
    assert re.search(r"int nb = std::min\(num_bands, \(int\)std::ceil\(std::log\(max_len\) / std::log\(2\.0\)\)\);", host)
    assert re.search(r"const int al = i <= b->num_bands - 3 \? 7 : 1;", host)
    assert CM.MULTIBAND == _lib.BLEND_MULTIBAND == O._OracleBlenderHandle.MULTI_BAND
    # the geometry restated here against the numpy reference's own (written from SURVEY.md A.6)
    for scene in (CM.down0_runs(), CM.sharded("binary"), CM.up_borders(8)):
        ref = CM.numpy_reference(scene)[0]
        assert ref.B == scene.B and ref.roi == scene.proi
        for fd, (_, m, tl) in zip(ref.fed, scene.feeds):
            rect, (left, top) = CM.feed_rect(scene.B, scene.proi, m.shape[1], m.shape[0], tl)
            assert rect == fd["rect"] and (left, top) == (fd["image"][0] - rect[0], fd["image"][1] - rect[1])
    # the shapes lie around the constants
    assert set(CM.COUNT_N) >= {CM.COUNT_SIGN, CM.COUNT_SHIFT, CM.COUNT_SHIFT + 1, CM.COUNT_RCP - 1, CM.COUNT_RCP, CM.COUNT_RCP + 1,
                               CM.COVER_IMAGES - 1, CM.COVER_IMAGES, CM.COVER_IMAGES + 1, 128, 129, CM.PACKED_IMAGES, CM.PACKED_IMAGES + 1}
    assert CM.WIDE_W > CM.DEFER_SEGS * CM.TILE_W and CM.GREY_W > CM.TILE_W
    assert {w % CM.TILE_W for w in CM.OCC_W} == {0, 8, 16} and min(CM.UP_W) == CM.STRIP_W


# ---------------------------------------------------------------------------------------------------------------------------------
# the scenes, the two references
# ---------------------------------------------------------------------------------------------------------------------------------
SCENES = ([("accumulator_wrap", (n,)) for n in CM.WRAP_N] + [("accumulator_wrap", (255, s)) for s in ("same", "big")] +
          [("count_edges", (n,)) for n in CM.COUNT_N] + [("grey_bytes", c) for c in CM.GREY_CASES] + [("grey_wide", ())] +
          [("down0_runs", (g,)) for g in (False, True)] + [("down0_batched", (g,)) for g in (False, True)] + [("up_borders", c) for c in CM.UP_CASES] +
          [("occupancy_edges", (w, z)) for w in CM.OCC_W for z in CM.OCC_ZERO_AT] + [("collapse_overshoot", (k,)) for k in CM.OVERSHOOT_CASES] +
          [("launch_matrix", (k,)) for k in CM.LAUNCH_CASES] + [("sharded", (k,)) for k in CM.SHARDED_CASES] + [("feed_order", ()), ("acc_extremes", ())])


def oracle_blend(scene):
    b = O._OracleBlenderHandle(CM.MULTIBAND, scene.bands, 0.0)
    b.prepare(scene.roi)
    assert b.num_bands() == scene.B
    for img, mask, corner in scene.feeds:
        b.feed(np.asarray(img).astype(np.int16), mask, corner)
    return b.blend()


@functools.lru_cache(maxsize=None)
def classified(builder, *args):
    """(scene, classify(scene)): once per scene; the oracle agrees with the numpy reference on it to the byte"""
    scene = getattr(CM, builder)(*args)
    c = CM.classify(scene)
    o16, om = oracle_blend(scene)
    assert np.array_equal(om, c["mask"]) and np.array_equal(o16, c["out"]), (builder, args, int(np.count_nonzero(o16 != c["out"])))
    return scene, c


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("builder,args", SCENES, ids=lambda v: v if isinstance(v, str) else "-".join(map(str, v)))
def test_both_references_agree_and_the_facts_hold(builder, args):
    scene, c = classified(builder, *args)
    f, L0 = scene.facts, c["levels"].get(0, {})
    assert c["kernels"] and c["B"] == scene.B
    if builder == "accumulator_wrap":
        wrapped = sum(sum(L["wrap"].values()) for L in c["levels"].values())
        assert (wrapped == 0) if f["cannot_wrap"] else (wrapped > 0 or f["n"] < 150)
        if f["cannot_wrap_twice"]:
            assert all(L["wrap"]["+2"] == L["wrap"]["-2"] == 0 for L in c["levels"].values())
    elif builder == "acc_extremes":
        acc = c["ref"].lap[0]
        assert all((acc[y, x] == v).all() for (y, x), v in f["sums"].items()) and set(f["sums"].values()) == {32767, -32768}
        assert L0["tier"]["div"] == L0["lanes"] and c["kernels"][-1] == "mb_level0_pk_kernel<false, false, false>"
    elif builder == "count_edges":
        cmap = f["count_map"]
        cnt = sum((m & 1).astype(np.int64) for _, m, _ in scene.feeds)
        assert np.array_equal(cnt, cmap) and f["counts"] == sorted({0, 1, 2, 3, 15, 16, 17, f["n"]} & set(range(f["n"] + 1)))
        if f["n"] <= CM.PACKED_IMAGES:
            assert {k: L0["tier"][k] for k in f["tiers"]} == f["tiers"] and L0["count_max"] == f["n"]
            # the limit sits between every two pixels of a strip, between two strips and between the two rows
            for lo, hi in CM.count_pairs(f["n"]):
                if lo != hi:
                    cols = {x % 8 for y, x in np.argwhere((cmap[:, :-1] == lo) & (cmap[:, 1:] == hi))}
                    assert cols == set(range(8)), (lo, hi, cols)
                    assert ((cmap[0::2] == lo) & (cmap[1::2] == hi)).any() and ((cmap[0::2] == hi) & (cmap[1::2] == lo)).any()
        else:
            assert not c["levels"] and c["kernels"][-1] == "mb_level_kernel<true>"
    elif builder in ("grey_bytes", "grey_wide"):
        assert not c["flags"]["pk_ok"] and L0["tier"]["deferred"] == len(f["deferred"]) and L0["defer"]["segments"] == f["segments"]
        assert sum(v for k, v in L0["defer"]["per_wave"].items() if isinstance(k, int) and k) == len({(y, x // CM.LANES) for y, x in f["deferred"]})
        if builder == "grey_wide":
            assert L0["defer"]["tile_columns"] == f["tile_columns"] == CM.DEFER_SEGS + 1
    elif builder == "collapse_overshoot":
        L = c["levels"][f["level"] - 1]["collapse"]
        if f["tap"]:
            assert L["tap_max"] == f["tap"] and (sum(L["wide"]) == 0) == f["packed"]
            assert L["at_limit"][min(f["tap"], CM.TAP_LIMIT + 1)] > 0 or f["tap"] > CM.TAP_LIMIT + 1
        if f["one_plane"]:
            assert L["wide"][0] > 0 and L["wide"][1:] == [0, 0] and L["one_plane"] == L["wide"][0]
    elif builder == "launch_matrix" and f.get("saturates"):
        assert c["out"].max() == 32767 and max(int(v.max()) for v in c["ref"].norm) < 32767  # reached by the collapse's add alone
    elif builder == "up_borders":
        assert c["levels"][0]["lanes"] == (CM.UP_H // 2) * (args[0] // 8) and f["coarse_w"] == args[0] // 2 and c["B"] == args[1]
    elif builder == "occupancy_edges":
        assert not scene.feeds[f["zero_index"]][1].any() and all(L["search"]["hit"] < L["search"]["rect"] for L in c["levels"].values())


# ---------------------------------------------------------------------------------------------------------------------------------
# every path, by name
# ---------------------------------------------------------------------------------------------------------------------------------
def _lv(c, lv):
    return c["levels"][lv]


@functools.lru_cache(maxsize=None)
def sharded_kernels(case, exchange):
    """the kernels of both ranks' blenders for CM.sharded(case), from the product's own plan (pure geometry: no GPU)"""
    from stitching_amd.distributed import ShardPlan, make_shard_blender, owners_contiguous

    scene = CM.sharded(case)
    corners, sizes = [c for _, _, c in scene.feeds], [(m.shape[1], m.shape[0]) for _, m, _ in scene.feeds]
    owners = owners_contiguous(len(corners), scene.facts["world"])
    plan = ShardPlan(corners, sizes, owners, scene.facts["world"], make_shard_blender(None, scene.roi, scene.bands), exchange, False)
    assert plan.num_bands == scene.B and len(plan.messages) == 2 and {m[2] for m in plan.messages} == {0, 1}
    per_rank, prof = CM.expected_sharded(scene, owners, plan.messages, exchange)
    return [k for rank in per_rank for k in rank], prof


def _sharded(case, exchange, name):
    return lambda c: sharded_kernels(case, exchange)[0].count(name)


def _kernel(name):
    return lambda c: sum(k == name for k in c["kernels"])


def _ballots(n, lv=0):
    return lambda c: (_lv(c, lv)["search"]["ballots"] == n) * _lv(c, lv)["search"]["hits_in_ballot"][-1]


PATHS = [
    # the collapse: packed and its 32-bit fallback, on both sides of the limit, at level 0 and in mb_level_pk_kernel
    ("level 0 collapse packed, largest tap 500", ("collapse_overshoot", "l1_500"), lambda c: _lv(c, 0)["collapse"]["at_limit"][500] * (sum(_lv(c, 0)["collapse"]["wide"]) == 0)),
    ("level 0 collapse 32-bit, largest tap 501", ("collapse_overshoot", "l1_501"), lambda c: _lv(c, 0)["collapse"]["at_limit"][501] * (sum(_lv(c, 0)["collapse"]["wide"]) > 0)),
    ("level 0 collapse 32-bit in one plane of three", ("collapse_overshoot", "l1_501_one_plane"), lambda c: _lv(c, 0)["collapse"]["one_plane"]),
    ("level 1 collapse packed, largest tap 500", ("collapse_overshoot", "l2_500"), lambda c: _lv(c, 1)["collapse"]["at_limit"][500] * (sum(_lv(c, 1)["collapse"]["wide"]) == 0)),
    ("level 1 collapse 32-bit, largest tap 501", ("collapse_overshoot", "l2_501"), lambda c: _lv(c, 1)["collapse"]["at_limit"][501] * (sum(_lv(c, 1)["collapse"]["wide"]) > 0)),
    ("level 0 collapse packed with negative taps", ("collapse_overshoot", "neg"), lambda c: int(_lv(c, 0)["collapse"]["tap_min"] < -300)),
    # the accumulators
    ("level 0 sums pass +32767", ("accumulator_wrap", 255), lambda c: _lv(c, 0)["wrap"]["+1"]),
    ("level 0 sums pass -32768", ("accumulator_wrap", 255), lambda c: _lv(c, 0)["wrap"]["-1"]),
    ("mb_level_pk_kernel sums pass +32767", ("accumulator_wrap", 255), lambda c: _lv(c, 1)["wrap"]["+1"]),
    ("mb_level_pk_kernel sums pass -32768", ("accumulator_wrap", 255), lambda c: _lv(c, 1)["wrap"]["-1"]),
    ("mb_level_fast_kernel sums go round twice", ("accumulator_wrap", 255, "big"), lambda c: _lv(c, 1)["wrap"]["+2"] + _lv(c, 1)["wrap"]["-2"]),
    # the normalisation tiers and their limits inside one patch
    ("tier a - sign(a)", ("count_edges", 255), lambda c: _lv(c, 0)["tier"]["sign"]),
    ("tier shift", ("count_edges", 255), lambda c: _lv(c, 0)["tier"]["shift"]),
    ("tier reciprocal", ("count_edges", 255), lambda c: _lv(c, 0)["tier"]["rcp"]),
    ("tier division", ("count_edges", 255), lambda c: _lv(c, 0)["tier"]["div"]),
    ("a patch on 1 | 2", ("count_edges", 255), lambda c: _lv(c, 0)["straddle"]["1|2"]),
    ("a patch on 2 | 3", ("count_edges", 255), lambda c: _lv(c, 0)["straddle"]["2|3"]),
    ("a patch on 15 | 16", ("count_edges", 255), lambda c: _lv(c, 0)["straddle"]["15|16"]),
    ("a patch on 254 | 255", ("count_edges", 255), lambda c: _lv(c, 0)["straddle"]["254|255"]),
    ("sums that are exact positive multiples of the count", ("count_edges", 17), lambda c: _lv(c, 0)["exact"]["+"]),
    ("sums that are exact negative multiples of the count", ("count_edges", 17), lambda c: _lv(c, 0)["exact"]["-"]),
    ("positive sums one above a multiple of the count", ("count_edges", 17), lambda c: _lv(c, 0)["off_by_one"]["+above"]),
    ("positive sums one below a multiple of the count", ("count_edges", 17), lambda c: _lv(c, 0)["off_by_one"]["+below"]),
    ("negative sums one above a multiple of the count", ("count_edges", 17), lambda c: _lv(c, 0)["off_by_one"]["-above"]),
    ("negative sums one below a multiple of the count", ("count_edges", 17), lambda c: _lv(c, 0)["off_by_one"]["-below"]),
    ("a sum exactly on 32767", ("acc_extremes",), lambda c: _lv(c, 0)["acc_extremes"]["max"]),
    ("a sum exactly on -32768, wrapped from 32768 and unwrapped", ("acc_extremes",), lambda c: _lv(c, 0)["acc_extremes"]["min"] * _lv(c, 0)["wrap"]["+1"]),
    ("a count of 255 in a byte counter", ("count_edges", 255), lambda c: int(_lv(c, 0)["count_max"] == 255)),
    ("mb_level_pk_kernel tier a - sign(a)", ("occupancy_edges", 1040, "middle"), lambda c: _lv(c, 1)["tier"]["sign"]),
    ("mb_level_pk_kernel tier division", ("occupancy_edges", 1040, "middle"), lambda c: _lv(c, 1)["tier"]["div"]),
    ("mb_level_pk_kernel all-ones image visit", ("occupancy_edges", 1040, "middle"), lambda c: _lv(c, 1)["weights"]["ones"]),
    ("mb_level_pk_kernel general image visit", ("occupancy_edges", 1040, "middle"), lambda c: _lv(c, 1)["weights"]["general"]),
    # the image counts
    # (a wavefront asks 64 images per ballot; the count is the hits the LAST ballot returns, 0 unless the ballots are as many as named)
    ("search in one ballot, all 63 lanes of it", ("count_edges", 63), _ballots(1)),
    ("search in one ballot, all 64 lanes of it", ("count_edges", 64), _ballots(1)),
    ("search in two ballots, image 64 alone in the second", ("count_edges", 65), _ballots(2)),
    ("search in two full ballots (128)", ("count_edges", 128), _ballots(2)),
    ("search in three ballots, image 128 alone in the third", ("count_edges", 129), _ballots(3)),
    ("search in four ballots (255)", ("count_edges", 255), _ballots(4)),
    ("mb_level_pk_kernel search in four ballots (255)", ("count_edges", 255), _ballots(4, 1)),
    ("256 images: the generic kernels at every level below the coarse launch, no packed level", ("count_edges", 256),
     lambda c: int(not c["levels"] and c["kernels"][-2:] == ["mb_level_kernel<false>", "mb_level_kernel<true>"])),
    ("255 images: the packed kernels", ("count_edges", 255), lambda c: int(c["kernels"][-2:] == ["mb_level_pk_kernel<false>", "mb_level0_pk_kernel<false, false, false>"])),
    # the level-0 pyrDown
    ("run interior", ("down0_runs", False), lambda c: c["down0"]["runs"]["interior"]),
    ("run mirrored in the left border", ("down0_runs", False), lambda c: c["down0"]["runs"]["mirrored left"]),
    ("run mirrored in the right border", ("down0_runs", False), lambda c: c["down0"]["runs"]["mirrored right"]),
    ("run that meets a border", ("down0_runs", False), lambda c: c["down0"]["runs"]["border"]),
    ("interior run with a0 = 0", ("down0_runs", False), lambda c: c["down0"]["limits"]["interior a0 = 0"]),
    ("interior run with a0 + 10 = iw - 1", ("down0_runs", False), lambda c: c["down0"]["limits"]["interior a0 + 10 = iw - 1"]),
    ("run with a0 = -1", ("down0_runs", False), lambda c: c["down0"]["limits"]["a0 = -1"]),
    ("run with a0 + 10 = iw", ("down0_runs", False), lambda c: c["down0"]["limits"]["a0 + 10 = iw"]),
    ("mirrored run with s_low = 0", ("down0_runs", False), lambda c: c["down0"]["limits"]["s_low = 0"]),
    ("mirrored run with s_low + 10 = iw - 1", ("down0_runs", False), lambda c: c["down0"]["limits"]["s_low + 10 = iw - 1"]),
    ("first run the mirror fails for, left", ("down0_runs", False), lambda c: c["down0"]["limits"]["mirror fails left"]),
    ("first run the mirror fails for, right", ("down0_runs", False), lambda c: c["down0"]["limits"]["mirror fails right"]),
    ("the mirror fails by one column", ("down0_runs", False), lambda c: c["down0"]["limits"]["mirror fails by one"]),
    ("image more than one mirror image from its border (!NEAR)", ("down0_runs", False), lambda c: c["down0"]["near"]["far"]),
    ("NEAR", ("down0_runs", False), lambda c: c["down0"]["near"]["near"]),
    ("NEAR at its limit", ("occupancy_edges", 512, "middle"), lambda c: c["down0"]["limits"]["near at its limit"]),
    ("rows by = -1, 0, ih - 1, ih", ("down0_runs", False), lambda c: min(c["down0"]["limits"][k] for k in ("by = -1", "by = 0", "by = ih - 1", "by = ih"))),
    ("mask sums packed in a launch that is not declared binary", ("down0_runs", True), lambda c: c["down0"]["mask_sums"]["packed"]),
    ("mask sums fp32 for one grey byte", ("down0_runs", True), lambda c: c["down0"]["mask_sums"]["fp32"]),
    ("grey in byte 0 of a run", ("grey_bytes", "run_bytes", 1), lambda c: c["down0"]["limits"]["grey in byte 0"]),
    ("grey in byte 10 of a run", ("grey_bytes", "run_bytes", 1), lambda c: c["down0"]["limits"]["grey in byte 10"]),
    ("grey in byte 11 of a run only: packed", ("grey_bytes", "run_bytes", 1), lambda c: c["down0"]["limits"]["grey in byte 11 only"]),
    ("whole launch packed although not declared binary", ("grey_bytes", "views", 254), lambda c: c["down0"]["mask_sums"]["packed"] * ("fp32" not in c["down0"]["mask_sums"])),
    # mb_down0_lds_kernel's batched branch (its own mirrored picks and grey ballot) against the task loop
    ("pyrDown tile columns in the task loop (dn_task_level0)", ("down0_runs", False), lambda c: c["down0"]["waves"]["task loop"] * ("batched" not in c["down0"]["waves"])),
    ("batched pyrDown tile columns", ("down0_batched", False), lambda c: c["down0"]["waves"]["batched"]),
    ("mirrored runs in a batched tile column", ("down0_batched", False), lambda c: c["down0"]["waves"]["batched: mirrored runs"]),
    ("interior runs in a batched tile column", ("down0_batched", False), lambda c: c["down0"]["waves"]["batched: interior runs"]),
    ("the batched branch's ballot: packed", ("down0_batched", True), lambda c: c["down0"]["mask_sums"]["batched packed"]),
    ("the batched branch's ballot: fp32 for one grey byte", ("down0_batched", True), lambda c: c["down0"]["mask_sums"]["batched fp32"]),
    # deferral
    ("lane 0 the only deferred lane", ("grey_bytes", "lane0_px0", 1), lambda c: _lv(c, 0)["defer"]["per_wave"].get("only lane 0", 0)),
    ("lane 63 the only deferred lane", ("grey_bytes", "lane63_px7", 254), lambda c: _lv(c, 0)["defer"]["per_wave"].get("only lane 63", 0)),
    ("all 64 lanes deferred", ("grey_bytes", "all64", 1), lambda c: _lv(c, 0)["defer"]["per_wave"].get(64, 0)),
    ("no lane deferred in the launch", ("grey_bytes", "views", 254), lambda c: int(_lv(c, 0)["tier"]["deferred"] == 0 and _kernel("mb_level0_deferred_kernel")(c) == 1)),
    ("a segment with 64 entries", ("grey_bytes", "n64", 127), lambda c: int(_lv(c, 0)["defer"]["segments"] == {0: 64})),
    ("a segment with 65 entries", ("grey_bytes", "n65", 128), lambda c: int(_lv(c, 0)["defer"]["segments"] == {0: 65})),
    ("tile columns 0 and 256 share a segment", ("grey_wide",), lambda c: int(_lv(c, 0)["defer"]["segments"] == {0: 2} and _lv(c, 0)["defer"]["tile_columns"] == 257)),
    # pyrUp borders
    ("first strip is the last strip (coarse width 4)", ("up_borders", 8, 3), lambda c: _lv(c, 0)["lanes"]),
    ("coarse width 8", ("up_borders", 16, 3), lambda c: _lv(c, 0)["lanes"]),
    ("mb_level_pk_kernel: first strip is the last strip (level 1 of 4 bands, 8 columns)", ("up_borders", 16, 4),
     lambda c: _lv(c, 1)["lanes"] * (c["ref"].finished[1].shape[1] == 8) * _kernel("mb_level_pk_kernel<false>")(c)),
    # the image search
    ("an image the occupancy map keeps out of a tile, level 0", ("occupancy_edges", 1040, "middle"), lambda c: _lv(c, 0)["search"]["rect"] - _lv(c, 0)["search"]["hit"]),
    ("an image the occupancy map keeps out of a tile, level 1", ("occupancy_edges", 1040, "middle"), lambda c: _lv(c, 1)["search"]["rect"] - _lv(c, 1)["search"]["hit"]),
    # the launches (stx_fast_mb_down_batch: six; stx_fast_mb_level: those the public entry points reach without strips, see test_gpu)
    ("mb_down0_lds_kernel<true, true>", ("launch_matrix", "bands3"), _kernel("mb_down0_lds_kernel<true, true>")),
    ("mb_down0_lds_kernel<false, true>", ("launch_matrix", "grey"), _kernel("mb_down0_lds_kernel<false, true>")),
    ("mb_down_lds_kernel<true>", ("launch_matrix", "bands5"), _kernel("mb_down_lds_kernel<true>")),
    ("mb_down0_kernel<true> (int16 image)", ("launch_matrix", "mixed_s16"), _kernel("mb_down0_kernel<true>")),
    ("mb_coarse_kernel", ("launch_matrix", "bands3"), _kernel("mb_coarse_kernel")),
    ("mb_level0_pk_kernel<false, false, false>", ("launch_matrix", "bands3"), _kernel("mb_level0_pk_kernel<false, false, false>")),
    ("mb_level0_pk_kernel<false, true, false> + mb_level0_deferred_kernel", ("launch_matrix", "grey"), _kernel("mb_level0_deferred_kernel")),
    ("mb_level_pk_kernel<false>", ("launch_matrix", "bands5"), _kernel("mb_level_pk_kernel<false>")),
    ("mb_level_fast_kernel<false, false, false, false>", ("launch_matrix", "mixed_s16"), _kernel("mb_level_fast_kernel<false, false, false, false>")),
    ("mb_level_kernel<true> under int16 images", ("launch_matrix", "all_s16"), _kernel("mb_level_kernel<true>")),
    ("mb_level_kernel<false>: fewer than three bands", ("launch_matrix", "bands2"), _kernel("mb_level_kernel<false>")),
    ("no pyramid at all: 0 bands", ("launch_matrix", "bands0"), lambda c: int(c["kernels"] == ["mb_level_kernel<true>"])),
    # strips, contributions and emit: two ranks' blenders (expected_sharded over the product's ShardPlan)
    ("mb_level0_pk_kernel<true>: binary contributions", ("sharded", "binary"), _sharded("binary", "contribs", "mb_level0_pk_kernel<true>")),
    ("mb_level_fast_kernel<true, true, false, false>: a contribution beside a grey mask", ("sharded", "grey"), _sharded("grey", "contribs", "mb_level_fast_kernel<true, true, false, false>")),
    ("mb_level_fast_kernel<false, true, false, true>", ("sharded", "binary"), _sharded("binary", "contribs", "mb_level_fast_kernel<false, true, false, true>")),
    ("mb_level_fast_kernel<false, true, false, false>: an int16 image beside a contribution", ("sharded", "s16"), _sharded("s16", "contribs", "mb_level_fast_kernel<false, true, false, false>")),
    ("mb_emit_multi_kernel<true, false>", ("sharded", "binary"), _sharded("binary", "contribs", "mb_emit_multi_kernel<true, false>")),
    ("mb_emit_multi_kernel<false, true>", ("sharded", "binary"), _sharded("binary", "contribs", "mb_emit_multi_kernel<false, true>")),
    ("mb_emit_multi_kernel<false, false>: an int16 image exported", ("sharded", "s16"), _sharded("s16", "contribs", "mb_emit_multi_kernel<false, false>")),
    ("generic emit, level 0 of an int16 image", ("sharded", "s16"), _sharded("s16", "contribs", "mb_level_kernel<true> (emit)")),
    ("generic emit, the three coarsest levels", ("sharded", "binary"), _sharded("binary", "contribs", "mb_level_kernel<false> (emit)")),
    ("received image strips: the launches of fed images, deferral on both ranks", ("sharded", "grey"), _sharded("grey", "strips", "mb_level0_deferred_kernel")),
]


def test_every_path_is_reached_by_a_named_family(capsys):
    lines = []
    for name, (builder, *args), count in PATHS:
        n = int(count(classified(builder, *args)[1]))
        lines.append("%-70s %-40s %d" % (name, builder + str(tuple(args)), n))
        assert n >= 1, (name, builder, args)
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    # the launches of a kept rig: the REPLAY and WEIGHTS = false instantiations
    k = CM.expected_launches(CM.launch_matrix("bands5"), adopted=True)
    assert k[0].count("mb_level_pk_kernel<true>") == 2 and "mb_level0_pk_kernel<false, false, true>" in k[0] and k[2] == 3
    assert "mb_down0_lds_kernel<true, false>" in k[0] and k[0].count("mb_down_lds_kernel<false>") == 4
    g = CM.expected_launches(CM.launch_matrix("grey"), adopted=True)
    assert "mb_level0_pk_kernel<false, true, true>" in g[0] and "mb_down0_lds_kernel<false, false>" in g[0] and g[2] == 3
    assert CM.expected_launches(CM.count_edges(65), adopted=True)[2] == 0 and CM.expected_launches(CM.count_edges(64), adopted=True)[2] == 2


# ---------------------------------------------------------------------------------------------------------------------------------
# what the older tests' inputs reach
# ---------------------------------------------------------------------------------------------------------------------------------
def _many_images(n):
    """the feeds of test_gpu_parity.test_blend_many_images_over_the_same_pixels (the generator both share)"""
    return CM.Scene(5, list(zip(*helpers.many_images_feeds(n))), {})


def _sparse_masks(kind):
    """the feeds of test_gpu_parity.test_blend_sparse_masks_bit_exact (the mask generator both share), warped by the oracle"""
    imgs, cams = helpers.small_ring(4, 1500, 420, span=150.0)
    rng = np.random.default_rng(31)
    kept = {}

    def fn(masks, corners, sizes):
        kept["masks"] = helpers.sparse_masks(kind, masks, rng)
        return kept["masks"]

    o = helpers.run_pipeline(O.Warper, O.Blender, imgs, cams, blend_strength=6, masks_fn=fn)
    return CM.Scene(o["blender"].blender.num_bands(), list(zip(o["w_imgs"], kept["masks"], o["corners"])), {})


def test_what_the_older_inputs_reach(capsys):
    """classify() over the inputs of the two hand-made parity tests: which paths of PATHS' kinds they reach and which they do not.
    The figures are recorded in profiles/constructed_multiband.md; asserted here is the gap the constructed families close"""
    lines = []
    for name, scene in (("many images n = 40", _many_images(40)), ("sparse masks, grey_islands", _sparse_masks("grey_islands"))):
        c = CM.classify(scene)
        lines.append(name + ": B %d, %s" % (c["B"], c["kernels"]))
        lines.append("  down0 %s" % c["down0"])
        for lv, L in c["levels"].items():
            lines.append("  level %d: %s" % (lv, {k: v for k, v in L.items()}))
            assert sum(L["collapse"]["wide"]) == 0 and abs(L["collapse"]["tap_max"]) < 400 and sum(L["wrap"].values()) == 0
        assert c["down0"]["near"].get("far", 0) == 0
        if "defer" in c["levels"].get(0, {}):
            pw = c["levels"][0]["defer"]["per_wave"]
            assert 64 not in pw and "only lane 63" not in pw and max(c["levels"][0]["defer"]["segments"].values(), default=0) != 64
    with capsys.disabled():
        print("\n" + "\n".join(lines))


# ---------------------------------------------------------------------------------------------------------------------------------
# the variants: one mistake each
# ---------------------------------------------------------------------------------------------------------------------------------
def _round_short(f):
    return NB.wrap16(np.rint(np.asarray(f, np.float32).astype(np.float64)).astype(np.int64))


class VariantMultiBand(NB.NumpyMultiBand):
    """NumpyMultiBand.feed and .blend restated with knobs; every default is the contract"""

    def __init__(self, num_bands, add=NB.wrap16, eps=NB.EPS, prod=NB.trunc_short, quot=NB.trunc_short, collapse=NB.sat16, up_left=1,
                 img_border="symmetric", down_mode="mirror", weight_border="constant", scale=1.0 / 255.0, grey=lambda m: m):
        super().__init__(num_bands)
        self.k = dict(add=add, eps=np.float32(eps), prod=prod, quot=quot, collapse=collapse, up_left=up_left, img_border=img_border,
                      down_mode=down_mode, weight_border=weight_border, scale=np.float32(scale), grey=grey)

    def _down16(self, a):
        t = ndimage.correlate1d(a.astype(np.int64), NB.K5, axis=0, mode=self.k["down_mode"])
        t = ndimage.correlate1d(t, NB.K5, axis=1, mode=self.k["down_mode"])
        return ((t[::2, ::2] + 128) >> 8).astype(np.int16)

    def _up_axis(self, a, axis):
        a = np.moveaxis(a.astype(np.int64), axis, 0)
        n = a.shape[0]
        left = a[self.k["up_left"]:self.k["up_left"] + 1] if n > 1 else a[0:1]
        ext = np.concatenate([left, a, a[n - 1:n]], axis=0)
        z = np.zeros((2 * (n + 2),) + a.shape[1:], np.int64)
        z[::2] = ext
        t = ndimage.correlate1d(z, NB.K5, axis=0, mode="constant", cval=0)
        return np.moveaxis(t[2:2 + 2 * n], 0, axis)

    def _up16(self, a):
        return ((self._up_axis(self._up_axis(a, 0), 1) + 32) >> 6).astype(np.int16)

    def feed(self, img16, mask, tl):
        B, k = self.B, self.k
        ih, iw = mask.shape
        (fx, fy, fw, fh), (left, top) = CM.feed_rect(B, self.roi, iw, ih, tl)
        pad = ((top, fh - top - ih), (left, fw - left - iw))
        g = [np.pad(np.asarray(img16, np.int16), pad + ((0, 0),), mode=k["img_border"])]
        w0 = k["grey"](np.asarray(mask, np.uint8)).astype(np.float32) * k["scale"]
        wt = [np.pad(w0, pad, mode=k["weight_border"])]
        for _ in range(B):
            g.append(self._down16(g[-1]))
            wt.append(NB.pyr_down_32f(wt[-1]))
        lap = [NB.sat16(g[i].astype(np.int32) - self._up16(g[i + 1]).astype(np.int32)) for i in range(B)] + [g[B]]
        x0, y0, x1, y1 = fx, fy, fx + fw, fy + fh
        for i in range(B + 1):
            prod = k["prod"]((lap[i].astype(np.float32) * wt[i][:, :, None]).astype(np.float32))
            d = self.lap[i][y0:y1, x0:x1]
            d[...] = k["add"](d.astype(np.int64) + prod.astype(np.int64))
            self.wts[i][y0:y1, x0:x1] = (self.wts[i][y0:y1, x0:x1] + wt[i]).astype(np.float32)
            x0, y0, x1, y1 = x0 // 2, y0 // 2, x1 // 2, y1 // 2

    def blend(self):
        B, k = self.B, self.k
        with np.errstate(divide="ignore", invalid="ignore"):  # (eps = 0: 0 / 0 where no image is)
            lv = [k["quot"]((self.lap[i].astype(np.float32) / (self.wts[i] + k["eps"])[:, :, None]).astype(np.float32)) for i in range(B + 1)]
        for i in range(B, 0, -1):
            lv[i - 1] = k["collapse"](self._up16(lv[i]).astype(np.int64) + lv[i - 1].astype(np.int64))
        w, h = self.final
        out = lv[0][:h, :w].copy()
        m = np.where(self.wts[0][:h, :w] > NB.EPS, 255, 0).astype(np.uint8)
        out[m == 0] = 0
        return out, m


def _variant(scene, reverse=False, **kw):
    b = VariantMultiBand(scene.bands, **kw)
    b.prepare(scene.roi)
    for img, mask, corner in (reversed(scene.feeds) if reverse else scene.feeds):
        b.feed(np.asarray(img).astype(np.int16), mask, corner)
    return b.blend()


def _contract(builder, *args):
    scene, c = classified(builder, *args)
    return scene, (c["out"], c["mask"])


def test_the_restated_blender_is_the_contract_when_nothing_is_altered():
    for key in (("down0_runs", True), ("up_borders", 8, 3), ("accumulator_wrap", 150), ("launch_matrix", "all_s16"), ("occupancy_edges", 520, "first")):
        scene, want = _contract(*key)
        assert _same(want, _variant(scene)), key


VARIANTS = [
    ("saturating accumulator", dict(add=NB.sat16), [("accumulator_wrap", 150), ("accumulator_wrap", 255)]),
    ("division without the 1e-5", dict(eps=0.0), [("count_edges", 2), ("count_edges", 17)]),
    ("rounded product", dict(prod=_round_short), [("occupancy_edges", 520, "middle")]),
    ("rounded quotient", dict(quot=_round_short), [("count_edges", 3)]),
    ("wrapping collapse add", dict(collapse=NB.wrap16), [("launch_matrix", "s16_overshoot")]),
    ("pyrUp border -1 -> 0", dict(up_left=0), [("up_borders", 8, 3), ("up_borders", 16, 3), ("up_borders", 40, 3), ("up_borders", 16, 4)]),
    ("REFLECT_101 around the image", dict(img_border="reflect"), [("down0_runs", False)]),
    ("REFLECT in pyrDown", dict(down_mode="reflect"), [("down0_runs", False)]),
    ("reflected weight border", dict(weight_border="symmetric"), [("down0_runs", False)]),
    ("weights as m / 256", dict(scale=1.0 / 256.0), [("grey_bytes", "lane0_px0", 127), ("grey_bytes", "views", 254)]),
    ("a grey byte taken for 255", dict(grey=lambda m: np.where(m != 0, 255, 0).astype(np.uint8)), [("grey_bytes", "lane0_px0", 127), ("grey_bytes", "run_bytes", 1)]),
]


@pytest.mark.parametrize("name,knobs,keys", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_each_variant_is_caught_by_its_family(name, knobs, keys):
    for key in keys:
        scene, want = _contract(*key)
        got = _variant(scene, **knobs)
        assert not _same(want, got), (name, key)


def test_feed_order_shows_where_fp32_weight_sums_are_rounded():
    """int16 wrap-around is associative and every product is truncated on its own, so the order of the images shows only in the fp32
    sums of weights that are no dyadic fractions: grey masks.  With binary masks it does not show at all"""
    scene, want = _contract("feed_order")
    back = _variant(scene, reverse=True)
    assert np.array_equal(want[1], back[1]) and np.count_nonzero(want[0] != back[0]) >= 1
    scene, want = _contract("count_edges", 255)
    assert _same(want, _variant(scene, reverse=True))


def test_a_mask_test_against_0_cannot_be_told_from_the_one_against_1e_5():
    """the panorama mask is W_0 > 1e-5 and W_0 sums mask bytes / 255: its smallest non-zero value is 1 / 255"""
    scene, c = classified("grey_bytes", "lane0_px0", 1)
    w0 = c["ref"].wts[0]
    assert w0[w0 > 0].min() >= np.float32(1.0 / 255.0) * np.float32(0.999) > NB.EPS and np.array_equal(w0 > 0, w0 > NB.EPS)


# ---------------------------------------------------------------------------------------------------------------------------------
# the arithmetic claims of the kernels' comments
# ---------------------------------------------------------------------------------------------------------------------------------
def test_the_packed_collapse_stays_inside_int16_up_to_taps_of_500_and_how_far_beyond():
    """up_patch_pks_math: HE = t + 6 t + t (|.| <= 8 T), then HE + 6 HE + HE + 32 (|.| <= 64 T + 32) before the shift: inside int16 for
    |t| <= T as long as 64 T + 32 <= 32767, i.e. T <= 511 — the kernel's limit of 500 has 11 to spare; a tap of 512 is the first that
    leaves int16 (all 18 taps equal)"""
    def worst(t):
        he = t + 6 * t + t
        ho = t + t
        return max(abs(he), abs(he + 6 * he + he + 32), abs(he + 6 * he + he - 32) if t < 0 else 0, abs(ho + 6 * ho + ho + 8), abs(he + he + 8), abs(ho + ho + 2))
    assert all(worst(t) <= 32767 and worst(-t) <= 32768 for t in range(CM.TAP_LIMIT + 1))
    first = next(t for t in range(CM.TAP_LIMIT, 1000) if worst(t) > 32767)
    assert first == 512 and 64 * 511 + 32 == 32736


def test_the_sign_and_shift_forms_equal_the_division_for_every_int16_sum():
    a = np.arange(-32768, 32768, dtype=np.int64)
    for n in (1, 2):
        want = NB.trunc_short((a.astype(np.float32) / (np.float32(n) + NB.EPS)).astype(np.float32)).astype(np.int64)
        s = a - np.sign(a)                        # a - sign(a)
        neg = (s < 0).astype(np.int64)
        got = s if n == 1 else (s + neg) >> 1     # towards zero
        assert np.array_equal(got, want), n


def test_byte_counters_of_255_images_do_not_carry():
    """cntb: four counters per register, += 0x01010101 per covering image; and cnt + 1 in the 16-bit pair layout of the tier test"""
    c = 0
    for k in range(1, CM.PACKED_IMAGES + 1):
        c += 0x01010101
        assert c <= 0xFFFFFFFF and [(c >> s) & 0xFF for s in (0, 8, 16, 24)] == [k] * 4
    assert c == 0xFFFFFFFF and [((c + 0x01010101) >> s) & 0xFF for s in (0, 8, 16, 24)] == [0, 1, 1, 1]  # the 256th image carries
    assert 0x00FF00FF + 0x00010001 == 0x01000100  # counts of 255 plus one: no carry from the low half into the high
