"""The constructed blend families (tests/constructed_blends.py) without a GPU: the constants they are shaped around are the ones in the
sources, every family's stated facts hold against BOTH CPU references (the oracle's blender handle, OpenCV's algorithm restated in
C++, and tests/numpy_blenders.py, scipy), which agree bit for bit, and each family tells the contract from a plausibly wrong variant.

The variants below are restatements with ONE mistake each, of the kind the kernels of csrc/stx_blend.hip can carry unnoticed; they live
here, are numpy only and are never imported by the product:

  variant                                                        family that tells it from the contract
  column pass: the zero rows of column j taken from column j^1   1 chunk edges
  column pass: a link that looks one chunk away only             2 far links
  no cap | a cap of 8191                                         3 column cap ("top", "bottom")
  row pass: the carry dropped at a step edge                     4 row steps (forward: lone zero "first", backward: "last")
  row pass: the rows of a workgroup share its first row's result 5 LDS rows (where a workgroup has 2 or 4 rows)
  pixels outside the image count as zero                         7 views
  gathers: an outside pixel of a partial group contributes       8 placement (feather and "no")
  feather: saturating adds                                       10 accumulator wrap (all three)
  feather: weights summed in another order                       11 weight sum order
  "no": the first fed image wins | the mask of the winner        12 "no" stack (binary and grey)
  "no": the early exit fires with one lane still undecided       12 "no" stack (binary: the hole)
  "no": the early exit fires although a mask is grey             12 "no" stack (grey)
Nothing here provokes a fault: these are host computations."""
import os
import re

import numpy as np
import pytest

from oracle import oracle as O
from stitching_amd import _lib
from tests import constructed_blends as CB
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
    internal, hip, host = _src("stx_internal.h"), _src("stx_blend.hip"), _src("stx_blend_host.cpp")
    hip = hip[hip.index("constexpr int DT_INF"):]  # the distance transform's constants and, below them, the feather and "no" blenders
    assert CB.CHUNK_ROWS == _int(r"constexpr\s+int\s+STX_DT_RC\s*=\s*(\d+)\s*;", internal)
    assert re.search(r"constexpr\s+int\s+DT_RC\s*=\s*STX_DT_RC\s*;", hip)
    hip = hip[hip.index("Feather blender as a deferred gather"):]
    assert CB.CAP == _int(r"constexpr\s+int\s+STX_FEATHER_DIST_CAP\s*=\s*(\d+)\s*;", internal)
    assert CB.ROW_GROUP == _int(r"constexpr\s+int\s+DT_RW\s*=\s*(\d+)\s*;", hip)
    # the column pass: 8 rows at a time, two halves of 32, 4 columns per lane, 64 lanes
    assert CB.BITSET_ROWS == _int(r"for \(int g = 0; g < (\d+); g\+\+\)", hip) == _int(r"for \(int r = 0; r < (\d+); r\+\+\)", hip)
    assert CB.HALF_ROWS == _int(r"for \(int rr = 0; rr < (\d+); rr\+\+\)", hip) and 2 * CB.HALF_ROWS == CB.CHUNK_ROWS
    assert len(re.findall(r"const int x = \(blockIdx\.x \* 64 \+ threadIdx\.x\) \* %d[,;]" % CB.COL_GROUP, hip)) == 3
    assert len(re.findall(r"dim3\(\(max_w \+ 255\) / 256, (?:max_chunks, )?n\), dim3\(64\)", hip)) == 3
    # the row pass: a step is 64 lanes of DT_RW pixels; LDS per row from the one expression launcher and feed check share
    assert re.search(r"const int nseg = \(P\.w \+ 64 \* DT_RW - 1\) / \(64 \* DT_RW\);", hip) and CB.ROW_STEP == 64 * CB.ROW_GROUP
    assert CB.LDS_BYTES == _int(r"constexpr\s+int\s+STX_FEATHER_LDS_BYTES\s*=\s*(\d+)\s*;", internal)
    m = re.search(r"constexpr int stx_feather_lds_pitch\(int w\) \{ return \(\(w \+ (\d+)\) / (\d+)\) \* (\d+); \}", internal)
    assert m and [int(v) for v in m.groups()] == [CB.ROW_STEP - 1, CB.ROW_STEP, CB.ROW_STEP // CB.ROW_GROUP]
    assert re.findall(r"stx_feather_lds_pitch\(w\) \* 16(?: \* (\d))? <= STX_FEATHER_LDS_BYTES \? (\d)", internal) == [("4", "4"), ("2", "2"), ("", "1")]
    assert re.search(r"const int lds_pitch = stx_feather_lds_pitch\(max_w\);\s*const int rows = stx_feather_rows_per_block\(max_w\);", hip)
    assert re.search(r"dim3\(\(max_h \+ rows - 1\) / rows, n\), dim3\(256\), \(size_t\)lds_pitch \* 16 \* rows,", hip)
    assert re.search(r"if \(b->kind == STX_BLEND_FEATHER\) STX_TRY\(stx_feather_refuse_width\(img->w\)\);", host)
    assert re.search(r"inline int stx_feather_refuse_width\(int w\)\s*\{\s*if \(stx_feather_rows_per_block\(w\) > 0\) return STX_OK;", internal)
    assert [CB.rows_per_block(w) for w in (1, 8192, 8193, 16384, 16385, 32768, 32769)] == [4, 4, 2, 2, 1, 1, 0]
    assert CB.LDS_WIDTHS[2] == _int(r"#define STX_FEATHER_MAX_WIDTH (\d+)", open(os.path.join(ROOT, "include", "stitching_amd.h")).read())
    # the gathers: 256 columns x 4 rows per workgroup, 4 columns per lane
    assert len(re.findall(r"const dim3 grid\(\(K\.w \+ %d\) / %d, \(K\.h \+ %d\) / %d\);" % (CB.SPAN_COLS - 1, CB.SPAN_COLS, CB.SPAN_ROWS - 1, CB.SPAN_ROWS), hip)) == 2
    assert len(re.findall(r"const int x4 = \(blockIdx\.x \* 64 \+ \(threadIdx\.x & 63\)\) \* %d;" % CB.COL_GROUP, hip)) == 2
    assert (CB.NO, CB.FEATHER) == (_lib.BLEND_NO, _lib.BLEND_FEATHER) == (O._OracleBlenderHandle.NO, O._OracleBlenderHandle.FEATHER)
    # the shapes lie around them
    assert {CB.CHUNK_ROWS * k + d for k in (1, 2) for d in (-1, 0, 1)} | {CB.HALF_ROWS + d for d in (-1, 0, 1)} | {CB.BITSET_ROWS + d for d in (-1, 0, 1)} <= set(CB.CHUNK_EDGE_H)
    assert {CB.ROW_STEP * k + d for k in (1, 2) for d in (-1, 0, 1)} | {CB.ROW_GROUP * k + d for k in (1, 2) for d in (-1, 0, 1)} <= set(CB.ROW_STEP_W)
    assert {CB.LDS_WIDTHS[0], CB.LDS_WIDTHS[0] + 1, CB.LDS_WIDTHS[1], CB.LDS_WIDTHS[1] + 1, CB.LDS_WIDTHS[2]} == set(CB.LDS_W)
    assert CB.COLUMN_CAP_H > CB.CAP + CB.CHUNK_ROWS and (CB.LONE_W - 1) // CB.ROW_STEP == 3
    assert {CB.SPAN_COLS + d for d in (-3, -2, -1, 0, 1)} <= set(CB.PLACE_X) and {w % CB.COL_GROUP for w in CB.PLACE_PANO_W} == {0, 1, 2, 3}


def test_the_probe_table_is_strictly_increasing():
    """the int16 panorama under a probe pair names the distance: 0, 1, 5, 9, ... 16380, 16381, 16382, steps of at least 1"""
    t = CB.PROBE_TABLE
    assert len(t) == CB.CAP + 1 and list(t[:4]) == [0, 1, 5, 9] and list(t[-3:]) == [16380, 16381, 16382]
    assert np.diff(t).min() == 1
    assert np.array_equal(CB.probe_decode(t[:, None, None].repeat(3, 2).astype(np.int16))[:, 0], np.arange(CB.CAP + 1))
    assert np.diff(CB.probe_value(np.arange(CB.CAP + 1), sharpness=2.0 ** -13)).min() >= 1
    # not with another value, nor with u8 values: so 32767 it is
    assert np.diff(CB.probe_value(np.arange(CB.CAP + 1), value=30000)).min() <= 0
    assert np.diff(CB.probe_value(np.arange(CB.CAP + 1), value=255)).min() <= 0


# ---------------------------------------------------------------------------------------------------------------------------------
# the two references
# ---------------------------------------------------------------------------------------------------------------------------------
def oracle_blend(scene):
    b = O._OracleBlenderHandle(scene.kind, 0, scene.sharpness)
    b.prepare(scene.roi)
    for img, mask, corner in scene.feeds:
        b.feed(np.asarray(img).astype(np.int16), mask, corner)
    return b.blend()


def numpy_blend(scene, blender=None):
    b = blender or (NB.NumpyFeather(scene.sharpness) if scene.kind == CB.FEATHER else NB.NumpyNo())
    b.prepare(scene.roi)
    for img, mask, corner in scene.feeds:
        b.feed(np.asarray(img).astype(np.int16), mask, corner)
    return b.blend()


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def contract(scene):
    """the oracle's (int16 panorama, mask); numpy_blenders agrees with it bit for bit, and the probe's facts hold"""
    got = oracle_blend(scene)
    assert _same(got, numpy_blend(scene))
    if scene.facts.get("probe"):
        d = CB.probe_decode(got[0])
        assert d.min() >= 0
        for want, corner, (_, mask, _) in zip(scene.facts["dist"], scene.facts["corners"], scene.feeds[::2]):
            x0, y0 = corner[0] - scene.roi[0], corner[1] - scene.roi[1]
            if want is not None:
                assert np.array_equal(d[y0:y0 + mask.shape[0], x0:x0 + mask.shape[1]], want)
        for (y, x), v in scene.facts.get("at", {}).items():
            assert d[y, x] == v
        for (y, x), v in scene.facts.get("would_be", {}).items():
            assert v > CB.CAP == d[y, x]
    return got


# ---------------------------------------------------------------------------------------------------------------------------------
# the variants: one mistake each
# ---------------------------------------------------------------------------------------------------------------------------------
BIG = 1 << 28


def column_pass(mask, swap=False, near_only=False, cap=CB.CAP):
    """per pixel the distance to the nearest zero of its own column.  swap: the zero rows of column j are those of column j ^ 1
    (none past the image) | near_only: zero rows more than one chunk away are not seen"""
    z = np.asarray(mask) == 0
    h, w = z.shape
    if swap:
        z = np.stack([z[:, j ^ 1] if (j ^ 1) < w else np.zeros(h, bool) for j in range(w)], axis=1)
    rows = np.arange(h)[:, None]
    last = np.maximum.accumulate(np.where(z, rows, -BIG), axis=0)
    nxt = np.minimum.accumulate(np.where(z, rows, BIG)[::-1], axis=0)[::-1]
    if near_only:
        last = np.where(rows // CB.CHUNK_ROWS - last // CB.CHUNK_ROWS <= 1, last, -BIG)
        nxt = np.where(nxt // CB.CHUNK_ROWS - rows // CB.CHUNK_ROWS <= 1, nxt, BIG)
    return np.minimum(np.minimum(rows - last, nxt - rows), cap)


def _running_min(a, step):
    """inclusive running minimum along the rows of `a`, from the left; step: restarted at every multiple of it"""
    if not step:
        return np.minimum.accumulate(a, axis=1)
    h, w = a.shape
    p = np.pad(a, ((0, 0), (0, -w % step)), constant_values=BIG).reshape(h, -1, step)
    return np.minimum.accumulate(p, axis=2).reshape(h, -1)[:, :w]


def row_pass(g, cap=CB.CAP, drop=None, share=1):
    """min over x' of g[x'] + |x - x'|, saturated.  drop: "forward" / "backward": that sweep's carry is lost at every step edge |
    share: rows y of a workgroup of `share` rows all get the result of its first row"""
    h, w = g.shape
    x = np.arange(w)[None, :]
    fwd = _running_min(g - x, CB.ROW_STEP if drop == "forward" else 0) + x
    flipped = (fwd + x)[:, ::-1]
    if drop == "backward":  # the steps are cut from column 0, not from the right end
        pad = -w % CB.ROW_STEP
        flipped = np.pad(flipped, ((0, 0), (pad, 0)), constant_values=BIG)
        back = _running_min(flipped, CB.ROW_STEP)[:, pad:]
    else:
        back = _running_min(flipped, 0)
    d = np.minimum(back[:, ::-1] - x, cap)
    return d[np.arange(h) // share * share] if share > 1 else d


def two_pass(mask, col={}, row={}, cap=CB.CAP):
    """the distance transform as the kernels cut it: columns, then rows.  cap: another saturation value where a zero is too far (a
    mask without any zero is "no zero anywhere", CB.CAP, whatever the cap: that is the transform's starting value)"""
    if np.asarray(mask).all():
        return np.full(np.shape(mask), CB.CAP, np.int64)
    return row_pass(column_pass(mask, cap=cap, **col), cap=cap, **row)


def outside_is_zero(mask):
    return two_pass(np.pad(mask, 1))[1:-1, 1:-1]


def _spill(roi, arrays, tl):
    """the image's columns widened to whole lane groups of the panorama (edge pixels repeated), inside the roi"""
    x0 = tl[0] - roi[0]
    w = arrays[0].shape[1]
    left = x0 % CB.COL_GROUP
    right = min(-(x0 + w) % CB.COL_GROUP, roi[2] - (x0 + w))
    return [np.pad(a, ((0, 0), (left, right)) + ((0, 0),) * (a.ndim - 2), mode="edge") for a in arrays], (tl[0] - left, tl[1])


class VariantFeather(NB.NumpyFeather):
    """NumpyFeather.feed restated with: dist: another distance transform | add: another int16 add | spill: the pixels of a partial
    lane group that lie outside the image contribute"""

    def __init__(self, sharpness, dist=two_pass, add=NB.wrap16, spill=False):
        super().__init__(sharpness)
        self.dist, self.add, self.spill = dist, add, spill

    def feed(self, img16, mask, tl):
        wgt = np.minimum((self.dist(np.asarray(mask, np.uint8)).astype(np.float32) * self.sharpness).astype(np.float32), np.float32(1.0))
        img16 = np.asarray(img16, np.int16)
        if self.spill:
            (img16, wgt), tl = _spill(self.roi, [img16, wgt], tl)
        x0, y0 = tl[0] - self.roi[0], tl[1] - self.roi[1]
        h, w = wgt.shape
        d = self.dst[y0:y0 + h, x0:x0 + w]
        prod = NB.trunc_short((img16.astype(np.float32) * wgt[:, :, None]).astype(np.float32))
        d[...] = self.add(d.astype(np.int64) + prod.astype(np.int64))
        self.w[y0:y0 + h, x0:x0 + w] = (self.w[y0:y0 + h, x0:x0 + w] + wgt).astype(np.float32)


class VariantNo(NB.NumpyNo):
    """NumpyNo.feed restated with: first_wins: a pixel keeps the first image whose mask is set | winner_mask: the panorama's mask is
    the mask of the image that gave the pixel, not the OR | spill: as above"""

    def __init__(self, first_wins=False, winner_mask=False, spill=False):
        self.first_wins, self.winner_mask, self.spill = first_wins, winner_mask, spill

    def feed(self, img16, mask, tl):
        img16, mask = np.asarray(img16, np.int16), np.asarray(mask, np.uint8)
        if self.spill:
            (img16, mask), tl = _spill(self.roi, [img16, mask], tl)
        x0, y0 = tl[0] - self.roi[0], tl[1] - self.roi[1]
        h, w = mask.shape
        d, dm = self.dst[y0:y0 + h, x0:x0 + w], self.m[y0:y0 + h, x0:x0 + w]
        take = (mask != 0) & (dm == 0) if self.first_wins else mask != 0
        d[take] = img16[take]
        if self.winner_mask:
            dm[take] = mask[take]
        else:
            dm |= mask


def no_gather_walk(scene, short=0, trust_binary=False):
    """the "no" blender as no_gather_kernel walks it: per row and 256-column span the images from the last fed backwards; a pixel takes
    the first set mask it meets, the masks are ORed; where every mask is binary the walk of a span ends once all its pixels are
    decided.  short: it ends with up to that many lane groups still undecided | trust_binary: it ends so although a mask is grey"""
    x0, y0, w, h = scene.roi
    out, macc, decided = np.zeros((h, w, 3), np.int16), np.zeros((h, w), np.uint8), np.zeros((h, w), bool)
    binary = trust_binary or all(np.isin(m, (0, 255)).all() for _, m, _ in scene.feeds)
    for y in range(h):
        for s0 in range(0, w, CB.SPAN_COLS):
            s1 = min(s0 + CB.SPAN_COLS, w)
            for img, mask, (cx, cy) in reversed(scene.feeds):
                ly, a, b = y - (cy - y0), max(s0, cx - x0), min(s1, cx - x0 + mask.shape[1])
                if not 0 <= ly < mask.shape[0] or a >= b:
                    continue
                undecided = ~decided[y, s0:s1]
                groups = np.add.reduceat(undecided, np.arange(0, s1 - s0, CB.COL_GROUP)) > 0
                if binary and groups.sum() <= short:
                    break
                m = mask[ly, a - (cx - x0):b - (cx - x0)]
                take = (m != 0) & ~decided[y, a:b]
                out[y, a:b][take] = np.asarray(img, np.int16)[ly, a - (cx - x0):b - (cx - x0)][take]
                macc[y, a:b] |= m
                decided[y, a:b] |= take
    return out, macc


def _variant(scene, **kw):
    return numpy_blend(scene, VariantFeather(scene.sharpness, **kw) if scene.kind == CB.FEATHER else VariantNo(**kw))


def _dist(**kw):
    return lambda mask: two_pass(mask, **kw)


def test_the_restated_feeds_are_the_contract_when_nothing_is_altered():
    for scene in (CB.chunk_edges(129, 2), CB.far_links("both"), CB.row_steps(1025, 3), CB.views("half"), CB.ones_path(),
                  CB.accumulator_wrap("border"), CB.placement(CB.NO, np.int16, 259), CB.no_stack(1, np.uint8)):
        assert _same(contract(scene), _variant(scene))


# ---------------------------------------------------------------------------------------------------------------------------------
# the families
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", CB.CHUNK_EDGE_H)
def test_chunk_edges(h):
    killed = 0
    for rot in range(len(CB.CHUNK_EDGE_ROWS)):
        scene = CB.chunk_edges(h, rot)
        assert all(r < h for r in scene.facts["zero_rows"].values())
        want = contract(scene)
        killed += not _same(want, _variant(scene, dist=_dist(col=dict(swap=True))))
    assert killed >= (1 if h == 1 else len(CB.CHUNK_EDGE_ROWS) - 1)


@pytest.mark.parametrize("where", CB.FAR_LINK_WHERE)
def test_far_links(where):
    scene = CB.far_links(where)
    assert len(scene.facts["empty_chunks"]) >= 4 and (where != "both" or scene.facts["empty_chunks"] == [1, 2, 3, 4])
    assert not _same(contract(scene), _variant(scene, dist=_dist(col=dict(near_only=True))))


@pytest.mark.parametrize("where", CB.COLUMN_CAP_WHERE)
def test_column_cap(where):
    scene = CB.column_cap(where)
    want = contract(scene)
    no_cap, cap_8191 = _variant(scene, dist=_dist(cap=65535)), _variant(scene, dist=_dist(cap=CB.CAP - 1))
    if where == "both":  # every pixel within 4134 steps of a zero: the cap acts inside the column pass only, the result hides it
        assert scene.facts["dist"][0].max() < CB.CAP - 1 and _same(want, no_cap) and _same(want, cap_8191)
    else:
        assert not _same(want, no_cap) and not _same(want, cap_8191)


@pytest.mark.parametrize("w", CB.ROW_STEP_W)
def test_row_steps(w):
    killed = {"forward": 0, "backward": 0}
    for rot in range(len(CB.ROW_STEP_COLS)):
        scene = CB.row_steps(w, rot)
        assert all(c < w for c in scene.facts["zero_cols"].values())
        want = contract(scene)
        for drop in killed:
            killed[drop] += not _same(want, _variant(scene, dist=_dist(row=dict(drop=drop))))
    # told apart where a pixel and its nearest zero column lie in different steps: there are such pixels from 513 columns on
    assert all((n > 0) == (w > CB.ROW_STEP) for n in killed.values()), killed


@pytest.mark.parametrize("where", CB.LONE_WHERE)
def test_lone_zero_carries_over_three_step_edges(where):
    scene = CB.lone_zero(where)
    assert scene.facts["step_edges_crossed"] == 3
    want = contract(scene)
    mine, other = ("forward", "backward") if where == "first" else ("backward", "forward")
    assert not _same(want, _variant(scene, dist=_dist(row=dict(drop=mine))))
    assert _same(want, _variant(scene, dist=_dist(row=dict(drop=other))))


@pytest.mark.parametrize("w", CB.LDS_W)
def test_lds_rows(w):
    scene = CB.lds_rows(w)
    rows = scene.facts["rows_per_block"]
    assert rows == {8192: 4, 8193: 2, 16384: 2, 16385: 1, 32768: 1}[w] and scene.facts["workgroups"] == {4: 2, 2: 3, 1: 5}[rows]
    want = contract(scene)
    # the cap of the row pass: the widest image alone has pixels further than 8192 from the zeros in columns 0, w / 2 and w - 1
    assert (scene.facts["dist"][0].max() == CB.CAP) == (w == CB.LDS_WIDTHS[2]) == (not _same(want, _variant(scene, dist=_dist(cap=65535))))
    assert _same(want, _variant(scene, dist=_dist(row=dict(share=rows)))) == (rows == 1)


def test_unequal_batch_every_image_as_alone():
    scene = CB.unequal_batch()
    got = contract(scene)
    for k, (mask, zeros, corner) in enumerate(CB.unequal_masks()):
        alone = contract(CB.probe_scene([mask], [corner], [zeros]))
        x0, y0 = corner[0] - scene.roi[0], corner[1] - scene.roi[1]
        assert np.array_equal(got[0][y0:y0 + mask.shape[0], x0:x0 + mask.shape[1]], alone[0]), k


@pytest.mark.parametrize("density", CB.VIEW_DENSITY)
def test_views(density):
    scene = CB.views(density)
    edge = scene.facts["edge_at_least_2"]
    assert len(edge) >= 100 and (density == "sparse") == (scene.facts["n_zeros"] <= 1000)
    want = contract(scene)
    assert CB.probe_decode(want[0])[edge[:, 0], edge[:, 1]].min() >= 2
    assert outside_is_zero(scene.feeds[0][1])[edge[:, 0], edge[:, 1]].max() == 1
    assert not _same(want, _variant(scene, dist=outside_is_zero))


@pytest.mark.parametrize("pano_w", CB.PLACE_PANO_W)
@pytest.mark.parametrize("dtype", (np.uint8, np.int16))
@pytest.mark.parametrize("kind", (CB.FEATHER, CB.NO))
def test_placement(kind, dtype, pano_w):
    scene = CB.placement(kind, dtype, pano_w)
    assert scene.roi == (0, 0, pano_w, len(scene.facts["spots"])) and scene.facts["tail"] == pano_w % 4
    assert {x for _, x in scene.facts["spots"]} == {x for x in CB.PLACE_X if x < pano_w} and len(scene.feeds) == 1 + len(scene.facts["spots"])
    assert not _same(contract(scene), _variant(scene, spill=True))


def test_ones_path_one_lane_leaves_it():
    scene = CB.ones_path()
    f = scene.facts
    wa = np.minimum(two_pass(scene.feeds[0][1]) * np.float32(scene.sharpness), 1)
    assert sorted(map(tuple, np.argwhere(wa < 1))) == f["below_one"] and f["span"] == 1
    assert {x // CB.COL_GROUP for _, x in f["below_one"]} == {f["lane_group"]}  # one lane, in each of three rows
    assert (two_pass(scene.feeds[1][1]) * np.float32(scene.sharpness) >= 1).all()
    contract(scene)


@pytest.mark.parametrize("which", CB.WRAP_KINDS)
def test_accumulator_wrap(which):
    scene = CB.accumulator_wrap(which)
    want = contract(scene)
    f = scene.facts
    if which == "border":
        assert [s > 32767 for s in f["sums"].values()] == [False, False, True] and f["wraps_at"] == 3
        assert want[0][3, 3, 0] < 0 < want[0][2, 2, 0]
    else:
        assert f["sum"] > 32767 and f["wrapped"] == f["sum"] - 65536 and (want[0][want[1] != 0] == f["value"]).all()
        assert which != "ones" or (O.convert_scale_abs(want[0]) == f["u8"]).all()
    assert not _same(want, _variant(scene, add=NB.sat16))


def test_weight_sum_order():
    scene = CB.weight_sum_order()
    want = contract(scene)
    scene.feeds.reverse()
    back = contract(scene)
    assert np.array_equal(want[1], back[1]) and np.count_nonzero(want[0] != back[0]) >= 1


@pytest.mark.parametrize("dtype", (np.uint8, np.int16))
@pytest.mark.parametrize("grey", (0, 1))
def test_no_stack(grey, dtype):
    scene = CB.no_stack(grey, dtype)
    f = scene.facts
    out, mask = contract(scene)
    hy, hx = f["hole"]
    top = scene.feeds[f["winner_elsewhere"]]
    assert top[1][hy, hx] == 0 and np.count_nonzero(top[1][:, :CB.SPAN_COLS] == 0) == 1
    # the hole: one lane of span 0 has to walk on, down to the image the construction names
    below = scene.feeds[f["winner_hole"]]
    assert all(scene.feeds[k][1][hy, hx] == 0 for k in range(f["winner_hole"] + 1, 5)) and below[1][hy, hx] != 0
    assert mask[hy, hx] == f["mask_hole"] and below[0][hy, hx].any() and np.array_equal(out[hy, hx], below[0][hy, hx].astype(np.int16))
    assert _same((out, mask), no_gather_walk(scene))
    one_short = no_gather_walk(scene, short=1)
    if grey:  # grey masks bar the exit, early or not; an exit that ignores them loses the bits of the images it never reaches
        assert _same((out, mask), one_short) and not _same((out, mask), no_gather_walk(scene, trust_binary=True))
    else:
        assert not one_short[0][hy, hx].any() and one_short[1][hy, hx] == 0 and not _same((out, mask), one_short)
    covered = top[1] != 0
    assert np.array_equal(out[covered], top[0].astype(np.int16)[covered])
    if dtype == np.int16:
        assert (out < 0).any()
    if grey:
        assert (mask[f["grey_only"]] == f["or_of_greys"]).all()
        assert np.array_equal(out[f["grey_only"]], scene.feeds[f["winner_grey_only"]][0].astype(np.int16)[f["grey_only"]])
    else:
        assert set(np.unique(mask)) <= {0, 255}
    assert not _same((out, mask), _variant(scene, first_wins=True))
    assert _same((out, mask), _variant(scene, winner_mask=True)) == (not grey)  # binary masks: OR and winner's mask are both 255
