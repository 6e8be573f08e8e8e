"""The constructed input families (tests/constructed_inputs.py) on the MI355X: every family through S.ColorSeamEstimator().find,
S.SeamEstimator("voronoi").find or largest_interior_rectangle, byte for byte (and tuple for tuple) against the numpy contracts.  What
each family reaches, and that it tells the contract from a subtly wrong variant, is asserted without a GPU in
tests/test_constructed_inputs.py; here only the device is asked."""
import itertools

import numpy as np
import pytest

import stitching_amd as S
from stitching_amd.cropper import largest_interior_rectangle
from tests import constructed_inputs as CI
from tests import numpy_color_seams as ZC
from tests import numpy_lir as ZL
from tests import numpy_seams as ZS

pytestmark = pytest.mark.gpu


def _find(est, want, corners, imgs, masks):
    """est.find against `want`, 0 differing bytes; the inputs come back unmodified"""
    before_m, before_i = [m.copy() for m in masks], [a.copy() for a in imgs]
    got = est.find(imgs, corners, masks)
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert isinstance(g, np.ndarray) and g.dtype == np.uint8 and g.shape == w.shape
        assert np.array_equal(g, w), (k, int(np.count_nonzero(g != w)))
    assert all(np.array_equal(m, b) for m, b in zip(masks, before_m)) and all(np.array_equal(a, b) for a, b in zip(imgs, before_i))
    return est


def _color(corners, imgs, masks, pairs=1, levels=1):
    est = _find(S.ColorSeamEstimator(), ZC.find(imgs, corners, masks), corners, imgs, masks)
    assert est.info["pairs"] == pairs and est.info["levels"] == levels
    return est


def _voronoi(corners, imgs, masks, pairs=1, levels=1):
    est = _find(S.SeamEstimator("voronoi"), ZS.find("voronoi", corners, masks), corners, imgs, masks)
    assert est.info["pairs"] == pairs and est.info["levels"] == levels
    return est


def _lir(mask, dev=None):
    before = mask.copy()
    xywh, counts, _ = largest_interior_rectangle(mask if dev is None else dev)
    assert xywh == ZL.lir(mask), (mask.shape, xywh, ZL.lir(mask))
    assert counts == ZL.single_contour(mask), (mask.shape, counts, ZL.single_contour(mask))
    assert np.array_equal(mask, before)
    return xywh, counts


def _pitched(a, ctx, fill):
    """`a` as a view into a larger device buffer whose surroundings hold `fill`.  -> (view, check): check() reads the whole buffer
    back and asserts that neither the view nor its surroundings changed"""
    big = np.full((a.shape[0] + 9, a.shape[1] + 13) + a.shape[2:], fill, a.dtype)
    big[5:5 + a.shape[0], 7:7 + a.shape[1]] = a
    dev = S.DeviceImage.from_numpy(big, ctx)

    def check():
        assert np.array_equal(dev.numpy(), big)

    return dev[5:5 + a.shape[0], 7:7 + a.shape[1]], check


# ---------------------------------------------------------------------------------------------------------------------------------
# colour seams
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", CI.ZIGZAG_L)
def test_zigzag_walk_back_over_the_whole_window(gpu_ctx, L):
    """the seam moves one column per row: the walk-back window's outermost columns, steps that start on t = 0 and t = W - 1"""
    for case in (c for c in CI.zigzag_cover() if c[0] == L):
        corners, imgs, masks, _ = CI.zigzag_pair(*case)
        _color(corners, imgs, masks)


def test_zigzag_as_pitched_views(gpu_ctx):
    for case in ((200, 70, False, False), (129, 65, True, True)):
        corners, imgs, masks, _ = CI.zigzag_pair(*case)
        want = ZC.find(imgs, corners, masks)
        views = [_pitched(a, gpu_ctx, 200) for a in imgs] + [_pitched(m, gpu_ctx, 255) for m in masks]
        est = S.ColorSeamEstimator()
        got = est.find([v for v, _ in views[:2]], corners, [v for v, _ in views[2:]])
        assert all(isinstance(g, S.DeviceImage) and np.array_equal(g.numpy(), w) for g, w in zip(got, want))
        assert est.info["pairs"] == 1 and est.info["levels"] == 1
        for _, check in views:  # the inputs and what surrounds them in their buffers come back unmodified
            check()


@pytest.mark.parametrize("W,jog", ((3, 0), (5, 0), (3, -1), (5, 1)))
def test_accumulators_on_both_sides_of_2_31(gpu_ctx, W, jog):
    """L = 16384: the final arg-min (jog 0), `right < best` (jog -1) and `left < best` (jog +1) compare u32 values across 2^31"""
    corners, imgs, masks, f = CI.saturated_pair(W, jog)
    assert f["seam_sum"] < 2 ** 31 <= f["neighbour_sum"]
    _color(corners, imgs, masks)


def test_tie_between_the_diagonals_on_the_seam(gpu_ctx):
    for transpose in (False, True):
        _color(*CI.fork_pair(transpose)[:3])


def test_one_launch_for_pairs_of_very_different_shape(gpu_ctx):
    corners, imgs, masks, f = CI.mixed_level()
    _color(corners, imgs, masks, pairs=len(f["pairs"]), levels=f["nlevels"])
    _voronoi(corners, imgs, masks, pairs=len(f["pairs"]), levels=f["nlevels"])


# ---------------------------------------------------------------------------------------------------------------------------------
# voronoi
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rw", CI.RAGGED_RW)
def test_ragged_masks(gpu_ctx, rw):
    """windows of 255 .. 257, 511 .. 513 and 620 columns, roi heights around the column sweeps' batches of 8, three densities"""
    for rh, density in itertools.product(CI.RAGGED_RH, CI.RAGGED_DENSITY):
        _voronoi(*CI.ragged_pair(rw, rh, density, 0)[:3])


def test_far_sources_rows_without_a_source_and_ties(gpu_ctx):
    _voronoi(*CI.far_source_pair()[:3])
    _voronoi(*CI.tie_pair()[:3])


# ---------------------------------------------------------------------------------------------------------------------------------
# largest interior rectangle
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CI.PROFILES)
def test_histogram_masks(gpu_ctx, name):
    """nearest-smaller walks across many lanes' chunks, pointers in LDS (up to 4864 wide) and in the global scratch slice"""
    for W, anchor in itertools.product(CI.HISTOGRAM_W, ("bottom", "top")):
        _lir(CI.histogram_mask(name, W, anchor=anchor)[0])


def test_histogram_mask_as_a_pitched_view(gpu_ctx):
    for name, W in (("descending", 4865), ("tent", 700)):
        mask, _ = CI.histogram_mask(name, W, anchor="top")
        view, check = _pitched(mask, gpu_ctx, 255)
        _lir(mask, view)
        check()


def test_notched_mask_grid_stride_and_global_scratch(gpu_ctx):
    mask, f = CI.notched_mask()
    assert f["grid_stride"] and not f["in_lds"]
    assert _lir(mask)[1] == (1, f["notches"])


def test_contour_masks(gpu_ctx):
    """label chains 1e4 .. 1e5 long, exact component and hole counts"""
    for mask, f in (CI.spiral_mask(), CI.spiral_mask(closed=True), CI.serpentine_mask(), CI.rings_mask(50, 201), CI.rings_mask(50, 198),
                    CI.rings_mask(50, 197), CI.diagonal_mask(), CI.diagonal_mask(complement=True)):
        assert _lir(mask)[1] == f["counts"]
