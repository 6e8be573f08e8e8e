"""Seam finding without a GPU: known answers of the restatement (tests/numpy_seams.py), its distance against scipy's, the host-only C
entry stx_seam_schedule (levels run in any order inside a level give the sequential result) and the seam-estimator switch."""
import sys
import types

import numpy as np
import pytest

import stitching_amd as S
from stitching_amd import config
from stitching_amd.seam_estimation import schedule
from tests import numpy_seams as Z


def _full(w, h, v=255):
    return np.full((h, w), v, np.uint8)


# ---------------------------------------------------------------------------------------------------------------------------------
# restatement known answers
# ---------------------------------------------------------------------------------------------------------------------------------
def test_overlap_roi_and_pair_order():
    assert Z.overlap_roi((0, 0), (10, 4), (6, 1), (10, 4)) == (6, 1, 4, 3)
    assert Z.overlap_roi((0, 0), (5, 5), (5, 0), (5, 5)) is None  # touching is not overlapping
    sizes = [(10, 4)] * 3
    assert [(i, j) for i, j, _ in Z.pairs([(0, 0), (100, 0), (5, 0)], sizes)] == [(0, 2)]
    assert [(i, j) for i, j, _ in Z.pairs([(0, 0), (0, 0), (0, 0)], sizes)] == [(0, 1), (0, 2), (1, 2)]


def test_two_rectangles_seam_column_and_tie():
    """A at x in [0, 10), B at [7, 17): the roi is x in [7, 10).  A's unique pixels end at x = 6, B's begin at x = 10:
    dist1 = x - 6, dist2 = 10 - x -> x = 7: 1 < 3 (A keeps), x = 8: 2 == 2 (a tie: B keeps), x = 9: 3 > 1 (B keeps)."""
    a, b = _full(10, 4), _full(10, 4)
    out = Z.find("voronoi", [(0, 0), (7, 0)], [a, b])
    assert np.all(out[0][:, :8] == 255) and np.all(out[0][:, 8:] == 0)
    assert np.all(out[1][:, 0] == 0) and np.all(out[1][:, 1:] == 255)
    assert np.all(a == 255) and np.all(b == 255)  # inputs untouched
    # one column further apart: no tie, A keeps x = 7, 8 of the roi [6, 10)
    out = Z.find("voronoi", [(0, 0), (6, 0)], [a, b])
    assert np.all(out[0][:, :8] == 255) and np.all(out[0][:, 8:] == 0)
    assert np.all(out[1][:, :2] == 0) and np.all(out[1][:, 2:] == 255)


def test_identical_masks_go_to_image_j():
    """No unique pixel on either side: both distances are 8192, never strictly smaller, so mask i is zeroed over the roi."""
    m = _full(8, 6)
    out = Z.find("voronoi", [(3, 2), (3, 2)], [m, m])
    assert np.all(out[0] == 0) and np.all(out[1] == 255)


def test_mask_inside_the_other():
    """B's mask lies inside A's: B has no unique pixel (dist2 = 8192 everywhere), A has: A takes the whole roi."""
    a = _full(8, 8)
    b = np.zeros((8, 8), np.uint8)
    b[2:6, 2:6] = 255
    out = Z.find("voronoi", [(0, 0), (0, 0)], [a, b])
    assert np.all(out[0] == 255) and np.all(out[1] == 0)
    # an image inside the other with full masks: the same
    out = Z.find("voronoi", [(0, 0), (2, 2)], [a, _full(4, 4)])
    assert np.all(out[0] == 255) and np.all(out[1] == 0)


def test_grey_values_are_kept_and_count_as_set():
    a, b = _full(10, 4, 254), _full(10, 4, 128)
    b[0, 9] = 1
    out = Z.find("voronoi", [(0, 0), (7, 0)], [a, b])
    assert np.all(out[0][:, :8] == 254) and np.all(out[0][:, 8:] == 0)
    assert np.all(out[1][:, 0] == 0) and np.all(out[1][:, 1:9] == 128) and out[1][0, 9] == 1


def test_non_overlapping_pairs_stay_untouched():
    rng = np.random.default_rng(3)
    ms = [(rng.random((5, 5)) < 0.7).astype(np.uint8) * 255 for _ in range(3)]
    out = Z.find("voronoi", [(0, 0), (5, 0), (0, 5)], ms)  # within the gap of each other, but no overlap
    assert all(np.array_equal(o, m) for o, m in zip(out, ms))


def test_negative_corners_give_the_same_seam():
    a, b = _full(10, 4), _full(10, 4)
    want = Z.find("voronoi", [(0, 0), (7, 0)], [a, b])
    got = Z.find("voronoi", [(-1000, -37), (-993, -37)], [a, b])
    assert all(np.array_equal(x, y) for x, y in zip(got, want))


def test_three_images_depend_on_pair_order():
    """A at x in [0, 3), B and C at [1, 4), one row.  (0, 1): A keeps x = 1 (1 < 2), B keeps x = 2 (2 > 1).  (0, 2): A is left with x = 0,
    1, so x = 1 ties (1 == 1, C keeps) and x = 2 is C's alone.  (1, 2): B has no unique pixel left: C keeps everything.  Run in reverse
    order, A keeps x = 1 and C loses x = 1."""
    ms = [_full(3, 1), _full(3, 1), _full(3, 1)]
    corners = [(0, 0), (1, 0), (1, 0)]
    out = Z.find("voronoi", corners, ms)
    assert out[0].tolist() == [[255, 0, 0]] and out[1].tolist() == [[0, 0, 0]] and out[2].tolist() == [[255, 255, 255]]
    rev = [m.copy() for m in ms]
    for i, j, roi in reversed(Z.pairs(corners, [(3, 1)] * 3)):
        Z.find_in_pair(rev, corners, i, j, roi)
    assert rev[0].tolist() == [[255, 255, 0]] and rev[2].tolist() == [[0, 255, 255]]


def test_saturation_at_8192():
    """A 9000-wide overlap: A's one unique column is at x = 0, B has no unique pixel (8192 everywhere).  Up to x = 8191 dist1 < 8192 (B is
    zeroed), from x = 8192 on dist1 saturates at 8192, a tie: A is zeroed."""
    w = 9000
    a, b = _full(w, 2), _full(w, 2)
    b[:, 0] = 0
    out = Z.find("voronoi", [(0, 0), (0, 0)], [a, b])
    assert np.all(out[0][:, :8192] == 255) and np.all(out[0][:, 8192:] == 0)
    assert np.all(out[1][:, :8192] == 0) and np.all(out[1][:, 8192:] == 255)
    d = Z.l1_distance(np.pad(np.ones((2, 1), bool), ((0, 0), (0, w))))
    assert d[0, 8191] == 8191 and d[0, 8192] == 8192 and d.max() == 8192


def test_no_returns_copies():
    ms = [_full(4, 3, 7), _full(5, 2)]
    out = Z.find("no", [(0, 0), (1, 1)], ms)
    assert all(np.array_equal(o, m) and o is not m for o, m in zip(out, ms))


@pytest.mark.parametrize("seed", range(6))
def test_distance_against_scipy(seed):
    from scipy import ndimage

    rng = np.random.default_rng(seed)
    h, w = rng.integers(1, 60, 2)
    src = rng.random((h, w)) < [0.0, 0.002, 0.02, 0.2, 0.6, 0.97][seed]
    want = ndimage.distance_transform_cdt(~src, metric="taxicab").astype(np.int64)
    want = np.where(want < 0, Z.DIST_SAT, np.minimum(want, Z.DIST_SAT)) if src.any() else np.full((h, w), Z.DIST_SAT)
    assert np.array_equal(Z.l1_distance(src), want)


# ---------------------------------------------------------------------------------------------------------------------------------
# host schedule (no GPU)
# ---------------------------------------------------------------------------------------------------------------------------------
def _layout(rng, n):
    sizes = [(int(rng.integers(5, 40)), int(rng.integers(5, 30))) for _ in range(n)]
    corners = [(int(rng.integers(-20, 60)), int(rng.integers(-15, 40))) for _ in range(n)]
    masks = [((rng.random((h, w)) < 0.85) * rng.choice([255, 254, 90], (h, w))).astype(np.uint8) for w, h in sizes]
    return corners, sizes, masks


def test_schedule_matches_the_pair_list():
    rng = np.random.default_rng(0)
    corners, sizes, _ = _layout(rng, 9)
    pairs, levels = schedule(corners, sizes)
    assert [tuple(p) for p in pairs.tolist()] == [(i, j) + roi for i, j, roi in Z.pairs(corners, sizes)]
    assert len(levels) == len(pairs) and (levels >= 0).all()
    assert schedule([], [])[0].shape == (0, 6)


@pytest.mark.parametrize("seed", range(12))
def test_levels_in_any_order_give_the_sequential_result(seed):
    rng = np.random.default_rng(100 + seed)
    corners, sizes, masks = _layout(rng, int(rng.integers(2, 10)))
    want = Z.find("voronoi", corners, masks)
    pairs, levels = schedule(corners, sizes)
    for how in ("reversed", "shuffled"):
        out = [m.copy() for m in masks]
        for lev in range(int(levels.max()) + 1 if len(levels) else 0):
            idx = [k for k in range(len(pairs)) if levels[k] == lev]
            idx = idx[::-1] if how == "reversed" else list(rng.permutation(idx))
            for k in idx:
                i, j, x, y, w, h = pairs[k].tolist()
                Z.find_in_pair(out, corners, i, j, (x, y, w, h))
        assert all(np.array_equal(a, b) for a, b in zip(out, want)), how


def test_schedule_levels_of_a_chain_and_of_far_pairs():
    # a chain of images 30 wide, 18 apart: neighbouring rois are 6 apart, within the gap -> every pair a level of its own
    sizes = [(30, 10)] * 4
    _, levels = schedule([(18 * k, 0) for k in range(4)], sizes)
    assert levels.tolist() == [0, 1, 2]
    # 40 apart with 50-wide images: rois 30 apart, more than the gap -> one level
    _, levels = schedule([(40 * k, 0) for k in range(4)], [(50, 10)] * 4)
    assert levels.tolist() == [0, 0, 0]


def test_schedule_rejects_bad_arguments():
    with pytest.raises(S.StitchingError):
        schedule([(0, 0)], [(0, 5)])


# ---------------------------------------------------------------------------------------------------------------------------------
# the switch
# ---------------------------------------------------------------------------------------------------------------------------------
def _fake_cv2():
    cv = types.ModuleType("cv2")

    class _Finder:
        def __init__(self, *a):
            self.arg = a

        def find(self, imgs, corners, masks):
            return masks

    cv.detail_DpSeamFinder = cv.detail_GraphCutSeamFinder = _Finder
    cv.detail = types.SimpleNamespace(SeamFinder_VORONOI_SEAM=2, SeamFinder_NO=0, SeamFinder_createDefault=lambda k: _Finder(k))
    return cv, _Finder


def test_switch_default_is_opencv(monkeypatch):
    monkeypatch.delenv("STITCHING_AMD_SEAM_ESTIMATOR", raising=False)
    monkeypatch.setattr(config, "_seam_estimator", None)
    assert S.seam_estimator() == "opencv"
    monkeypatch.setitem(sys.modules, "cv2", None)  # no OpenCV
    f = S.SeamFinder("voronoi")
    assert f.finder is None
    with pytest.raises(S.StitchingError, match="pass an estimator= object"):
        f.find([], [], [])


def test_switch_env_var(monkeypatch):
    for val, want in (("device", "device"), ("opencv", "opencv"), ("", "opencv")):
        monkeypatch.setattr(config, "_seam_estimator", None)
        monkeypatch.setenv("STITCHING_AMD_SEAM_ESTIMATOR", val)
        assert S.seam_estimator() == want
    monkeypatch.setattr(config, "_seam_estimator", None)
    monkeypatch.setenv("STITCHING_AMD_SEAM_ESTIMATOR", "cuda")
    with pytest.raises(S.StitchingError):
        S.seam_estimator()
    monkeypatch.setattr(config, "_seam_estimator", "opencv")
    with pytest.raises(S.StitchingError):
        S.set_seam_estimator("bogus")
    assert S.set_seam_estimator("device") == "opencv" and S.seam_estimator() == "device"


def test_switch_builds_the_device_finder_for_voronoi_and_no(monkeypatch):
    cv, finder_cls = _fake_cv2()
    monkeypatch.setitem(sys.modules, "cv2", cv)
    monkeypatch.setattr(config, "_seam_estimator", "device")
    for name in ("voronoi", "no"):
        f = S.SeamFinder(name)
        assert isinstance(f.finder, S.SeamEstimator) and f.finder.kind == name
    for name in ("dp_color", "dp_colorgrad", "gc_color", "gc_colorgrad"):
        assert isinstance(S.SeamFinder(name).finder, finder_cls)
    own = object()
    assert S.SeamFinder("voronoi", estimator=own).finder is own
    # "opencv": the cv.detail objects, as before
    monkeypatch.setattr(config, "_seam_estimator", "opencv")
    for name in S.SeamFinder.SEAM_FINDER_CHOICES:
        assert isinstance(S.SeamFinder(name).finder, finder_cls)


def test_switch_dp_without_cv2_names_the_device_finders(monkeypatch):
    monkeypatch.setitem(sys.modules, "cv2", None)
    monkeypatch.setattr(config, "_seam_estimator", "device")
    f = S.SeamFinder("dp_color")
    assert f.finder is None
    with pytest.raises(S.StitchingError, match="'voronoi' and 'no'"):
        f.find([], [], [])
    assert isinstance(S.SeamFinder("no").finder, S.SeamEstimator)


def test_estimator_rejects_bad_arguments():
    with pytest.raises(S.StitchingError):
        S.SeamEstimator("dp_color")
    est = S.SeamEstimator("voronoi")
    assert est.find([], [], []) == [] and est.info["pairs"] == 0
    img, m = np.zeros((4, 5, 3), np.uint8), _full(5, 4)
    with pytest.raises(S.StitchingError):
        est.find([img], [(0, 0), (1, 1)], [m])
    with pytest.raises(S.StitchingError, match="its image"):
        est.find([img], [(0, 0)], [_full(6, 4)])
    with pytest.raises(S.StitchingError, match="u8"):
        est.find([img], [(0, 0)], [m.astype(np.float32)])
    with pytest.raises(S.StitchingError, match="u8"):
        est.find([img], [(0, 0)], [np.zeros((4, 5, 3), np.uint8)])
