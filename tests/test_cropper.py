"""The restatement tests/numpy_lir.py (no GPU): known answers of the largest interior rectangle and its tie rule, the fast DP against
the lir_basis restatement and a brute-force enumeration, the contour counts on hand-counted masks, and the reference's rectangle
arithmetic through stitching_amd.Rectangle / Cropper's static helpers."""
import numpy as np
import pytest

import stitching_amd as S
from stitching_amd.cropper import INVALID_CONTOUR
from tests import numpy_lir as Z


def _all(mask):
    a, b = Z.lir(mask), Z.lir_spans(mask)
    assert a == b, (a, b)
    return a


def test_known_answers():
    assert _all(np.ones((4, 6), np.uint8)) == (0, 0, 6, 4)
    one = np.zeros((5, 5), np.uint8)
    one[3, 2] = 255
    assert _all(one) == (2, 3, 1, 1)
    assert _all(np.ones((1, 9), bool)) == (0, 0, 9, 1)
    assert _all(np.ones((9, 1), bool)) == (0, 0, 1, 9)
    assert _all(np.zeros((3, 4), np.uint8)) == (0, 0, 0, 0)
    ell = np.zeros((6, 6), np.uint8)
    ell[:, :2] = 1  # 2 x 6 = 12
    ell[4:, :] = 1  # 6 x 2 = 12: tie, the smaller y wins
    assert _all(ell) == (0, 0, 2, 6)
    ell[:, :2] = 0
    ell[:, 4:] = 1  # right arm (4, 0, 2, 6) and bottom bar (0, 4, 6, 2): smaller y
    assert _all(ell) == (4, 0, 2, 6)


def test_plus_ties():
    plus = np.zeros((7, 7), np.uint8)
    plus[2:5, :] = 1
    plus[:, 2:5] = 1
    # 3 x 7 both ways: the vertical bar (2, 0) has the smaller y
    assert _all(plus) == (2, 0, 3, 7)


def test_staircase_ties():
    # a staircase: equal-area candidates on different rows, columns and widths
    st = np.zeros((6, 6), np.uint8)
    st[0:2, 0:6] = 1  # 6 x 2 = 12
    st[2:4, 0:4] = 1  # 4 x 4 = 16
    st[4:6, 0:2] = 1  # 2 x 6 = 12
    assert _all(st) == (0, 0, 4, 4)
    st = np.zeros((4, 12), np.uint8)
    st[0, 0:6] = 1  # 6 x 1 at y 0
    st[1:3, 6:9] = 1  # 3 x 2 at y 1, x 6
    st[3, 0:6] = 1  # 6 x 1 at y 3
    assert _all(st) == (0, 0, 6, 1)
    # equal area and y, different x: the smaller x; equal area, y and x: the wider one
    st = np.zeros((4, 10), np.uint8)
    st[1:3, 1:4] = 1  # 3 x 2 at (1, 1)
    st[1, 5:10] = 1
    st[1:3, 5:8] = 1  # 3 x 2 at (5, 1), 5 x 1 at (5, 1)
    assert _all(st) == (1, 1, 3, 2)
    sq = np.zeros((4, 4), np.uint8)
    sq[0, :] = 1
    sq[:, 0] = 1  # 4 x 1 and 1 x 4 at (0, 0): the wider one
    assert _all(sq) == (0, 0, 4, 1)


def test_random_masks_against_brute_force():
    rng = np.random.default_rng(1)
    for k in range(300):
        h, w = (int(v) for v in rng.integers(1, 25, 2))
        p = (0.2, 0.5, 0.8, 0.95)[k % 4]
        m = rng.random((h, w)) < p
        want = Z.brute_force(m)
        assert Z.lir(m) == want, (k, m.astype(int))
        if h * w <= 200:
            assert Z.lir_spans(m) == want, (k, m.astype(int))


def test_larger_masks_against_lir_spans():
    rng = np.random.default_rng(2)
    for h, w, p in ((128, 128, 0.97), (100, 128, 0.99), (128, 37, 0.9)):
        m = rng.random((h, w)) < p
        assert Z.lir(m) == Z.lir_spans(m)
    blob = np.zeros((96, 128), np.uint8)
    yy, xx = np.mgrid[:96, :128]
    blob[((yy - 48) / 40.0) ** 2 + ((xx - 64) / 60.0) ** 2 <= 1] = 255
    assert Z.lir(blob) == Z.lir_spans(blob)


def _sc(rows):
    return Z.single_contour(np.array([[int(c) for c in r] for r in rows], np.uint8))


def test_single_contour_hand_counted():
    assert _sc(["111", "101", "111"]) == (1, 1)  # one-pixel hole
    assert _sc(["0110", "1001", "1001", "0110"]) == (1, 1)  # zeros that reach the corners only diagonally stay inside
    assert _sc(["1110", "1111", "1111"]) == (1, 0)  # a zero on the image edge is no hole
    assert _sc(["110", "110", "001"]) == (1, 0)  # blocks touching diagonally: one 8-connected component
    assert _sc(["1100", "0000", "0011"]) == (2, 0)  # two separate blocks
    assert _sc(["11111", "10001", "10001", "11111"]) == (1, 1)  # a ring
    assert _sc(["000", "000"]) == (0, 0)  # empty
    assert _sc(["111", "111"]) == (1, 0)  # full
    assert _sc(["11111", "10101", "11111"]) == (1, 2)  # two holes
    assert _sc(["1111111", "1000001", "1010001", "1000001", "1111111"]) == (2, 1)  # an island in a hole


def test_rectangle_and_times():
    r = S.Rectangle(3, 4, 10, 20)
    assert (r.area, r.corner, r.size, r.x2, r.y2) == (200, (3, 4), (10, 20), 13, 24)
    # numpy.float64 aspects landing on .5: round half to even
    assert S.Rectangle(1, 3, 5, 7).times(np.float64(0.5)) == S.Rectangle(0, 2, 2, 4)
    assert S.Rectangle(5, 9, 11, 13).times(np.float64(1.5)) == S.Rectangle(8, 14, 16, 20)
    assert Z.times((1, 3, 5, 7), np.float64(0.5)) == (0, 2, 2, 4)
    assert all(type(v) is int for v in S.Rectangle(1, 2, 3, 4).times(np.float64(2.5)))


def test_cropper_static_helpers():
    C = S.Cropper
    assert C.get_zero_center_corners([(-5, 10), (3, -2), (0, 0)]) == [(0, 12), (8, 0), (5, 2)]
    assert Z.zero_center_corners([(-5, 10), (3, -2), (0, 0)]) == [(0, 12), (8, 0), (5, 2)]
    rects = C.get_rectangles([(0, 0), (8, 2)], [(10, 10), (10, 6)])
    assert rects == [S.Rectangle(0, 0, 10, 10), S.Rectangle(8, 2, 10, 6)]
    lir = S.Rectangle(2, 1, 12, 6)
    overlaps = C.get_overlaps(rects, lir)
    assert overlaps == [S.Rectangle(2, 1, 8, 6), S.Rectangle(8, 2, 6, 5)]
    assert C.get_intersections(rects, overlaps) == [S.Rectangle(2, 1, 8, 6), S.Rectangle(0, 0, 6, 5)]
    plan = Z.crop_plan([(0, 0), (8, 2)], [(10, 10), (10, 6)], tuple(lir))
    assert plan["overlaps"] == [tuple(o) for o in overlaps]
    assert plan["intersections"] == [(2, 1, 8, 6), (0, 0, 6, 5)]
    # zero-width overlap is allowed; a gap is not
    assert C.get_overlap(S.Rectangle(0, 0, 5, 5), S.Rectangle(5, 0, 5, 5)) == S.Rectangle(5, 0, 0, 5)
    assert Z.overlap((0, 0, 5, 5), (5, 0, 5, 5)) == (5, 0, 0, 5)
    with pytest.raises(S.StitchingError, match="^Rectangles do not overlap!$"):
        C.get_overlap(S.Rectangle(0, 0, 5, 5), S.Rectangle(6, 0, 5, 5))
    with pytest.raises(ValueError, match="do not overlap"):
        Z.overlap((0, 0, 5, 5), (0, 6, 5, 5))
    img = np.arange(12 * 10).reshape(12, 10)
    assert np.array_equal(C.crop_rectangle(img, S.Rectangle(8, 9, 6, 6)), img[9:15, 8:14])
    assert C.crop_rectangle(img, S.Rectangle(8, 9, 6, 6)).shape == (3, 2)  # clipped like numpy


def test_crop_plan_scaled():
    corners, sizes, lir = [(0, 0), (8, 2)], [(10, 10), (10, 6)], (2, 1, 12, 6)
    plan = Z.crop_plan(corners, sizes, lir, np.float64(1.5))
    cr = S.Cropper()
    cr.overlapping_rectangles = [S.Rectangle(*o) for o in plan["overlaps"]]
    cr.intersection_rectangles = [S.Rectangle(*i) for i in plan["intersections"]]
    assert cr.crop_rois(corners, sizes, np.float64(1.5)) == (plan["corners"], plan["sizes"])
    assert plan["corners"] == [(0, 0), (9, 1)] and plan["sizes"] == [(12, 9), (9, 8)]
    assert [tuple(r) for r in (cr.intersection_rectangles[i].times(np.float64(1.5)) for i in range(2))] == plan["crops"]


def test_cropper_false_passes_through():
    cr = S.Cropper(False)
    imgs = [np.zeros((3, 4)), np.ones((5, 6))]
    cr.prepare(imgs, imgs, [(0, 0), (1, 1)], [(4, 3), (6, 5)])  # no GPU, no work
    out = list(cr.crop_images(iter(imgs), 2.0))
    assert all(a is b for a, b in zip(out, imgs))
    assert cr.crop_rois([(7, 8)], [(4, 3)]) == ([(7, 8)], [(4, 3)])
    assert cr.crop_img(imgs[1], 1) is imgs[1]


def test_names_and_message():
    assert "Cropper" in S.__all__ and "Rectangle" in S.__all__
    assert S.Cropper.DEFAULT_CROP is True
    assert INVALID_CONTOUR.startswith("Invalid Contour. Run with --no-crop (using the stitch interface)")
    assert INVALID_CONTOUR.endswith("or Cropper(False) (using the cropper class)")
