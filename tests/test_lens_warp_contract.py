"""The contract of the warp through the lens on the host: tests/numpy_lens_warp.py against cv::remap's arithmetic with an identity lens,
its derived accuracy bound on real lenses, the width of its intermediates, coordinates that are no numbers, and its sensitivity to two
subtly wrong variants.  No device and no library (the per-pixel projector families take their backward maps from the CPU oracle:
tests/numpy_warper.py has only their forward maps).

The identity statement, as the CPU shows it: with identity nodes the contract equals numpy_warper.remap_linear_reflect at EVERY pixel
under numpy_warper.warp_mask — not only where the 1/32-px position lies inside the frame.  Under the mask cvRound(x) is in [0, W - 1],
so the position is at most half a pixel outside; there BORDER_REFLECT reads the edge pixel for both taps of that axis, and so does the
clip of the position with clamped taps.  No exception was found, the statement is not narrowed."""
import numpy as np
import pytest

import stitching_amd as S
from tests import numpy_lens_warp as LW
from tests import numpy_rectify as NR
from tests import numpy_warper as NW
from tests.test_rectify_contract import FISH, K as LENS_K, SRC, WIDE, image

FOCAL = 70.0
TABLED = ["spherical", "cylindrical", "plane"]
FAMILIES = ["fisheye", "paniniA2B1"]


def camera(size, yaw=0.21, pitch=-0.08):
    """K of a `FOCAL`-px camera centred on a frame of `size`, R a yaw about y after a small pitch about x: float32 3 x 3 each"""
    w, h = size
    K = np.array([[FOCAL, 0, w / 2.0], [0, FOCAL, h / 2.0], [0, 0, 1]], np.float32)
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    R = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    return K, R.astype(np.float32)


def identity_nodes(size):
    return NR.quantise(*NR.node_pixels(*size))


def maps_and_mask(kind, size, oracle=None):
    """the backward map over the warp's ROI and the warped mask of a frame of `size`"""
    K, R = camera(size)
    if oracle is None:
        roi = NW.warp_roi(kind, FOCAL, K, R, size)
        xm, ym = NW.map_backward(kind, FOCAL, K, R, roi)
    else:
        roi = oracle.warp_roi(kind, FOCAL, K, R, size)
        xm, ym = oracle.build_maps(kind, FOCAL, K, R, roi)
    return xm, ym, NW.remap_nearest_constant(np.full((size[1], size[0]), 255, np.uint8), xm, ym)


# ---- 1: an identity lens is the existing warp -----------------------------------------------------------------------------------------
def check_identity(xm, ym, mask):
    src = image(SRC, 3, seed=9)
    want = NW.remap_linear_reflect(src, xm, ym)
    got = LW.lens_warp(src, identity_nodes(SRC), SRC, xm, ym)
    under = mask != 0
    assert under.any() and not under.all()
    # the half-pixel rim is part of what is compared: positions outside the frame occur under the mask
    qx, qy = NW._cv_round(xm * NW.F(32)), NW._cv_round(ym * NW.F(32))
    rim = under & ((qx < 0) | (qx > 32 * (SRC[0] - 1)) | (qy < 0) | (qy > 32 * (SRC[1] - 1)))
    assert rim.any()
    assert np.array_equal(got[under], want[under]), np.argwhere((got != want).any(-1) & under)[:4]
    return got, want, under


@pytest.mark.parametrize("kind", TABLED)
def test_identity_nodes_equal_remap_under_the_mask(kind):
    got, want, under = check_identity(*maps_and_mask(kind, SRC))
    if kind != "plane":  # outside the mask the two borders differ: reflection against replication
        assert (got != want)[~under].any()


@pytest.mark.parametrize("kind", FAMILIES)
def test_identity_nodes_equal_remap_under_the_mask_per_pixel_families(kind, oracle):
    check_identity(*maps_and_mask(kind, SRC, oracle))


def test_identity_nodes_give_the_position_back():
    qx, qy = np.meshgrid(np.arange(0, 32 * (SRC[0] - 1) + 1, 7, dtype=np.int32), np.arange(0, 32 * (SRC[1] - 1) + 1, 5, dtype=np.int32))
    q = LW.through_lens(identity_nodes(SRC), qx, qy, SRC)
    assert np.array_equal(q[..., 0], qx) and np.array_equal(q[..., 1], qy)


# ---- 2: the 1/32 px bound ---------------------------------------------------------------------------------------------------------------
LENSES = {
    "brown": lambda: (S.LensMap.brown(LENS_K, WIDE, SRC), lambda nk, u, v: NR.brown_source(LENS_K, WIDE, nk, u, v)),
    "fisheye": lambda: (S.LensMap.fisheye(LENS_K, FISH, SRC, fit="inside"), lambda nk, u, v: NR.fisheye_source(LENS_K, FISH, nk, u, v)),
    "brown_80x60": lambda: (S.LensMap.brown(LENS_K, WIDE, SRC, dst_size=(80, 60)), lambda nk, u, v: NR.brown_source(LENS_K, WIDE, nk, u, v)),
}


def all_positions(size, step=3):
    """every `step`-th 1/32-px position of the rectified frame, the last ones included"""
    w, h = size
    xs = np.unique(np.r_[np.arange(0, 32 * (w - 1) + 1, step), 32 * (w - 1)]).astype(np.int32)
    ys = np.unique(np.r_[np.arange(0, 32 * (h - 1) + 1, step), 32 * (h - 1)]).astype(np.int32)
    return np.meshgrid(xs, ys)


@pytest.mark.parametrize("name", list(LENSES))
def test_quantisation_bound(name):
    lens, model = LENSES[name]()
    sx, sy = model(lens.new_K, *NR.node_pixels(*lens.dst_size))
    assert np.array_equal(lens.nodes, NR.quantise(sx, sy))
    qx, qy = all_positions(lens.dst_size)
    q = LW.through_lens(lens.nodes, qx, qy, lens.dst_size)
    err = np.abs(q / 32.0 - LW.float_bilinear_at(sx, sy, qx, qy)).max()
    print(f"{name}: largest |q / 32 - B| = {err:.6f} px, bound {LW.QUANTISATION_BOUND:.6f}")
    assert LW.QUANTISATION_BOUND == 1.0 / 32.0
    assert err <= LW.QUANTISATION_BOUND
    assert err > 1.0 / 128.0  # the bound is not idle: more than the node rounding alone is met


# ---- 3: intermediates -------------------------------------------------------------------------------------------------------------------
def extreme_nodes(size):
    """nodes that alternate between the clip limits of the Q6 coordinates: the widest products the contract can meet"""
    nx, ny = NR.node_counts(*size)
    n = np.empty((ny, nx, 2), np.int32)
    i, j = np.meshgrid(np.arange(nx), np.arange(ny))
    n[..., 0] = np.where((i + j) & 1, NR.Q6_MAX, NR.Q6_MIN)
    n[..., 1] = np.where((i + j) & 1, NR.Q6_MIN, NR.Q6_MAX)
    return n


@pytest.mark.parametrize("nodes", ["brown", "limits", "all_max"])
def test_intermediates_are_int32_within_2_30(nodes):
    size = SRC
    n = {"brown": lambda: S.LensMap.brown(LENS_K, WIDE, SRC).nodes, "limits": lambda: extreme_nodes(size),
         "all_max": lambda: np.full(NR.node_counts(*size)[::-1] + (2,), NR.Q6_MAX, np.int32)}[nodes]()
    stages = []
    LW.through_lens(n, *all_positions(size, 5), size, stages=stages)
    assert len(stages) == 6
    for a in stages:
        assert a.dtype == np.int32
        assert np.abs(a.astype(np.int64)).max() <= 2 ** 30
    with pytest.raises(AssertionError):
        LW.through_lens(n, *[a.astype(np.int64) for a in all_positions(size, 64)], size)
    with pytest.raises(ValueError):
        LW.through_lens(n.astype(np.int64), *all_positions(size, 64), size)


# ---- 4: coordinates out of range ----------------------------------------------------------------------------------------------------------
def test_coordinates_that_are_no_positions_land_on_clamped_taps():
    lens = S.LensMap.brown(LENS_K, WIDE, SRC)
    src = image(SRC, 3, seed=4)
    w, h = SRC
    bad = np.array([np.nan, np.inf, -np.inf, -1.0, 3.0e9, -3.0e9, 1.0e30, 6.8e7, 6.7e7, -6.8e7, 1.0e6, -1.0e6], np.float32)
    # what each becomes: NaN, infinities and everything whose 32-fold lies outside int32 (6.8e7: 2.18e9) are INT_MIN, so position 0;
    # the rest (6.7e7: 2.14e9 is inside) clips to its side
    hold = np.array([0, 0, 0, 0, 0, 0, 0, 0, w - 1, 0, w - 1, 0], np.float32)
    hold_y = np.where(hold > 0, h - 1, 0).astype(np.float32)
    good = np.float32(11.3)
    for xm, ym, wx, wy in ((bad, np.full_like(bad, good), hold, np.full_like(bad, good)), (np.full_like(bad, good), bad, np.full_like(bad, good), hold_y),
                           (bad, bad[::-1].copy(), hold, hold_y[::-1].copy())):
        got = LW.lens_warp(src, lens.nodes, SRC, xm[None], ym[None])
        want = LW.lens_warp(src, lens.nodes, SRC, wx[None], wy[None])
        assert got.shape == (1, bad.size, 3) and np.array_equal(got, want)
    qx, _ = LW.positions(bad[None], bad[None], SRC)
    assert np.array_equal(qx[0], (hold * 32).astype(np.int32))
    # nodes that point far outside the source: the taps are clamped, the result is the source's corner pixel
    far = np.full(NR.node_counts(w, h)[::-1] + (2,), NR.Q6_MIN, np.int32)
    out = LW.lens_warp(src, far, SRC, bad[None], bad[None])
    assert np.all(out == src[0, 0])
    far[...] = NR.Q6_MAX
    assert np.all(LW.lens_warp(src, far, SRC, bad[None], bad[None]) == src[-1, -1])


# ---- 5: wrong variants are told apart ---------------------------------------------------------------------------------------------------
def single_stage(nodes, qx, qy):
    """one rounding at the end instead of two stages: q = (S + 2^18) >> 19 of the exact Q6 x 2^18 sum"""
    i, j, ax, ay = qx >> 9, qy >> 9, (qx & 511)[..., None].astype(np.int64), (qy & 511)[..., None].astype(np.int64)
    n = nodes.astype(np.int64)
    s = (512 - ay) * ((512 - ax) * n[j, i] + ax * n[j, i + 1]) + ay * ((512 - ax) * n[j + 1, i] + ax * n[j + 1, i + 1])
    return ((s + (1 << 18)) >> 19).astype(np.int32)


def nearest_node(nodes, qx, qy):
    """the nearest node's coordinate instead of the interpolation"""
    return ((nodes[(qy + 256) >> 9, (qx + 256) >> 9] + 1) >> 1).astype(np.int32)


@pytest.mark.parametrize("variant", [single_stage, nearest_node])
def test_a_wrong_variant_differs_on_the_brown_lens(variant):
    lens = S.LensMap.brown(LENS_K, WIDE, SRC)
    src = image(SRC, 3, seed=6)
    xm, ym, mask = maps_and_mask("spherical", SRC)
    qx, qy = LW.positions(xm, ym, SRC)
    q, wrong = LW.through_lens(lens.nodes, qx, qy, SRC), variant(lens.nodes, qx, qy)
    assert (q != wrong).any()
    assert (LW.sample_clamped(src, q) != LW.sample_clamped(src, wrong))[mask != 0].any()
