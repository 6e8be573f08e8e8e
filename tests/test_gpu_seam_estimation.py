"""Seam finding on the MI355X (stitching_amd.SeamEstimator) against the restatement tests/numpy_seams.py, byte for byte: named cases from
one image to config 4's 64-frame grid and a full-resolution ring, numpy / device / view inputs, residency, and the reference's order end
to end (low-resolution seams, final-resolution resize + compose) against the oracle chain.
Ragged masks, far sources, rows without a source and ties (constructed, not warped): tests/test_gpu_constructed_inputs.py."""
import numpy as np
import pytest

import stitching_amd as S
from stitching_amd import config, synthetic
from tests import numpy_seams as Z

pytestmark = pytest.mark.gpu

LW, LH = 365, 274  # the reference's low_megapix 0.1 of a 4:3 frame


def _cams(wtype, n, w, h):
    if wtype == "affine":
        return synthetic.affine_scan_cameras(n, w, h)
    return synthetic.ring_cameras(n, w, h, focal_factor=0.75, span_deg=min(340.0, 45.0 * n))


def _warped(cams, wtype, w, h, aspect=1):
    """The product's warper on frames of w x h: images, masks (numpy) and corners."""
    frames = synthetic.make_frames(range(len(cams)), w, h)
    wp = S.Warper(wtype)
    wp.set_scale(cams)
    sizes = [(w, h)] * len(cams)
    imgs = [np.asarray(x) for x in wp.warp_images(frames, cams, aspect)]
    masks = [np.asarray(x) for x in wp.create_and_warp_masks(sizes, cams, aspect)]
    corners, _ = wp.warp_rois(sizes, cams, aspect)
    return [tuple(int(v) for v in c) for c in corners], imgs, masks


def _case(name):
    """-> corners, imgs, masks of a named case."""
    if name == "n1":
        return _warped(_cams("spherical", 1, 192, 144), "spherical", 192, 144)
    if name == "n2_cyl":
        return _warped(_cams("cylindrical", 2, 192, 144), "cylindrical", 192, 144)
    if name == "n3_sph":
        return _warped(_cams("spherical", 3, 192, 144), "spherical", 192, 144)
    if name == "n4_affine":
        return _warped(_cams("affine", 4, 160, 120), "affine", 160, 120)
    if name == "n8_negative":
        c, i, m = _warped(_cams("spherical", 8, 128, 96), "spherical", 128, 96)
        return [(x - 1000, y - 37) for x, y in c], i, m
    if name == "special":  # an image without overlap, an empty mask, grey values
        c, i, m = _warped(_cams("cylindrical", 4, 160, 120), "cylindrical", 160, 120)
        c[3] = (c[3][0] + 5000, c[3][1])
        m[1] = np.zeros_like(m[1])
        m[2] = m[2].copy()
        m[2][::3] = np.where(m[2][::3] == 255, 254, m[2][::3])
        m[0] = m[0].copy()
        m[0][:, ::5] = np.where(m[0][:, ::5] == 255, 77, m[0][:, ::5])
        return c, i, m
    if name == "config2_low":
        return _warped(synthetic.ring_cameras(8, LW, LH, focal_factor=0.75), "spherical", LW, LH)
    if name == "config4_low":
        cams = synthetic.grid_cameras(16, 4, LW, LH, max_edge_lat_deg=50.0, layout_yaw=16)
        return _warped(cams, "cylindrical", LW, LH)
    if name == "saturation":  # a 9000-wide overlap: distances saturate at 8192 (tests/test_seam_estimation.py)
        w = 9000
        a, b = np.full((3, w), 255, np.uint8), np.full((3, w), 255, np.uint8)
        b[:, 0] = 0
        return [(0, 0), (0, 0)], [np.zeros((3, w, 3), np.uint8)] * 2, [a, b]
    if name == "config2_full":  # three neighbours of config 2's ring at full resolution (4000 x 3000 frames)
        cams = synthetic.ring_cameras(8, 4000, 3000, focal_factor=0.75)[:3]
        return _warped(cams, "spherical", 4000, 3000)
    raise KeyError(name)


CASES = ("n1", "n2_cyl", "n3_sph", "n4_affine", "n8_negative", "special", "config2_low", "config4_low", "saturation", "config2_full")


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("kind", Z.KINDS)
def test_device_equals_the_restatement(gpu_ctx, kind, case):
    corners, imgs, masks = _case(case)
    before = [m.copy() for m in masks]
    est = S.SeamEstimator(kind)
    got = est.find(imgs, corners, masks)
    want = Z.find(kind, corners, masks, [(i.shape[1], i.shape[0]) for i in imgs])
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert isinstance(g, np.ndarray) and g.dtype == np.uint8 and g.shape == w.shape
        assert np.array_equal(g, w), (k, int(np.count_nonzero(g != w)))
    assert all(np.array_equal(m, b) for m, b in zip(masks, before))
    if kind == "voronoi":
        assert est.info["pairs"] == len(Z.pairs(corners, [(i.shape[1], i.shape[0]) for i in imgs]))
        assert est.info["levels"] >= (1 if est.info["pairs"] else 0)
        if case == "config4_low":
            assert est.info["levels"] > 1
        if case == "saturation":
            assert np.all(got[0][:, 8192:] == 0) and np.all(got[0][:, :8192] == 255)
    again = S.SeamEstimator(kind).find(imgs, corners, masks)
    assert all(np.array_equal(a, b) for a, b in zip(again, got))


def test_device_and_view_inputs_stay_and_stay_on_the_device(gpu_ctx):
    corners, imgs, masks = _case("n3_sph")
    want = Z.find("voronoi", corners, masks)
    d_masks = [S.DeviceImage.from_numpy(m, gpu_ctx) for m in masks]
    d_imgs = [S.DeviceImage.from_numpy(i, gpu_ctx) for i in imgs]
    got = S.SeamEstimator("voronoi").find(d_imgs, corners, d_masks)
    assert all(isinstance(g, S.DeviceImage) for g in got)
    assert all(np.array_equal(g.numpy(), w) for g, w in zip(got, want))
    assert all(np.array_equal(d.numpy(), m) for d, m in zip(d_masks, masks))
    # cropper-style views: a pitched rectangle of a larger device mask; corners moved by the rectangle's origin
    big = [np.zeros((m.shape[0] + 9, m.shape[1] + 13), np.uint8) for m in masks]
    for b, m in zip(big, masks):
        b[5:5 + m.shape[0], 7:7 + m.shape[1]] = m
        b[:5] = 255  # outside the view: must not be read
    d_big = [S.DeviceImage.from_numpy(b, gpu_ctx) for b in big]
    views = [d[5:5 + m.shape[0], 7:7 + m.shape[1]] for d, m in zip(d_big, masks)]
    got = S.SeamEstimator("voronoi").find(imgs, corners, views)
    assert all(np.array_equal(g.numpy(), w) for g, w in zip(got, want))
    assert all(np.array_equal(d.numpy(), b) for d, b in zip(d_big, big))
    got = S.SeamEstimator("no").find(imgs, corners, views)
    assert all(np.array_equal(g.numpy(), m) for g, m in zip(got, masks))


def test_residency(gpu_ctx, monkeypatch):
    corners, imgs, masks = _case("n2_cyl")
    assert all(isinstance(g, np.ndarray) for g in S.SeamEstimator("voronoi").find(imgs, corners, masks))
    monkeypatch.setattr(config, "_device_resident", True)
    got = S.SeamEstimator("voronoi").find(imgs, corners, masks)
    assert all(isinstance(g, S.DeviceImage) for g in got)
    assert all(np.array_equal(g.numpy(), w) for g, w in zip(got, Z.find("voronoi", corners, masks)))


def test_errors_from_the_device_entry(gpu_ctx):
    corners, imgs, masks = _case("n2_cyl")
    est = S.SeamEstimator("voronoi")
    with pytest.raises(S.StitchingError, match="u8x1"):
        est.find(imgs, corners, [S.DeviceImage.from_numpy(np.dstack([m] * 3), gpu_ctx) for m in masks])
    with pytest.raises(S.StitchingError, match="its image"):
        est.find(imgs, corners, [S.DeviceImage.from_numpy(m[1:], gpu_ctx) for m in masks])


def test_end_to_end_in_stitcher_order(oracle, gpu_ctx, monkeypatch):
    """Stitcher.stitch's order with injected cameras: low-resolution seams through SeamFinder("voronoi") in "device" mode, then
    SeamFinder.resize_all and compose at final resolution — against the oracle warper + the restatement's seams + oracle.seam_resize +
    the oracle blender."""
    from stitching_amd.pipeline import compose

    monkeypatch.setattr(config, "_seam_estimator", "device")
    n, w, h, wtype, strength = 4, 320, 240, "spherical", 5
    frames = synthetic.make_frames(range(n), w, h)
    cams = _cams(wtype, n, w, h)
    low = [np.asarray(S.resize_linear_exact(f, (w // 2, h // 2))) for f in frames]
    sizes_low = [(x.shape[1], x.shape[0]) for x in low]
    aspect = 0.5
    wp = S.Warper(wtype)
    wp.set_scale(cams)
    l_imgs = wp.warp_images(low, cams, aspect)
    l_masks = wp.create_and_warp_masks(sizes_low, cams, aspect)
    l_corners, _ = wp.warp_rois(sizes_low, cams, aspect)
    finder = S.SeamFinder("voronoi")
    assert isinstance(finder.finder, S.SeamEstimator)
    seams = finder.find(l_imgs, l_corners, l_masks)

    ow = oracle.Warper(wtype)
    ow.set_scale(cams)
    o_masks = [np.asarray(x) for x in ow.create_and_warp_masks(sizes_low, cams, aspect)]
    o_corners, _ = ow.warp_rois(sizes_low, cams, aspect)
    o_seams = Z.find("voronoi", o_corners, o_masks)
    assert all(np.array_equal(np.asarray(a), b) for a, b in zip(seams, o_seams))
    assert any(np.count_nonzero(s) < np.count_nonzero(m) for s, m in zip(o_seams, o_masks))  # the seams cut something

    sizes = [(f.shape[1], f.shape[0]) for f in frames]
    f_imgs = ow.warp_images(frames, cams)
    f_masks = [np.asarray(m) for m in ow.create_and_warp_masks(sizes, cams)]
    f_corners, f_sizes = ow.warp_rois(sizes, cams)
    fed = [oracle.seam_resize(s, m) for s, m in zip(o_seams, f_masks)]
    resized = S.SeamFinder.resize_all(seams, [S.DeviceImage.from_numpy(m, gpu_ctx) for m in f_masks])
    assert all(np.array_equal(np.asarray(a), b) for a, b in zip(resized, fed))
    ob = oracle.Blender("multiband", strength)
    ob.prepare(f_corners, f_sizes)
    for im, mk, c in zip(f_imgs, fed, f_corners):
        ob.feed(np.asarray(im), mk, c)
    o_pano, o_mask = ob.blend()
    pano, pmask = compose(frames, cams, warper_type=wtype, blend_strength=strength, seam_masks=seams, ctx=gpu_ctx)
    assert np.array_equal(np.asarray(pmask), np.asarray(o_mask))
    assert np.array_equal(np.asarray(pano), np.asarray(o_pano))
