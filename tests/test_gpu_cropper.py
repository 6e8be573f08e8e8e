"""The largest interior rectangle on the MI355X (stx_crop_lir / stitching_amd.Cropper) against the restatement tests/numpy_lir.py:
seeded random and tie-heavy masks, views and pitched buffers, the low-resolution panorama masks of BASELINE configs 2-5 and config 2's
full-resolution one, the Cropper API, and Stitcher.stitch's order end to end (crop, gain_blocks, voronoi seams, final crop, blend)
against the oracle chain.
Staircase histograms across many lanes' chunks, the global-scratch path and long label chains: tests/test_gpu_constructed_inputs.py."""
import numpy as np
import pytest

import stitching_amd as S
from stitching_amd import config, synthetic
from stitching_amd.cropper import INVALID_CONTOUR, largest_interior_rectangle
from tests import numpy_exposure as X
from tests import numpy_lir as Z
from tests import numpy_seams as SZ

pytestmark = pytest.mark.gpu

LW, LH = 365, 274  # the reference's low_megapix 0.1 of a 4:3 frame


def _check(mask, dev=None):
    (xywh, counts, ms) = largest_interior_rectangle(mask if dev is None else dev)
    host = np.asarray(mask)
    assert xywh == Z.lir(host), (host.shape, xywh, Z.lir(host))
    assert counts == Z.single_contour(host), (host.shape, counts, Z.single_contour(host))
    assert ms > 0.0
    return xywh, counts


SIZES = ((1, 1), (1, 300), (300, 1), (63, 65), (64, 64), (257, 129), (1000, 37), (4097, 777))


@pytest.mark.parametrize("hw", SIZES)
def test_random_masks(gpu_ctx, hw):
    rng = np.random.default_rng(hash(hw) % 2**32)
    for p in (0.05, 0.5, 0.9, 0.995):
        m = np.where(rng.random(hw) < p, 255, 0).astype(np.uint8)
        _check(m)
    # grey values count as true; blobs with holes
    m = (rng.random(hw) < 0.97).astype(np.uint8) * rng.integers(1, 256, hw, dtype=np.uint8)
    _check(m)


def test_tie_heavy_and_uniform_masks(gpu_ctx):
    rng = np.random.default_rng(5)
    plus = np.zeros((61, 61), np.uint8)
    plus[20:41, :] = 1
    plus[:, 20:41] = 1
    stairs = np.zeros((40, 40), np.uint8)
    for k in range(8):
        stairs[5 * k:5 * k + 5, : 40 - 5 * k] = 255
    checker = np.kron((np.indices((30, 30)).sum(0) % 2).astype(np.uint8), np.ones((4, 4), np.uint8))
    tiles = np.kron(rng.random((25, 40)) < 0.7, np.ones((6, 5), bool)).astype(np.uint8)
    for m in (plus, stairs, checker, tiles, np.zeros((50, 70), np.uint8), np.full((50, 70), 255, np.uint8),
              np.zeros((1, 1), np.uint8), np.full((5000, 3), 1, np.uint8), np.full((3, 6000), 1, np.uint8)):
        _check(m)
    assert _check(np.zeros((9, 9), np.uint8)) == ((0, 0, 0, 0), (0, 0))
    assert _check(np.full((9, 7), 255, np.uint8)) == ((0, 0, 7, 9), (1, 0))


def test_views_and_pitched_buffers(gpu_ctx):
    rng = np.random.default_rng(11)
    big = np.where(rng.random((300, 5200)) < 0.93, 255, 0).astype(np.uint8)
    d = S.DeviceImage.from_numpy(big, gpu_ctx)
    for (y0, y1, x0, x1) in ((0, 300, 0, 5200), (7, 250, 3, 200), (1, 2, 5, 4990), (30, 290, 100, 5199), (10, 11, 10, 11)):
        _check(big[y0:y1, x0:x1], d[y0:y1, x0:x1])
    # a pitched mask whose padding holds true cells that must not be read
    padded = np.full((120, 200), 255, np.uint8)
    padded[:, :150] = np.where(rng.random((120, 150)) < 0.9, 255, 0)
    view = S.DeviceImage.from_numpy(padded, gpu_ctx)[:, :150]
    assert view.stride_bytes >= 200
    _check(padded[:, :150], view)


def _low(cfg):
    if cfg == 2:
        cams, wtype = synthetic.ring_cameras(8, LW, LH, focal_factor=0.75), "spherical"
    elif cfg == 3:
        cams, wtype = synthetic.grid_cameras(8, 4, LW, LH, layout_yaw=8), "spherical"
    elif cfg == 4:
        cams, wtype = synthetic.grid_cameras(16, 4, LW, LH, max_edge_lat_deg=50.0, layout_yaw=16), "cylindrical"
    else:
        cams, wtype = synthetic.affine_scan_cameras(16, LW, LH), "affine"
    return cams, wtype, LW, LH


def _panorama_mask(cams, wtype, w, h):
    frames = synthetic.make_frames(range(len(cams)), w, h)
    wp = S.Warper(wtype)
    wp.set_scale(cams)
    sizes = [(w, h)] * len(cams)
    imgs = list(wp.warp_images(frames, cams))
    masks = list(wp.create_and_warp_masks(sizes, cams))
    corners, wsizes = wp.warp_rois(sizes, cams)
    mask = S.Cropper.estimate_panorama_mask(imgs, masks, corners, wsizes)
    return mask, imgs, masks, corners, wsizes


@pytest.mark.parametrize("cfg", (2, 3, 4, 5))
def test_low_resolution_panorama_masks(gpu_ctx, cfg):
    mask, *_ = _panorama_mask(*_low(cfg))
    host = np.asarray(mask)
    assert np.count_nonzero(host) > 0
    xywh, counts = _check(host)
    _check(host, S.DeviceImage.from_numpy(host, gpu_ctx))
    if counts == (1, 0):
        assert S.Cropper().estimate_largest_interior_rectangle(host) == S.Rectangle(*xywh)


def test_full_resolution_panorama_mask(gpu_ctx, monkeypatch):
    monkeypatch.setattr(config, "_device_resident", True)
    mask, *_ = _panorama_mask(synthetic.ring_cameras(8, 4000, 3000, focal_factor=0.75), "spherical", 4000, 3000)
    assert isinstance(mask, S.DeviceImage)
    host = mask.numpy()
    xywh, counts, _ = largest_interior_rectangle(mask)
    assert xywh == Z.lir(host)
    assert counts == Z.single_contour(host)


def test_cropper_api(gpu_ctx):
    cams, wtype, w, h = _low(2)
    mask, imgs, masks, corners, sizes = _panorama_mask(cams, wtype, w, h)
    cropper = S.Cropper()
    cropper.prepare(imgs, masks, corners, sizes)
    lir = Z.lir(np.asarray(mask))
    plan = Z.crop_plan(corners, sizes, lir, np.float64(2.0))
    assert [tuple(r) for r in cropper.overlapping_rectangles] == plan["overlaps"]
    assert [tuple(r) for r in cropper.intersection_rectangles] == plan["intersections"]

    pulled = []

    def recording(items):
        for i, it in enumerate(items):
            pulled.append(i)
            yield it

    gen = cropper.crop_images(recording(imgs))
    assert pulled == []
    first = next(gen)
    assert pulled == [0]
    assert np.array_equal(np.asarray(first), Z.crop(np.asarray(imgs[0]), plan["intersections"][0]))
    next(gen)
    assert pulled == [0, 1]

    d_imgs = [S.DeviceImage.from_numpy(np.asarray(i), gpu_ctx) for i in imgs]
    for k, (d, c) in enumerate(zip(cropper.crop_images(d_imgs), plan["intersections"])):
        assert isinstance(d, S.DeviceImage)
        assert d.device_ptr() == d_imgs[k].device_ptr() + c[1] * d_imgs[k].stride_bytes + c[0] * d_imgs[k].channels
        assert np.array_equal(d.numpy(), Z.crop(np.asarray(imgs[k]), c))
    # a scaled rectangle past the image: the clipped shape numpy slicing gives
    for aspect in (np.float64(2.0), np.float64(1.5)):
        for k, (d, c) in enumerate(zip(cropper.crop_images(d_imgs, aspect), Z.crop_plan(corners, sizes, lir, aspect)["crops"])):
            want = Z.crop(np.asarray(imgs[k]), c)
            assert d.shape == want.shape
            assert np.array_equal(np.asarray(d), want)
    got_c, got_s = cropper.crop_rois(corners, sizes, np.float64(2.0))
    assert got_c == plan["corners"] and got_s == plan["sizes"]

    ring = np.full((40, 40), 255, np.uint8)
    ring[10:20, 10:20] = 0
    with pytest.raises(S.StitchingError) as e:
        S.Cropper().estimate_largest_interior_rectangle(ring)
    assert str(e.value) == INVALID_CONTOUR
    with pytest.raises(S.StitchingError, match="Invalid Contour"):
        S.Cropper().estimate_largest_interior_rectangle(S.DeviceImage.from_numpy(np.zeros((8, 8), np.uint8), gpu_ctx))


@pytest.mark.parametrize("resident", (False, True))
def test_end_to_end_in_stitcher_order(oracle, gpu_ctx, monkeypatch, resident):
    """Stitcher.stitch's order with injected cameras: low-resolution warp, Cropper.prepare, crop of the low-resolution images, masks
    and rois, gain_blocks feed and voronoi seams on the device, final warp cropped with lir_aspect, apply, SeamFinder.resize and the
    multi-band blend — against the oracle warper + numpy_lir / crop_plan + the restatements + the oracle blender."""
    monkeypatch.setattr(config, "_exposure_estimator", "device")
    monkeypatch.setattr(config, "_seam_estimator", "device")
    monkeypatch.setattr(config, "_device_resident", resident)
    n, w, h, wtype, strength = 4, 320, 240, "spherical", 5
    frames = synthetic.make_frames(range(n), w, h)
    cams = synthetic.ring_cameras(n, w, h, focal_factor=0.75, span_deg=180.0)
    low = [np.asarray(S.resize_linear_exact(f, (w // 2, h // 2))) for f in frames]
    sizes_low = [(x.shape[1], x.shape[0]) for x in low]
    aspect, lir_aspect = 0.5, np.float64(2.0)

    # the product
    wp = S.Warper(wtype)
    wp.set_scale(cams)
    l_imgs = list(wp.warp_images(low, cams, aspect))
    l_masks = list(wp.create_and_warp_masks(sizes_low, cams, aspect))
    l_corners, l_sizes = wp.warp_rois(sizes_low, cams, aspect)
    cropper = S.Cropper()
    cropper.prepare(l_imgs, l_masks, l_corners, l_sizes)
    c_imgs = list(cropper.crop_images(l_imgs))
    c_masks = list(cropper.crop_images(l_masks))
    c_corners, c_sizes = cropper.crop_rois(l_corners, l_sizes)
    comp = S.ExposureErrorCompensator("gain_blocks")
    comp.feed(c_corners, c_imgs, c_masks)
    seams = S.SeamFinder("voronoi").find(c_imgs, c_corners, c_masks)
    sizes = [(f.shape[1], f.shape[0]) for f in frames]
    f_imgs = list(cropper.crop_images(wp.warp_images(frames, cams), lir_aspect))
    f_masks = list(cropper.crop_images(wp.create_and_warp_masks(sizes, cams), lir_aspect))
    f_corners, f_sizes = cropper.crop_rois(*wp.warp_rois(sizes, cams), lir_aspect)
    f_imgs = [comp.apply(i, c, im, m) for i, (im, c, m) in enumerate(zip(f_imgs, f_corners, f_masks))]
    fed = [S.SeamFinder.resize(s, m) for s, m in zip(seams, f_masks)]
    bl = S.Blender("multiband", strength)
    bl.prepare(f_corners, f_sizes)
    for im, mk, c in zip(f_imgs, fed, f_corners):
        bl.feed(im, mk, c)
    pano, pmask = bl.blend()
    if resident:
        assert all(isinstance(a, S.DeviceImage) for a in c_imgs + c_masks + f_imgs)

    # the oracle chain
    ow = oracle.Warper(wtype)
    ow.set_scale(cams)
    o_imgs = [np.asarray(x) for x in ow.warp_images(low, cams, aspect)]
    o_masks = [np.asarray(x) for x in ow.create_and_warp_masks(sizes_low, cams, aspect)]
    o_corners, o_sizes = ow.warp_rois(sizes_low, cams, aspect)
    ob = oracle.Blender("no", 5)
    ob.prepare(o_corners, o_sizes)
    for im, mk, c in zip(o_imgs, o_masks, o_corners):
        ob.feed(im, mk, c)
    _, o_pmask = ob.blend()
    o_pmask = np.asarray(o_pmask)
    assert Z.single_contour(o_pmask) == (1, 0)
    lir = Z.lir(o_pmask)
    assert tuple(cropper.overlapping_rectangles[0]) == Z.crop_plan(o_corners, o_sizes, lir)["overlaps"][0]
    low_plan = Z.crop_plan(o_corners, o_sizes, lir)
    oc_imgs = [Z.crop(a, r) for a, r in zip(o_imgs, low_plan["crops"])]
    oc_masks = [Z.crop(a, r) for a, r in zip(o_masks, low_plan["crops"])]
    assert all(np.array_equal(np.asarray(a), b) for a, b in zip(c_imgs, oc_imgs))
    assert all(np.array_equal(np.asarray(a), b) for a, b in zip(c_masks, oc_masks))
    assert (c_corners, c_sizes) == (low_plan["corners"], low_plan["sizes"])
    gains = X.feed("gain_blocks", low_plan["corners"], oc_imgs, oc_masks)
    assert all(np.array_equal(np.asarray(g), np.asarray(r, np.float32).reshape(np.asarray(g).shape)) for g, r in zip(comp.gains, gains))
    o_seams = SZ.find("voronoi", low_plan["corners"], oc_masks)
    assert all(np.array_equal(np.asarray(a), b) for a, b in zip(seams, o_seams))
    fo_imgs = [np.asarray(x) for x in ow.warp_images(frames, cams)]
    fo_masks = [np.asarray(m) for m in ow.create_and_warp_masks(sizes, cams)]
    plan = Z.crop_plan(o_corners, o_sizes, lir, lir_aspect)  # crop_img / crop_rois scale the low-resolution plan
    fc_imgs = [Z.crop(a, r) for a, r in zip(fo_imgs, plan["crops"])]
    fc_masks = [Z.crop(a, r) for a, r in zip(fo_masks, plan["crops"])]
    assert all(np.array_equal(np.asarray(a), b) for a, b in zip(f_masks, fc_masks))
    assert (f_corners, f_sizes) == (plan["corners"], plan["sizes"])
    fc_imgs = [oracle.block_gain_apply(im, g) for im, g in zip(fc_imgs, gains)]
    assert all(np.array_equal(np.asarray(a), b) for a, b in zip(f_imgs, fc_imgs))
    o_fed = [oracle.seam_resize(s, m) for s, m in zip(o_seams, fc_masks)]
    assert all(np.array_equal(np.asarray(a), b) for a, b in zip(fed, o_fed))
    ob = oracle.Blender("multiband", strength)
    ob.prepare(plan["corners"], plan["sizes"])
    for im, mk, c in zip(fc_imgs, o_fed, plan["corners"]):
        ob.feed(im, mk, c)
    o_pano, o_mask = ob.blend()
    assert np.array_equal(np.asarray(pmask), np.asarray(o_mask))
    assert np.array_equal(np.asarray(pano), np.asarray(o_pano))
