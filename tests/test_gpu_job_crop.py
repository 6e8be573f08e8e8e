"""StitchJob(..., cropper=): only the cropper's rectangle of every image is warped.  A warped pixel depends on its own coordinates only,
so the panorama must be byte for byte what the reference's order gives — warp whole, Cropper.crop_images, apply, SeamFinder.resize, feed
(stitching/stitcher.py:117-128) — for every blender, with block gains laid over the CROPPED image and with host seam masks, where the
seam-cell crop (view_rects) works inside the cropped image."""
import numpy as np
import pytest

import stitching_amd as S
from stitching_amd import config, synthetic
from stitching_amd.pipeline import StitchJob, compose
from stitching_amd.synthetic import blend_strength_for_bands

N, W, H = 4, 96, 72
# (low-resolution frame size, camera aspect of the low pass, lir_aspect); 2.5: Rectangle.times rounds, and one slice is clipped
SCALES = {"x2": ((48, 36), 0.5, np.float64(2.0)), "x2.5": ((38, 29), 0.4, 2.5)}
_cache = {}


def setup(gpu_ctx, wtype, scale):
    """frames, cameras, the cropper prepared on the low-resolution warps, host voronoi seam masks of the cropped low-resolution images,
    and the whole final warps with their rois — made once per (warper, scale), never changed"""
    key = (wtype, scale)
    if key in _cache:
        return _cache[key]
    low_size, aspect, lir_aspect = SCALES[scale]
    frames = synthetic.make_frames(range(N), W, H)
    cams = synthetic.ring_cameras(N, W, H, focal_factor=0.75, span_deg=110.0)
    low = [S.resize_linear_exact(f, low_size, ctx=gpu_ctx, device_resident=False) for f in frames]
    wp = S.Warper(wtype, ctx=gpu_ctx)
    wp.set_scale(cams)
    l_imgs, l_masks, l_rois = wp.warp_images_and_masks(low, cams, aspect)
    l_corners, l_sizes = [r[0:2] for r in l_rois], [r[2:4] for r in l_rois]
    cropper = S.Cropper()
    cropper.prepare(l_imgs, l_masks, l_corners, l_sizes)
    c_imgs, c_masks = list(cropper.crop_images(l_imgs)), list(cropper.crop_images(l_masks))
    c_corners, c_sizes = cropper.crop_rois(l_corners, l_sizes)
    seams = [np.asarray(m) for m in S.SeamFinder("voronoi", estimator=S.SeamEstimator("voronoi")).find(c_imgs, c_corners, c_masks)]
    whole = wp.warp_images_and_masks(frames, cams)
    _cache[key] = dict(frames=frames, cams=cams, cropper=cropper, lir_aspect=lir_aspect, seams=seams, whole=whole)
    return _cache[key]


def reference_order(ctx, s, wtype, blender_type, num_bands=None, strength=5, gains=None, seams=None):
    """warp whole (done once in setup), crop_images, apply, SeamFinder.resize, feed"""
    cropper, lir = s["cropper"], s["lir_aspect"]
    imgs, masks, rois = s["whole"]
    corners, sizes = [r[0:2] for r in rois], [r[2:4] for r in rois]
    c_imgs = [np.array(a) for a in cropper.crop_images(imgs, lir)]  # copies: apply multiplies in place
    c_masks = list(cropper.crop_images(masks, lir))
    c_corners, c_sizes = cropper.crop_rois(corners, sizes, lir)
    if gains is not None:
        c_imgs = [gains.apply(i, c, im, m) for i, (im, c, m) in enumerate(zip(c_imgs, c_corners, c_masks))]
    if seams is not None:
        c_masks = [S.SeamFinder.resize(sm, m) for sm, m in zip(seams, c_masks)]
    if num_bands is not None:
        roi = S.Blender.result_roi(c_corners, c_sizes)
        strength = blend_strength_for_bands(num_bands, roi[2], roi[3])
    bl = S.Blender(blender_type, strength, ctx=ctx)
    bl.prepare(c_corners, c_sizes)
    for im, mk, c in zip(c_imgs, c_masks, c_corners):
        bl.feed(im, mk, c)
    pano, pmask = bl.blend()
    return np.asarray(pano), np.asarray(pmask), [a.shape[:2] for a in c_imgs]


def block_gains(shapes, block, channels=1):
    """a compensator with seeded gain maps of `block`-sized blocks over the CROPPED images"""
    rng = np.random.default_rng(99)
    comp = S.ExposureErrorCompensator("gain_blocks" if channels == 1 else "channel_blocks", block_size=block, estimator=object())
    maps = [rng.uniform(0.7, 1.4, ((h + block - 1) // block, (w + block - 1) // block) + ((3,) if channels == 3 else ())).astype(np.float32)
            for h, w in shapes]
    comp.set_gains(maps)
    return comp


BLENDERS = [("multiband", 2), ("feather", None), ("no", None)]


@pytest.mark.gpu
@pytest.mark.parametrize("scale", list(SCALES))
@pytest.mark.parametrize("blender_type,bands", BLENDERS)
@pytest.mark.parametrize("wtype", ["spherical", "plane"])
def test_cropped_job_equals_warp_whole_then_crop(gpu_ctx, wtype, blender_type, bands, scale):
    s = setup(gpu_ctx, wtype, scale)
    want_pano, want_mask, shapes = reference_order(gpu_ctx, s, wtype, blender_type, bands)
    job = StitchJob(s["frames"], s["cams"], warper_type=wtype, blender_type=blender_type, num_bands=bands, ctx=gpu_ctx,
                    cropper=s["cropper"], crop_aspect=s["lir_aspect"])
    pano, pmask = job.run()
    assert isinstance(pano, S.DeviceImage) and config.device_resident() is False
    assert np.array_equal(pmask.numpy(), want_mask) and np.array_equal(pano.numpy(), want_pano)
    assert pano.shape[0] < max(r[3] for r in s["whole"][2])  # it IS cropped: lower than the tallest whole warp
    # the pair form of the argument, and a second run of the same job
    job2 = StitchJob(s["frames"], s["cams"], warper_type=wtype, blender_type=blender_type, num_bands=bands, ctx=gpu_ctx,
                     cropper=(s["cropper"], s["lir_aspect"]))
    assert np.array_equal(job2.run()[0].numpy(), want_pano) and np.array_equal(job.run()[0].numpy(), want_pano)


@pytest.mark.gpu
@pytest.mark.parametrize("scale", list(SCALES))
@pytest.mark.parametrize("blender_type,bands", BLENDERS)
@pytest.mark.parametrize("wtype", ["spherical", "plane"])
def test_block_gains_lie_over_the_cropped_image(gpu_ctx, wtype, blender_type, bands, scale):
    s = setup(gpu_ctx, wtype, scale)
    _, _, shapes = reference_order(gpu_ctx, s, wtype, "no")
    comp = block_gains(shapes, 8)
    want_pano, want_mask, _ = reference_order(gpu_ctx, s, wtype, blender_type, bands, gains=comp)
    pano, pmask = StitchJob(s["frames"], s["cams"], warper_type=wtype, blender_type=blender_type, num_bands=bands, ctx=gpu_ctx,
                            compensator=comp, cropper=s["cropper"], crop_aspect=s["lir_aspect"]).run()
    assert np.array_equal(pmask.numpy(), want_mask) and np.array_equal(pano.numpy(), want_pano)
    plain, _, _ = reference_order(gpu_ctx, s, wtype, blender_type, bands)
    assert not np.array_equal(plain, want_pano)  # the gains do something


@pytest.mark.gpu
@pytest.mark.parametrize("scale", list(SCALES))
@pytest.mark.parametrize("blender_type,bands", BLENDERS)
@pytest.mark.parametrize("wtype", ["spherical", "plane"])
def test_host_seam_masks_inside_the_crop(gpu_ctx, wtype, blender_type, bands, scale):
    """host seam masks: with the multi-band blender view_rects cuts every image to its seam cell INSIDE the cropped image; the gain
    maps still lie over the cropped image (the cell's offset travels with it)"""
    s = setup(gpu_ctx, wtype, scale)
    _, _, shapes = reference_order(gpu_ctx, s, wtype, "no")
    for comp in (None, block_gains(shapes, 8), block_gains(shapes, 8, channels=3)):
        want_pano, want_mask, _ = reference_order(gpu_ctx, s, wtype, blender_type, bands, gains=comp, seams=s["seams"])
        job = StitchJob(s["frames"], s["cams"], warper_type=wtype, blender_type=blender_type, num_bands=bands, ctx=gpu_ctx,
                        seam_masks=s["seams"], compensator=comp, cropper=s["cropper"], crop_aspect=s["lir_aspect"])
        pano, pmask = job.run()
        print(wtype, blender_type, scale, "seam-cell rectangles:", job.last_crop)
        assert np.array_equal(pmask.numpy(), want_mask) and np.array_equal(pano.numpy(), want_pano)
        # which branch a configuration takes: seam cells are cut with the multi-band blender where every clipped slice has its
        # crop_rois size — both plane scales, the non-integer aspect included; "spherical" / "x2.5" clips one slice (67 rows of a
        # 68-row rectangle) and skips them, "spherical" / "x2" finds no cell narrow enough to be worth a cut
        assert (job.last_crop is not None) == (blender_type == "multiband" and wtype == "plane")
        # compose() takes the same arguments
        pano2, _ = compose(s["frames"], s["cams"], warper_type=wtype, blender_type=blender_type,
                           blend_strength=job.blend_strength, compensator=comp, seam_masks=s["seams"], ctx=gpu_ctx,
                           cropper=s["cropper"], crop_aspect=s["lir_aspect"])
        assert np.array_equal(pano2.numpy(), want_pano)


@pytest.mark.gpu
def test_seam_cells_are_cut_inside_a_crop(gpu_ctx):
    """the combination really happens: at least one of the configurations above warps less than the cropper's rectangle"""
    cut = 0
    for wtype in ("spherical", "plane"):
        s = setup(gpu_ctx, wtype, "x2")
        job = StitchJob(s["frames"], s["cams"], warper_type=wtype, blender_type="multiband", num_bands=2, ctx=gpu_ctx,
                        seam_masks=s["seams"], cropper=s["cropper"], crop_aspect=s["lir_aspect"])
        job.run()
        cut += job.last_crop is not None and any(c is not None for c in job.last_crop)
    assert cut >= 1


@pytest.mark.gpu
def test_no_cropper_and_crop_false_are_todays_path(gpu_ctx):
    s = setup(gpu_ctx, "spherical", "x2")
    a = StitchJob(s["frames"], s["cams"], num_bands=2, ctx=gpu_ctx).run()[0].numpy()
    b = StitchJob(s["frames"], s["cams"], num_bands=2, ctx=gpu_ctx, cropper=S.Cropper(False), crop_aspect=2.0).run()[0].numpy()
    assert np.array_equal(a, b)
    with pytest.raises(S.StitchingError, match="not prepared"):
        StitchJob(s["frames"], s["cams"], ctx=gpu_ctx, cropper=S.Cropper())
