"""A StitchJob makes the geometry of its rig once: ROIs, warped masks, seam-mask resize and the multi-band blender's weight pyramids
are kept after the first run (stitching_amd/pipeline.py: StitchJob, rig_key; include/stitching_amd.h: stx_blend_keep_weights), later
runs warp the images alone and build their pyramids without the weight half.  Results cannot change: every comparison here is byte for
byte, panorama and mask, against a FRESH job built with reuse_geometry=False on the same inputs (whose own exactness against the oracle
the parity tests pin).

Shapes: 4 frames of 640 x 480, focal 0.75 W, 3 bands — every warped image spans several 64 x 14 pyrDown tiles and 512 x 8 gather tiles in
both directions; the 2 x 2 grid has pitched rows, so its feed rectangles hold empty occupancy tiles."""
import ctypes as C

import numpy as np
import pytest

import stitching_amd as S
from stitching_amd import config, synthetic
from stitching_amd.pipeline import StitchJob

N, W, H, BANDS = 4, 640, 480, 3
_cache = {}


def rig(name):
    """frames (two sets), cameras (two sets with different focals -> another scale): made once, never changed"""
    if name not in _cache:
        if name in ("ring", "tight"):  # tight: 4 frames over 110 degrees — seam cells a quarter of an image wide, worth a cut
            span = 180.0 if name == "ring" else 110.0
            cams = synthetic.ring_cameras(N, W, H, focal_factor=0.75, span_deg=span)
            cams2 = synthetic.ring_cameras(N, W, H, focal_factor=0.8, span_deg=span)
        else:
            cams = synthetic.grid_cameras(2, 2, W, H, focal_factor=0.75, span_deg=120.0)
            cams2 = synthetic.grid_cameras(2, 2, W, H, focal_factor=0.8, span_deg=120.0)
        _cache[name] = dict(frames=synthetic.make_frames(range(N), W, H), other=synthetic.make_frames(range(10, 10 + N), W, H), cams=cams,
                            cams2=cams2)
    return _cache[name]


def host(pair):
    return tuple(np.asarray(a) for a in pair)


def same(a, b):
    return np.array_equal(a[1], b[1]) and np.array_equal(a[0], b[0])


def fresh(ctx, frames, cams, scale_cams=None, **kw):
    """the yardstick: a job that keeps nothing, run once"""
    job = StitchJob(frames, cams, ctx=ctx, reuse_geometry=False, **kw)
    if scale_cams is not None:
        job.warper.set_scale(scale_cams)
    out = host(job.run())
    assert not job.last_reused and not job.last_weights_adopted
    return out


def low_res_seams(ctx, frames, cams):
    """host voronoi seam masks of the half-resolution warps (what a low-resolution pass leaves)"""
    low = [S.resize_linear_exact(f, (W // 2, H // 2), ctx=ctx, device_resident=False) for f in frames]
    wp = S.Warper("spherical", ctx=ctx)
    wp.set_scale(cams)
    imgs, masks, rois = wp.warp_images_and_masks(low, cams, 0.5)
    corners = [r[0:2] for r in rois]
    return [np.asarray(m) for m in S.SeamFinder("voronoi", estimator=S.SeamEstimator("voronoi")).find(imgs, corners, masks)]


def full_res_cells(ctx, frames, cams):
    """host 0 / 255 seam masks at the warped size, and the warped sizes"""
    wp = S.Warper("spherical", ctx=ctx)
    wp.set_scale(cams)
    _, masks, rois = wp.warp_images_and_masks(frames, cams)
    corners, sizes = [r[0:2] for r in rois], [r[2:4] for r in rois]
    return synthetic.voronoi_seam_masks([np.asarray(m) for m in masks], corners, sizes), sizes


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ring", "grid"])
def test_runs_of_one_job_equal_a_fresh_job(gpu_ctx, name):
    r = rig(name)
    want = fresh(gpu_ctx, r["frames"], r["cams"], num_bands=BANDS)
    job = StitchJob(r["frames"], r["cams"], num_bands=BANDS, ctx=gpu_ctx)
    for i in range(3):
        got = host(job.run())
        assert same(got, want), f"run {i + 1}"
        assert job.last_reused == (i > 0) and job.last_weights_adopted == (i > 0) and job.last_num_bands == BANDS
    job.release_geometry()
    assert same(host(job.run()), want) and not job.last_reused
    assert same(host(job.run()), want) and job.last_weights_adopted


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ring", "grid"])
def test_new_frames_of_the_same_rig(gpu_ctx, name):
    r = rig(name)
    job = StitchJob(r["frames"], r["cams"], num_bands=BANDS, ctx=gpu_ctx)
    first = host(job.run())
    got = host(job.run(frames=r["other"]))
    assert job.last_reused and job.last_weights_adopted
    assert same(got, fresh(gpu_ctx, r["other"], r["cams"], num_bands=BANDS)) and not np.array_equal(got[0], first[0])
    assert same(host(job.run(frames=r["frames"])), first)
    with pytest.raises(S.StitchingError, match="same rig, same sizes"):
        job.run(frames=[f[:, :-8] for f in r["frames"]])
    with pytest.raises(S.StitchingError, match="same rig, same sizes"):
        job.run(frames=r["frames"][:-1])


@pytest.mark.gpu
def test_a_changed_key_is_a_first_run(gpu_ctx):
    """another scale, another trig / remap / pyrDown mode between runs: the next run equals a fresh job made under that setting, and
    after switching back it does again"""
    r = rig("ring")
    job = StitchJob(r["frames"], r["cams"], num_bands=BANDS, ctx=gpu_ctx)
    base = fresh(gpu_ctx, r["frames"], r["cams"], num_bands=BANDS)
    assert same(host(job.run()), base) and same(host(job.run()), base) and job.last_weights_adopted

    job.warper.set_scale(r["cams2"])
    want = fresh(gpu_ctx, r["frames"], r["cams"], scale_cams=r["cams2"], num_bands=BANDS)
    assert same(host(job.run()), want) and not job.last_reused and not np.array_equal(want[0].shape, base[0].shape)
    assert same(host(job.run()), want) and job.last_reused
    job.warper.set_scale(r["cams"])
    assert same(host(job.run()), base) and not job.last_reused

    switches = [(config.set_trig_mode, ("glibc",), lambda p: (p,)), (config.set_remap_mode, ("float",), lambda p: (p,)),
                (config.set_pyrdown_mode, ("simd-hv", 8), lambda p: p)]
    for setter, args, back in switches:
        assert same(host(job.run()), base) and job.last_reused
        prev = setter(*args)
        try:
            want = fresh(gpu_ctx, r["frames"], r["cams"], num_bands=BANDS)
            assert same(host(job.run()), want) and not job.last_reused, setter.__name__
            assert same(host(job.run()), want) and job.last_reused
            # the generic pyrDown kernels keep no occupancy maps: such a blender's weights are not kept, the masks and ROIs are
            assert job.last_weights_adopted == (setter is not config.set_pyrdown_mode)
        finally:
            setter(*back(prev))
        assert same(host(job.run()), base) and not job.last_reused, setter.__name__


@pytest.mark.gpu
def test_host_seam_masks_grey_masks_and_seam_cell_crops(gpu_ctx):
    r = rig("tight")
    seams = low_res_seams(gpu_ctx, r["frames"], r["cams"])
    want = fresh(gpu_ctx, r["frames"], r["cams"], num_bands=BANDS, seam_masks=seams)
    job = StitchJob(r["frames"], r["cams"], num_bands=BANDS, ctx=gpu_ctx, seam_masks=seams)
    for i in range(3):
        assert same(host(job.run()), want), f"run {i + 1}"
        assert job.last_reused == (i > 0) and job.last_weights_adopted == (i > 0)
    print("seam-cell rectangles:", job.last_crop)
    assert job.last_crop is not None and any(c is not None for c in job.last_crop)  # cells are cut: the kept rectangles are no ROIs
    assert same(host(job.run(frames=r["other"])), fresh(gpu_ctx, r["other"], r["cams"], num_bands=BANDS, seam_masks=seams))
    # the whole images with grey masks (no seam-cell crops)
    want = fresh(gpu_ctx, r["frames"], r["cams"], num_bands=BANDS, seam_masks=seams, crop_to_masks=False)
    job = StitchJob(r["frames"], r["cams"], num_bands=BANDS, ctx=gpu_ctx, seam_masks=seams, crop_to_masks=False)
    for i in range(3):
        assert same(host(job.run()), want) and job.last_crop is None and job.last_weights_adopted == (i > 0)


def block_gains(sizes, block, seed=99):
    rng = np.random.default_rng(seed)
    comp = S.ExposureErrorCompensator("gain_blocks", block_size=block, estimator=object())
    comp.set_gains([rng.uniform(0.7, 1.4, ((h + block - 1) // block, (w + block - 1) // block)).astype(np.float32) for w, h in sizes])
    return comp


@pytest.mark.gpu
@pytest.mark.parametrize("crop_to_masks", [True, False])
def test_host_feed_masks_with_block_gains(gpu_ctx, crop_to_masks):
    r = rig("tight")
    cells, sizes = full_res_cells(gpu_ctx, r["frames"], r["cams"])
    comp = block_gains(sizes, 32)
    kw = dict(num_bands=BANDS, feed_masks=cells, compensator=comp, crop_to_masks=crop_to_masks)
    want = fresh(gpu_ctx, r["frames"], r["cams"], **kw)
    assert not same(want, fresh(gpu_ctx, r["frames"], r["cams"], num_bands=BANDS, feed_masks=cells, crop_to_masks=crop_to_masks))  # gains act
    job = StitchJob(r["frames"], r["cams"], ctx=gpu_ctx, **kw)
    for i in range(3):
        assert same(host(job.run()), want), f"run {i + 1}"
        assert job.last_reused == (i > 0) and job.last_weights_adopted == (i > 0)
    assert same(host(job.run(frames=r["other"])), fresh(gpu_ctx, r["other"], r["cams"], **kw))


@pytest.mark.gpu
@pytest.mark.parametrize("blender_type", ["multiband", "feather"])
def test_a_prepared_cropper(gpu_ctx, blender_type):
    r = rig("ring")
    low = [S.resize_linear_exact(f, (W // 2, H // 2), ctx=gpu_ctx, device_resident=False) for f in r["frames"]]
    wp = S.Warper("spherical", ctx=gpu_ctx)
    wp.set_scale(r["cams"])
    imgs, masks, rois = wp.warp_images_and_masks(low, r["cams"], 0.5)
    corners, sizes = [q[0:2] for q in rois], [q[2:4] for q in rois]
    cropper = S.Cropper()
    cropper.prepare(imgs, masks, corners, sizes)
    c_imgs, c_masks = list(cropper.crop_images(imgs)), list(cropper.crop_images(masks))
    c_corners, _ = cropper.crop_rois(corners, sizes)
    seams = [np.asarray(m) for m in S.SeamFinder("voronoi", estimator=S.SeamEstimator("voronoi")).find(c_imgs, c_corners, c_masks)]
    for extra in (dict(), dict(seam_masks=seams)):
        kw = dict(blender_type=blender_type, num_bands=BANDS if blender_type == "multiband" else None, cropper=cropper, crop_aspect=2.0, **extra)
        want = fresh(gpu_ctx, r["frames"], r["cams"], **kw)
        job = StitchJob(r["frames"], r["cams"], ctx=gpu_ctx, **kw)
        for i in range(3):
            assert same(host(job.run()), want), f"run {i + 1}"
            assert job.last_reused == (i > 0) and job.last_weights_adopted == (i > 0 and blender_type == "multiband")
        assert same(host(job.run(frames=r["other"])), fresh(gpu_ctx, r["other"], r["cams"], **kw))


def overwrite(ctx, dev, arr):
    """what a caller may do with a device mask it owns: new bytes in the same buffer"""
    hip = next(C.CDLL(line.split()[-1]) for line in open("/proc/self/maps") if "libamdhip64" in line)
    hip.hipMemcpy2D.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int]
    ctx.sync()
    a = np.ascontiguousarray(arr, np.uint8)
    assert a.shape == dev.shape
    assert hip.hipMemcpy2D(dev.device_ptr(), dev.stride_bytes, a.ctypes.data, a.strides[0], a.shape[1], a.shape[0], 1) == 0  # host to device


@pytest.mark.gpu
def test_device_feed_masks_are_the_callers(gpu_ctx):
    """masks given as device arrays may be rewritten between runs: nothing of such a job is kept"""
    r = rig("ring")
    cells, _ = full_res_cells(gpu_ctx, r["frames"], r["cams"])
    dev = [S.DeviceImage.from_numpy(m, gpu_ctx) for m in cells]
    job = StitchJob(r["frames"], r["cams"], num_bands=BANDS, ctx=gpu_ctx, feed_masks=dev)
    assert not job.reuse_geometry
    one = host(job.run())
    assert same(one, fresh(gpu_ctx, r["frames"], r["cams"], num_bands=BANDS, feed_masks=cells))
    changed = [m.copy() for m in cells]
    changed[1][: changed[1].shape[0] // 2] = 0  # image 1 gives up the upper half of its cell
    overwrite(gpu_ctx, dev[1], changed[1])
    two = host(job.run())
    assert not job.last_reused and not job.last_weights_adopted
    assert same(two, fresh(gpu_ctx, r["frames"], r["cams"], num_bands=BANDS, feed_masks=changed)) and not same(two, one)


def blend(ctx, corners, sizes, feeds, keep=False, use=None):
    """-> (panorama, mask, kept weights or None, adopted)"""
    bl = S.Blender("multiband", synthetic.blend_strength_for_bands(BANDS, *S.Blender.result_roi(corners, sizes)[2:4]), ctx=ctx)
    bl.prepare(corners, sizes)
    for img, mask, corner in feeds:
        bl.feed(img, mask, corner)
    kept = bl.blender.keep_weights() if keep else None
    adopted = bl.blender.use_weights(use) if use is not None else False
    pano, pmask = bl.blend()
    return np.asarray(pano), np.asarray(pmask), kept, adopted


@pytest.mark.gpu
def test_blender_keep_and_use(gpu_ctx):
    """through Blender directly: weights are adopted only by a blender whose feeds match the record field for field"""
    r = rig("grid")
    wp = S.Warper("spherical", ctx=gpu_ctx)
    wp.set_scale(r["cams"])
    S.set_device_resident(True)
    try:
        imgs, masks, rois = wp.warp_images_and_masks(r["frames"], r["cams"])
        imgs2, _, _ = wp.warp_images_and_masks(r["other"], r["cams"])
    finally:
        S.set_device_resident(False)
    corners, sizes = [q[0:2] for q in rois], [q[2:4] for q in rois]
    # room for one image a pixel to the right: the same prepared roi for every blender here
    p_corners, p_sizes = corners + [(corners[0][0] + 1, corners[0][1])], sizes + [sizes[0]]
    feeds = list(zip(imgs, masks, corners))
    pano, pmask, kept, _ = blend(gpu_ctx, p_corners, p_sizes, feeds, keep=True)
    assert kept is not None
    # the same feeds, new pixels: adopted, and equal to a plain blend
    feeds2 = list(zip(imgs2, masks, corners))
    want2 = blend(gpu_ctx, p_corners, p_sizes, feeds2)
    got2 = blend(gpu_ctx, p_corners, p_sizes, feeds2, use=kept)
    assert got2[3] is True and same(got2, want2) and not np.array_equal(want2[0], pano)
    assert same(blend(gpu_ctx, p_corners, p_sizes, feeds, use=kept), (pano, pmask))
    # an int16 image among the feeds: nothing adopted
    s16 = [(np.asarray(imgs[0]).astype(np.int16), masks[0], corners[0])] + feeds[1:]
    got = blend(gpu_ctx, p_corners, p_sizes, s16, use=kept)
    assert got[3] is False and same(got, blend(gpu_ctx, p_corners, p_sizes, s16))
    # another corner: nothing adopted
    moved = [(imgs[0], masks[0], (corners[0][0] + 1, corners[0][1]))] + feeds[1:]
    got = blend(gpu_ctx, p_corners, p_sizes, moved, use=kept)
    assert got[3] is False and same(got, blend(gpu_ctx, p_corners, p_sizes, moved)) and not np.array_equal(got[0], pano)
    # another mask buffer with the same bytes, one image fewer, another band count: nothing adopted
    copy = [(imgs[0], S.DeviceImage.from_numpy(np.asarray(masks[0]), gpu_ctx), corners[0])] + feeds[1:]
    got = blend(gpu_ctx, p_corners, p_sizes, copy, use=kept)
    assert got[3] is False and same(got, (pano, pmask))
    assert blend(gpu_ctx, p_corners, p_sizes, feeds[:-1], use=kept)[3] is False
    # a blender that adopted weights keeps none of its own, and a freed handle is never adopted
    bl = S.Blender("multiband", 5, ctx=gpu_ctx)
    bl.prepare(p_corners, p_sizes)
    assert bl.blender.num_bands() != BANDS
    for f in feeds:
        bl.feed(*f)
    assert bl.blender.use_weights(kept) is False
    bl.blend()
    kept.free()
    assert blend(gpu_ctx, p_corners, p_sizes, feeds, use=kept)[3] is False


def profile(ctx, job):
    ctx.sync()
    ctx.prof_reset()
    job.run()
    ctx.sync()
    return {e["kernel"]: e for e in ctx.prof_results() if e["calls"]}


@pytest.mark.gpu
def test_the_second_run_skips_the_roi_pass_and_the_weight_half(gpu_ctx):
    """the context's profiler: no warp_roi in the second run, fewer algorithmic bytes in its pyrDown launches"""
    r = rig("grid")
    gpu_ctx.prof_enable(True)
    try:
        plain = profile(gpu_ctx, StitchJob(r["frames"], r["cams"], num_bands=BANDS, ctx=gpu_ctx, reuse_geometry=False))
        job = StitchJob(r["frames"], r["cams"], num_bands=BANDS, ctx=gpu_ctx)
        first, second = profile(gpu_ctx, job), profile(gpu_ctx, job)
    finally:
        gpu_ctx.prof_enable(False)
        gpu_ctx.prof_reset()
    print({k: (v["calls"], v["algo_bytes"]) for k, v in first.items()}, {k: (v["calls"], v["algo_bytes"]) for k, v in second.items()})
    assert job.last_weights_adopted
    assert "warp_roi" in first and "warp_roi" in plain and "warp_roi" not in second
    for k in ("mb_down0", "mb_down"):
        assert first[k]["calls"] == second[k]["calls"] == plain[k]["calls"]
        assert first[k]["algo_bytes"] == plain[k]["algo_bytes"]
        assert 0 < second[k]["algo_bytes"] < first[k]["algo_bytes"]
    # the gathers read what they always read
    for k in first:
        if k.startswith("mb_level") or k == "mb_coarse":
            assert first[k]["algo_bytes"] == second[k]["algo_bytes"]


@pytest.mark.gpu
def test_composer_runs_one_job_per_plan(gpu_ctx):
    r = rig("ring")
    images = S.Images.of(r["frames"], 0.2, 0.05, -1)
    mw, mh = images.get_scaled_img_sizes(S.Images.Resolution.MEDIUM)[0]
    cams = synthetic.ring_cameras(N, mw, mh, focal_factor=0.75, span_deg=180.0)
    kw = dict(medium_megapix=0.2, low_megapix=0.05, finder="voronoi")
    comp = S.Composer(ctx=gpu_ctx, **kw)
    plan = comp.prepare(r["frames"], cams)
    want = np.asarray(S.Composer(ctx=gpu_ctx, **kw).compose(r["frames"], cams))
    a = host(comp.run(plan))
    b = host(comp.run(plan, images=r["frames"]))
    assert plan.job is not None and plan.job.last_reused and plan.job.last_weights_adopted
    assert np.array_equal(a[0], want) and same(a, b)
    # new frames of the rig on the plan: what a fresh plan's first run gives
    c = host(comp.run(plan, images=r["other"]))
    assert plan.job.last_reused
    other = S.Composer(ctx=gpu_ctx, **kw)
    assert same(c, host(other.run(other.prepare(r["frames"], cams), images=r["other"]))) and not np.array_equal(c[0], a[0])
    with pytest.raises(S.StitchingError, match="same rig, same sizes"):
        comp.run(plan, images=[f[:, :-8] for f in r["frames"]])
