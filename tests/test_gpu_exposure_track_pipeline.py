"""Exposure tracking through the pipeline classes: StitchJob(exposure_tracker=) and Composer.prepare(exposure_tracker=) against the
contract (tests/numpy_exposure_track.py).  The rig is that of tests/test_gpu_source_masks_pipeline.py: four 96 x 72 frames, yaw step 14
degrees.  Five sets of frames; from the third on camera 1's frames are multiplied by 1.3 and clipped.  After every run the tracker's
statistics equal the contract's on the images the warper returns for the job's rectangles under the contract's effective gains, its
factors equal the contract's residuals in their float64 bits, and panorama and mask equal, byte for byte, those of an untracked
StitchJob whose compensator was given the contract's effective gains by set_gains."""
import numpy as np
import pytest

import stitching_amd as S
from stitching_amd import synthetic
from stitching_amd.camera import CameraParams
from stitching_amd.distributed import ShardedStitchJob
from stitching_amd.pipeline import StitchJob
from tests import camera_rigs as CR
from tests import numpy_exposure_track as NT

pytestmark = pytest.mark.gpu

N, W, H = 4, 96, 72
YAWS = (-21.0, -7.0, 7.0, 21.0)
RUNS, STEP_AT, STEP = 5, 2, 1.3
STRIDE = 2
_cache = {}


def rig():
    if "rig" not in _cache:
        cams = [CameraParams(focal=0.75 * W, aspect=1.0, ppx=W / 2.0, ppy=H / 2.0,
                             R=CR.rotation(yaw, 1.5 if i % 2 else -1.5, 0.8 * (i - 1)).astype(np.float32)) for i, yaw in enumerate(YAWS)]
        sets = []
        for k in range(RUNS):
            frames = [f.copy() for f in synthetic.make_frames(range(10 * k, 10 * k + N), W, H)]
            if k >= STEP_AT:   # camera 1 steps its exposure
                frames[1] = np.clip(np.rint(frames[1].astype(np.float64) * STEP), 0, 255).astype(np.uint8)
            sets.append(frames)
        _cache["rig"] = (sets, cams)
    return _cache["rig"]


def plan_compensator(kind, seed=1):
    """a compensator of `kind` with constructed gains, as a low-resolution pass would leave it"""
    rng = np.random.default_rng(seed)
    comp = S.ExposureErrorCompensator(kind, estimator=object())
    if kind == "gain":
        comp.set_gains([rng.uniform(0.8, 1.25, (1, 1)) for _ in range(N)])
    elif kind == "channel":
        comp.set_gains([rng.uniform(0.8, 1.25, (3, 1)) for _ in range(N)])
    elif kind == "gain_blocks":
        comp.set_gains([rng.uniform(0.8, 1.25, (3, 4)).astype(np.float32) for _ in range(N)])
    elif kind == "channel_blocks":
        comp.set_gains([rng.uniform(0.8, 1.25, (3, 4, 3)).astype(np.float32) for _ in range(N)])
    return comp


def plan_gains(comp):
    return None if comp is None or comp.compensator_type == "no" else [np.array(g, copy=True) for g in comp.gains]


def host(pair):
    return tuple(np.asarray(a) for a in pair)


def same(a, b):
    return a[0].shape == b[0].shape and np.array_equal(a[1], b[1]) and np.array_equal(a[0], b[0])


def final_images(ref, g, comp):
    """the warped, compensated images and the warped masks of the rectangles g.rects, as an untracked job `ref` with compensator `comp`
    makes them: gain in the warp (or the lens path's second pass) where the tracked job's geometry says so, else apply_all behind it"""
    imgs, masks, _ = ref.warper.warp_images_and_masks(ref.frames, ref.cameras, ref.camera_aspect, rects=g.rects,
                                                      compensator=comp if g.gain_in_warp else None, camera_arrays=ref._cam_arrays)
    if not g.gain_in_warp:
        imgs = comp.apply_all(g.gain_corners, imgs, None, sub=g.gain_sub, ctx=ref.ctx)
    return [np.asarray(i) for i in imgs], [np.asarray(m) for m in masks]


def follow(gpu_ctx, tracker, plan, run, sets, untracked_kw, runs=RUNS):
    """`run(k, frames)` makes panorama k of the tracked job and returns (pano, mask, job).  Checks every run against the contract and
    an untracked job; -> the contract's residuals of every run and the statistics of every run"""
    _, cams = rig()
    plan_kind = "no" if plan is None else plan.compensator_type
    P = plan_gains(plan)
    version = None if plan is None else plan.gains_version
    eff_kind = NT.effective_kind(plan_kind, tracker.kind)
    r = np.ones((N, NT.planes_of(tracker.kind)))
    prev, rs, all_stats = None, [], []
    for k in range(runs):
        frames = sets[k]
        if prev is not None:
            r, _ = NT.track_update(tracker.kind, r, prev[0], prev[1], prev[2], rate=tracker.rate, limits=tracker.limits)
        pano, pmask, job = run(k, frames)
        got = (np.asarray(pano), np.asarray(pmask))
        assert job.last_reused == (k > 0)
        assert tracker.factors.dtype == np.float64 and tracker.factors.tobytes() == r.tobytes(), (k, tracker.factors, r)
        comp = S.ExposureErrorCompensator(eff_kind, estimator=object())
        comp.set_gains(NT.effective_gains(plan_kind, P, r, tracker.kind))
        ref = StitchJob(frames, cams, ctx=gpu_ctx, compensator=comp, **untracked_kw)
        want = host(ref.run())
        assert same(got, want), (k, int(np.count_nonzero(got[0] != want[0])))
        g = job._geometry
        imgs, masks = final_images(ref, g, comp)
        vs, origins, self_counts = NT.grids(g.rects, masks, tracker.stride)
        stats = NT.pair_stats(g.rects, vs, origins, imgs, tracker.stride)
        pairs, counts, dev = tracker.last_stats
        assert pairs.tolist() == [list(p) for p in NT.pair_jobs(g.rects)] and np.array_equal(counts, self_counts)
        assert np.array_equal(dev, stats), (k, dev, stats)
        prev = (NT.pair_jobs(g.rects), self_counts, stats)
        rs.append(r.copy())
        all_stats.append(stats)
    if plan is not None:   # read, never written
        assert plan.gains_version == version
        assert all(np.array_equal(a, b) for a, b in zip(plan_gains(plan) or [], P or []))
    return rs, all_stats


@pytest.mark.parametrize("rate", [1.0, 0.25])
@pytest.mark.parametrize("tracker_kind", ["gain", "channel"])
@pytest.mark.parametrize("plan_kind", ["no", "gain", "channel", "gain_blocks", "channel_blocks"])
def test_tracked_job_equals_the_contract(gpu_ctx, plan_kind, tracker_kind, rate):
    sets, cams = rig()
    plan = plan_compensator(plan_kind)
    tracker = S.ExposureTracker(tracker_kind, rate=rate, stride=STRIDE)
    job = StitchJob(sets[0], cams, ctx=gpu_ctx, compensator=plan, exposure_tracker=tracker)
    key = job.geometry_key()

    def run(k, frames):
        pano, pmask = job.run() if k == 0 else job.run(frames=frames)
        return pano, pmask, job

    rs, stats = follow(gpu_ctx, tracker, plan, run, sets, {})
    assert job.geometry_key() == key   # the factors are no part of the rig's key
    assert all((s[:, 0] > 0).sum() >= 3 for s in stats)
    # run 0 applies the plan's gains alone; from run 1 on the residuals move
    assert np.array_equal(rs[0], np.ones_like(rs[0])) and all(not np.array_equal(r, np.ones_like(r)) for r in rs[1:])
    assert tracker.info["updates"] == RUNS - 1 and tracker.info["solve_failures_total"] == 0 and tracker.info["pairs"] == len(stats[0])
    assert tracker.info["tile_jobs"] >= (stats[0][:, 0] > 0).sum() and tracker.info["grid_bytes"] > 0 and tracker.info["stats_ms"] > 0.0
    # release_geometry frees the grids; the factors survive, and the next run is a first run that goes on from them (and from the
    # statistics already collected)
    pairs, counts, last = tracker.last_stats
    nxt, _ = NT.track_update(tracker_kind, rs[-1], pairs, counts, last, rate=rate)
    before = tracker.factors
    job.release_geometry()
    assert tracker.factors.tobytes() == before.tobytes() == rs[-1].tobytes()
    job.run(frames=sets[-1])
    assert not job.last_reused and tracker.factors.tobytes() == nxt.tobytes()
    tracker.reset()
    assert np.array_equal(tracker.factors, np.ones_like(before)) and tracker.last_stats is None


def test_saturated_samples_are_counted_as_rejected(gpu_ctx):
    sets, cams = rig()
    frames = [f.copy() for f in sets[0]]
    frames[0][:, W // 2:] = 255
    tracker = S.ExposureTracker("gain", stride=STRIDE)
    job = StitchJob(frames, cams, ctx=gpu_ctx, exposure_tracker=tracker)
    job.run()
    assert tracker.last_stats[2][:, 7].sum() > 0
    job.run()
    assert 0.0 < tracker.info["rejected_share"] < 1.0


def test_cropper_job(gpu_ctx):
    """the path with gain_in_warp = False: gains by apply_all on the cropped images"""
    sets, cams = rig()
    low = [S.resize_linear_exact(f, (W // 2, H // 2), ctx=gpu_ctx, device_resident=False) for f in sets[0]]
    wp = S.Warper("spherical", ctx=gpu_ctx)
    wp.set_scale(cams)
    imgs, masks, rois = wp.warp_images_and_masks(low, cams, 0.5)
    cropper = S.Cropper()
    cropper.prepare(imgs, masks, [q[0:2] for q in rois], [q[2:4] for q in rois])
    kw = dict(cropper=cropper, crop_aspect=2.0)
    for plan_kind, tracker_kind in (("gain_blocks", "channel"), ("channel", "gain")):
        plan = plan_compensator(plan_kind, seed=2)
        tracker = S.ExposureTracker(tracker_kind, rate=1.0, stride=STRIDE)
        job = StitchJob(sets[0], cams, ctx=gpu_ctx, compensator=plan, exposure_tracker=tracker, **kw)

        def run(k, frames):
            pano, pmask = job.run() if k == 0 else job.run(frames=frames)
            return pano, pmask, job

        rs, _ = follow(gpu_ctx, tracker, plan, run, sets, kw, runs=4)
        assert not job._geometry.gain_in_warp and not np.array_equal(rs[-1], np.ones_like(rs[-1]))


LENS_K = np.array([[70.0, 0.0, 47.3], [0.0, 70.0, 35.6], [0.0, 0.0, 1.0]])
PINCUSHION = (0.25, 0.05, 0.0, 0.0)


def test_lens_job(gpu_ctx):
    """the warp through the lens: gains are its second pass"""
    sets, cams = rig()
    lens = S.LensMap.brown(LENS_K, PINCUSHION, (W, H), fit="same")
    kw = dict(lenses=lens, source_masks="lens")
    for plan_kind, tracker_kind in (("gain_blocks", "gain"), ("no", "channel")):
        plan = plan_compensator(plan_kind, seed=3)
        tracker = S.ExposureTracker(tracker_kind, rate=0.25, stride=STRIDE)
        job = StitchJob(sets[0], cams, ctx=gpu_ctx, compensator=plan, exposure_tracker=tracker, **kw)

        def run(k, frames):
            pano, pmask = job.run() if k == 0 else job.run(frames=frames)
            return pano, pmask, job

        rs, _ = follow(gpu_ctx, tracker, plan, run, sets, kw, runs=4)
        assert not np.array_equal(rs[-1], np.ones_like(rs[-1]))


def test_composer_prepare_takes_the_tracker(gpu_ctx):
    sets, _ = rig()
    images = S.Images.of(list(sets[0]), 0.6, 0.1, -1)
    mw, mh = images.get_scaled_img_sizes(S.Images.Resolution.MEDIUM)[0]
    cams = [CameraParams(focal=0.75 * mw, aspect=1.0, ppx=mw / 2.0, ppy=mh / 2.0, R=c.R) for c in rig()[1]]
    kw = dict(crop=False, finder="voronoi", compensator="gain_blocks")
    tracker = S.ExposureTracker("gain", rate=1.0, stride=STRIDE)
    composer = S.Composer(ctx=gpu_ctx, **kw)
    plan = composer.prepare(sets[0], cams, exposure_tracker=tracker)
    assert plan.exposure_tracker is tracker
    version, gains = plan.compensator.gains_version, plan_gains(plan.compensator)
    first = host(composer.run(plan))
    assert plan.job.exposure_tracker is tracker and not plan.job.last_reused
    # run 0 applies the plan's own gains: the bytes of a composer without a tracker
    bare = S.Composer(ctx=gpu_ctx, **kw)
    bare_plan = bare.prepare(sets[0], cams)
    assert same(first, host(bare.run(bare_plan)))
    r = np.ones((N, 1))
    for k in (1, 2, 3):
        pairs, counts, stats = tracker.last_stats
        r, _ = NT.track_update("gain", r, pairs, counts, stats, rate=1.0)
        got = host(composer.run(plan, images=sets[k]))
        assert plan.job.last_reused and tracker.factors.tobytes() == r.tobytes()
        comp = S.ExposureErrorCompensator("gain_blocks", estimator=object())
        comp.set_gains(NT.effective_gains("gain_blocks", gains, r, "gain"))
        bare_plan.compensator, bare_plan.job = comp, None
        assert same(got, host(bare.run(bare_plan, images=sets[k]))), k
    assert not np.array_equal(r, np.ones_like(r))
    assert plan.compensator.gains_version == version and all(np.array_equal(a, b) for a, b in zip(plan.compensator.gains, gains))
    with pytest.raises(S.StitchingError, match="ExposureTracker"):
        composer.prepare(sets[0], cams, exposure_tracker="gain")
    with pytest.raises(TypeError):
        composer.compose(sets[0], cams, exposure_tracker=tracker)


def test_refusals(gpu_ctx):
    sets, cams = rig()
    tracker = S.ExposureTracker()
    job = StitchJob(sets[0], cams, ctx=gpu_ctx, exposure_tracker=tracker)
    with pytest.raises(S.StitchingError, match="another StitchJob"):
        StitchJob(sets[0], cams, ctx=gpu_ctx, exposure_tracker=tracker)
    StitchJob(sets[0], cams, ctx=gpu_ctx, exposure_tracker=S.ExposureTracker())   # a tracker of its own is taken
    with pytest.raises(S.StitchingError, match="reuse_geometry"):
        StitchJob(sets[0], cams, ctx=gpu_ctx, reuse_geometry=False, exposure_tracker=S.ExposureTracker())
    dev = [S.as_device(np.full((H, W), 255, np.uint8), gpu_ctx) for _ in range(N)]
    with pytest.raises(S.StitchingError, match="reuse_geometry"):   # a caller's device masks: nothing is kept to measure on
        StitchJob(sets[0], cams, ctx=gpu_ctx, source_masks=dev, exposure_tracker=S.ExposureTracker())
    with pytest.raises(S.StitchingError, match="exposure tracker"):
        ShardedStitchJob(sets[0], cams, cams, 0, 1, ctx=gpu_ctx, exposure_tracker=S.ExposureTracker())
    with pytest.raises(S.StitchingError, match="ExposureTracker"):
        StitchJob(sets[0], cams, ctx=gpu_ctx, exposure_tracker=object())
    for bad in (dict(kind="gain_blocks"), dict(rate=0), dict(rate=1.01), dict(stride=0), dict(stride=65), dict(limits=(2.0, 4.0))):
        with pytest.raises(S.StitchingError):
            S.ExposureTracker(**bad)
    # the refusals left the first job and its tracker as they were
    job.run()
    job.run()
    assert job.last_reused and tracker.info["updates"] == 1
