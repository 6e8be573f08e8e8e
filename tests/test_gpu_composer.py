"""Composer: cameras in, panorama out.  Composer.compose must equal the chain a user would write by hand from the public classes in
Stitcher.stitch's order (stitching/stitcher.py:108-128), every class built with estimator= the device estimators — panorama and mask
byte for byte.  The frames are 96 x 72, where the default megapixel settings would make all three scales 1: the cases set
medium_megapix / low_megapix so that MEDIUM (82 x 61), LOW (52 x 39) and FINAL (96 x 72) differ; one case keeps the true defaults."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import stitching_amd as S
from stitching_amd import cropper as cropper_mod
from stitching_amd import pipeline, synthetic
from tests import glue_trace as GT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, W, H = 4, 96, 72
SCALED = {"medium_megapix": 0.005, "low_megapix": 0.002}
R = S.Images.Resolution


def rig(first=0, **kw):
    """frames and the cameras as registration leaves them: at MEDIUM scale"""
    frames = synthetic.make_frames(range(first, first + N), W, H)
    images = S.Images.of(frames, kw.get("medium_megapix", 0.6), kw.get("low_megapix", 0.1), -1)
    mw, mh = images.get_scaled_img_sizes(R.MEDIUM)[0]
    return frames, synthetic.ring_cameras(N, mw, mh, focal_factor=0.75, span_deg=110.0)


def chain(ctx, frames, cams, warper_type="spherical", blender_type="multiband", blend_strength=5, crop=True, compensator="gain_blocks",
          finder="voronoi", nr_feeds=1, block_size=32, medium_megapix=0.6, low_megapix=0.1, final_megapix=-1, gains_of=None):
    """Stitcher.stitch after estimate_scale, written out with the public classes (device residency on)"""
    S.set_device_resident(True)
    try:
        images = S.Images.of(list(frames), medium_megapix, low_megapix, final_megapix)
        medium = list(images.resize(R.MEDIUM))
        wp = S.Warper(warper_type, ctx=ctx)
        wp.set_scale(cams)
        low = list(images.resize(R.LOW, medium))
        sizes, aspect = images.get_scaled_img_sizes(R.LOW), images.get_ratio(R.MEDIUM, R.LOW)
        imgs = list(wp.warp_images(low, cams, aspect))
        masks = list(wp.create_and_warp_masks(sizes, cams, aspect))
        corners, sizes = wp.warp_rois(sizes, cams, aspect)
        cr = S.Cropper(crop)
        cr.prepare(imgs, masks, corners, sizes)
        masks, imgs = list(cr.crop_images(masks)), list(cr.crop_images(imgs))
        corners, sizes = cr.crop_rois(corners, sizes)
        est = None
        if compensator in ("channel", "channel_blocks"):
            est = S.ExposureEstimator(compensator, nr_feeds, block_size)
        elif compensator != "no":
            est = S.ExposureEstimator(compensator)
        comp = S.ExposureErrorCompensator(compensator, nr_feeds, block_size, estimator=est or object())
        if gains_of is None:
            comp.feed(corners, imgs, masks)
        else:  # the video case: the gains another set of frames left
            comp.set_gains(gains_of.gains)
        seams = S.SeamFinder(finder, estimator=S.SeamEstimator(finder)).find(imgs, corners, masks)
        final = list(images.resize(R.FINAL))
        sizes, aspect = images.get_scaled_img_sizes(R.FINAL), images.get_ratio(R.MEDIUM, R.FINAL)
        imgs = list(wp.warp_images(final, cams, aspect))
        masks = list(wp.create_and_warp_masks(sizes, cams, aspect))
        corners, sizes = wp.warp_rois(sizes, cams, aspect)
        lir = images.get_ratio(R.LOW, R.FINAL)
        masks, imgs = list(cr.crop_images(masks, lir)), list(cr.crop_images(imgs, lir))
        corners, sizes = cr.crop_rois(corners, sizes, lir)
        imgs = [comp.apply(i, c, im, m) for i, (c, im, m) in enumerate(zip(corners, imgs, masks))]
        fed = [S.SeamFinder.resize(s, m) for s, m in zip(seams, masks)]
        bl = S.Blender(blender_type, blend_strength, ctx=ctx)
        bl.prepare(corners, sizes)
        for im, mk, c in zip(imgs, fed, corners):
            bl.feed(im, mk, c)
        pano, pmask = bl.blend()
        return pano.numpy(), pmask.numpy()
    finally:
        S.set_device_resident(False)


CASES = {
    "defaults_voronoi": dict(finder="voronoi", **SCALED),
    "true_defaults_voronoi": dict(finder="voronoi"),
    "no_crop": dict(finder="voronoi", crop=False, **SCALED),
    "no_compensator": dict(finder="voronoi", compensator="no", **SCALED),
    "feather": dict(finder="voronoi", blender_type="feather", **SCALED),
    "plane_channel_blocks_no_finder": dict(finder="no", warper_type="plane", compensator="channel_blocks", block_size=16, **SCALED),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_compose_equals_the_hand_written_chain(gpu_ctx, name):
    kw = CASES[name]
    frames, cams = rig(**kw)
    want_pano, want_mask = chain(gpu_ctx, frames, cams, **kw)
    comp = S.Composer(ctx=gpu_ctx, **kw)
    plan = comp.prepare(frames, cams)
    pano, mask = comp.run(plan)
    assert isinstance(pano, S.DeviceImage) and isinstance(mask, S.DeviceImage) and S.device_resident() is False
    assert all(isinstance(m, S.DeviceImage) for m in plan.seam_masks)  # the plan's results stay on the device
    assert np.array_equal(mask.numpy(), want_mask) and np.array_equal(pano.numpy(), want_pano)
    assert np.array_equal(comp.compose(frames, cams).numpy(), want_pano)
    if kw.get("crop", True) and "medium_megapix" in kw:
        whole, _ = S.Composer(ctx=gpu_ctx, **dict(kw, crop=False)).run(S.Composer(ctx=gpu_ctx, **dict(kw, crop=False)).prepare(frames, cams))
        assert pano.shape[0] < whole.shape[0]  # cropped


@pytest.mark.gpu
def test_run_on_new_frames_of_the_same_rig(gpu_ctx):
    """the video case: cropper and voronoi seams depend on the geometry alone, so without a compensator a plan prepared from other
    frames composes new ones exactly as compose() does; with one, the plan's gains are kept"""
    kw = dict(finder="voronoi", compensator="no", **SCALED)
    old, cams = rig(0, **kw)
    new, _ = rig(4, **kw)
    comp = S.Composer(ctx=gpu_ctx, **kw)
    plan = comp.prepare(old, cams)
    pano, mask = comp.run(plan, images=new)
    want = comp.compose(new, cams).numpy()
    assert np.array_equal(pano.numpy(), want) and not np.array_equal(want, comp.run(plan)[0].numpy())
    kw = dict(finder="voronoi", **SCALED)
    comp = S.Composer(ctx=gpu_ctx, **kw)
    plan = comp.prepare(old, cams)
    gains = [g.copy() for g in plan.compensator.gains]
    got_pano, got_mask = comp.run(plan, images=new)
    want_pano, want_mask = chain(gpu_ctx, new, cams, gains_of=plan.compensator, **kw)  # the OLD frames' gains on the new frames
    assert np.array_equal(got_pano.numpy(), want_pano) and np.array_equal(got_mask.numpy(), want_mask)
    assert not np.array_equal(want_pano, chain(gpu_ctx, new, cams, **kw)[0])  # ... which are not the new frames' own gains
    assert all(np.array_equal(g, h) for g, h in zip(gains, plan.compensator.gains))
    with pytest.raises(S.StitchingError, match="same rig, same sizes"):
        comp.run(plan, images=[f[:, :-1] for f in new])


CHILD = r"""
import sys
sys.modules["cv2"] = None
sys.path.insert(0, sys.argv[1])
import hashlib, json
import numpy as np
import stitching_amd as S
from stitching_amd import synthetic
frames = synthetic.make_frames(range(4), 96, 72)
cams = synthetic.ring_cameras(4, 82, 61, focal_factor=0.75, span_deg=110.0)
pano = S.Composer(finder="voronoi", medium_megapix=0.005, low_megapix=0.002).compose(frames, cams).numpy()
out = {"sha": hashlib.sha256(np.ascontiguousarray(pano).tobytes()).hexdigest(), "shape": list(pano.shape)}
try:
    S.Composer(finder="dp_color", medium_megapix=0.005, low_megapix=0.002).compose(frames, cams)
    out["dp"] = "completed"
except S.StitchingError as e:
    out["dp"] = str(e)
print(json.dumps(out))
"""


@pytest.mark.gpu
def test_no_cv2_in_a_fresh_process(gpu_ctx):
    """a child process in which `import cv2` fails: "voronoi" composes all the same (nothing on its way looks for OpenCV), "dp_color"
    fails with SeamFinder's own error"""
    kw = dict(finder="voronoi", **SCALED)
    frames, cams = rig(**kw)
    want = S.Composer(ctx=gpu_ctx, **kw).compose(frames, cams).numpy()
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["shape"] == list(want.shape) and out["sha"] == hashlib.sha256(want.tobytes()).hexdigest()
    assert "needs OpenCV" in out["dp"]


def _kind(v):
    if isinstance(v, np.floating):
        return "np"
    if isinstance(v, (list, tuple)) and not (isinstance(v, tuple) and len(v) == 2 and all(isinstance(x, (int, np.integer)) for x in v)):
        return "seq"
    if isinstance(v, tuple):
        return "tuple"
    if isinstance(v, (np.ndarray, S.DeviceImage)):
        return "img"
    return type(v).__name__


WARPS = ("warp_images", "create_and_warp_masks", "warp_rois", "warp_images_and_masks")


def _stages(calls):
    """(class, stage, argument kinds): the three calls of Stitcher.warp (stitcher.py:185-189) and the product's fused
    warp_images_and_masks / its ROI pass are one "warp" stage; a repeated set_scale (StitchJob's own Warper) is one.
    What this normalisation can and cannot see: it fixes the ORDER set_scale -> warp -> create_panorama -> warp -> prepare -> feed ->
    blend and the kinds of the first three arguments; consecutive warp calls and consecutive feeds are merged, so an extra ROI pass or
    a second whole warp inside a stage would go unnoticed.  The recording holds no Cropper events (the reference's Cropper is glue,
    not a back-end class), so Warper and Blender — with Cropper.prepare's create_panorama — are all the fixture allows to compare."""
    out = []
    for cls, name, kinds in calls:
        if name in WARPS:
            name, kinds = "warp", kinds[:3]
        if out and out[-1][:2] == (cls, name) and name in ("warp", "feed"):
            assert out[-1][2] == kinds, (out[-1], kinds)
            continue
        if name == "set_scale" and (cls, name, kinds) in out:
            continue
        out.append((cls, name, kinds))
    return out


def _recorded_stages():
    tr = GT.load(os.path.join(ROOT, "tests", "golden", "reference_glue", "stitcher_crop.json"))
    label, calls = {}, []
    for e in tr["events"]:
        if e["op"] == "new":
            label[e["obj"]] = e["cls"]
        cls = e.get("cls") or label.get(e.get("obj"))
        if e["op"] in ("call", "static") and cls in ("Warper", "Blender"):
            def kind(a):
                if not isinstance(a, dict):
                    return type(a).__name__
                k = next(iter(a))
                return {"list": "seq", "gen": "seq", "ref": "img", "view": "img", "umat": "img"}.get(k, k)
            calls.append((cls, e["name"], tuple(kind(a) for a in e.get("args", []))))
    return _stages(calls)


@pytest.mark.gpu
def test_call_shapes_follow_the_recorded_reference_glue(gpu_ctx, monkeypatch):
    """what Composer asks of its Warper and Blender (Cropper.prepare's panorama mask included), in the order and with the kinds of
    arguments the unmodified reference glue asked of its own classes (tests/golden/reference_glue/stitcher_crop.json)"""
    calls, depth = [], [0]

    def spy(base, label, names):
        ns = {}
        for name in names:
            raw = base.__dict__.get(name)
            fn = getattr(base, name)

            def wrapper(*a, _fn=fn, _name=name, _cm=isinstance(raw, classmethod), **k):
                args = a if _cm else a[1:]
                if depth[0] == 0:
                    calls.append((label, _name, tuple(_kind(x) for x in args)))
                depth[0] += 1
                try:
                    return _fn(*a, **k)
                finally:
                    depth[0] -= 1
            ns[name] = staticmethod(wrapper) if isinstance(raw, classmethod) else wrapper
        return type(base.__name__, (base,), ns)

    W_ = spy(S.Warper, "Warper", ("set_scale",) + WARPS)
    B_ = spy(S.Blender, "Blender", ("create_panorama", "prepare", "feed", "blend"))
    monkeypatch.setattr(pipeline, "Warper", W_)
    monkeypatch.setattr(pipeline, "Blender", B_)
    monkeypatch.setattr(cropper_mod, "Blender", B_)
    kw = dict(finder="voronoi", **SCALED)
    frames, cams = rig(**kw)
    S.Composer(ctx=gpu_ctx, **kw).compose(frames, cams)
    got, want = _stages(calls), _recorded_stages()
    print(json.dumps(got), json.dumps(want))
    assert got == want


@pytest.mark.gpu
def test_a_context_of_its_own(gpu_ctx):
    """Composer(ctx=) on host frames: every stage — the resizes and the cropper's panorama mask included — runs on that context,
    and the result is the default context's"""
    kw = dict(finder="voronoi", **SCALED)
    frames, cams = rig(**kw)
    want_pano, want_mask = S.Composer(ctx=gpu_ctx, **kw).run(S.Composer(ctx=gpu_ctx, **kw).prepare(frames, cams))
    other = S.Context(0)
    try:
        assert other is not gpu_ctx and other.handle.value != gpu_ctx.handle.value
        comp = S.Composer(ctx=other, **kw)
        plan = comp.prepare(frames, cams)
        assert all(f.ctx is other for f in plan.frames) and all(m.ctx is other for m in plan.seam_masks)
        pano, mask = comp.run(plan)
        assert pano.ctx is other and mask.ctx is other
        assert np.array_equal(pano.numpy(), want_pano.numpy()) and np.array_equal(mask.numpy(), want_mask.numpy())
        pano2, _ = comp.run(plan, images=[f.copy() for f in frames])  # host frames again: uploaded on `other`
        assert pano2.ctx is other and np.array_equal(pano2.numpy(), want_pano.numpy())
        del comp, plan, pano, mask, pano2
    finally:
        import gc

        gc.collect()
        other.close()
