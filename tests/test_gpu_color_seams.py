"""The project's own colour-aware seam finder on the MI355X (stitching_amd.ColorSeamEstimator, csrc/stx_color_seams.hip) against its
contract tests/numpy_color_seams.py, byte for byte, on seeded random u8 images: cross extents around the wavefront, the workgroup and the
stride loop, seam lengths from 1, both orientations, ragged masks, several dependency levels, residency, the limits, and Composer with
seam_estimator= (also in a child process without cv2).
Inputs built to reach the walk-back window's edge, accumulators above 2^31 and mixed launches: tests/test_gpu_constructed_inputs.py."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import stitching_amd as S
from stitching_amd import config, synthetic
from stitching_amd.pipeline import compose
from stitching_amd.seam_estimation import schedule
from tests import numpy_color_seams as Z

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CROSS = (1, 2, 63, 64, 65, 255, 256, 257, 600)
LENGTHS = (1, 2, 3, 40)
SCALED = {"medium_megapix": 0.005, "low_megapix": 0.002}
R = S.Images.Resolution


def _images(rng, sizes, levels=256):
    """u8 BGR images; levels < 256: few distinct values, so that equal costs (the tie rules) are common"""
    step = 255 // (levels - 1)
    return [(rng.integers(0, levels, (h, w, 3)) * step).astype(np.uint8) for w, h in sizes]


def _masks(rng, sizes, density=0.9):
    return [((rng.random((h, w)) < density) * rng.choice([255, 254, 1], (h, w))).astype(np.uint8) for w, h in sizes]


def _check(corners, imgs, masks, est=None):
    est = est or S.ColorSeamEstimator()
    before_m, before_i = [m.copy() for m in masks], [a.copy() for a in imgs]
    got = est.find(imgs, corners, masks)
    want = Z.find(imgs, corners, masks)
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert isinstance(g, np.ndarray) and g.dtype == np.uint8 and g.shape == w.shape
        assert np.array_equal(g, w), (k, int(np.count_nonzero(g != w)))
    assert all(np.array_equal(m, b) for m, b in zip(masks, before_m)) and all(np.array_equal(a, b) for a, b in zip(imgs, before_i))
    return est, got


def _side_by_side(cross, length, transpose):
    """two images whose overlap is `cross` wide and `length` high (a vertical seam), or the same stacked (a horizontal one)"""
    sizes, corners = [(cross + 3, length), (cross + 2, length)], [(0, 0), (3, 0)]
    if transpose:
        sizes, corners = [(h, w) for w, h in sizes], [(y, x) for x, y in corners]
    assert Z.orientation(corners[0], sizes[0], corners[1], sizes[1]) == (not transpose, True)
    assert Z.pairs(corners, sizes)[0][2][2:] == ((length, cross) if transpose else (cross, length))
    return corners, sizes


@pytest.mark.parametrize("cross", CROSS)
@pytest.mark.parametrize("transpose", (False, True), ids=("vertical", "horizontal"))
def test_two_images(gpu_ctx, cross, transpose):
    rng = np.random.default_rng(cross + 1000 * transpose)
    for length in LENGTHS:
        corners, sizes = _side_by_side(cross, length, transpose)
        for levels in (256, 3):
            _check(corners, _images(rng, sizes, levels), _masks(rng, sizes))
        _check(corners[::-1], _images(rng, sizes[::-1]), _masks(rng, sizes[::-1], 1.0))  # the first image is j


def _ellipse(w, h, value):
    y, x = np.mgrid[0:h, 0:w]
    m = ((x - w / 2 + 0.5) / (w / 2)) ** 2 + ((y - h / 2 + 0.5) / (h / 2)) ** 2 <= 1.0
    return (m * value).astype(np.uint8)


def test_warped_looking_masks(gpu_ctx):
    """elliptical masks with a hole and a notch: `both` is neither a rectangle nor connected; mask values 1, 254 and 255"""
    rng = np.random.default_rng(21)
    sizes = [(150, 110), (140, 120), (131, 97)]
    corners = [(0, 0), (83, -9), (40, 61)]
    masks = [_ellipse(w, h, v) for (w, h), v in zip(sizes, (255, 254, 1))]
    masks[0][40:70, 100:125] = 0   # a hole inside the overlap with image 1
    masks[1][0:70, 28:36] = 0      # a notch from the top edge: cuts `both` in two
    masks[1][80:, 10:60] = np.where(masks[1][80:, 10:60] != 0, 255, 0)
    masks[2][30:40, :] = 0         # a band: two components
    x, y, w, h = Z.pairs(corners, sizes)[0][2]
    both = (masks[0][y:y + h, x:x + w] != 0) & (masks[1][y + 9:y + 9 + h, x - 83:x - 83 + w] != 0)
    assert both.any() and not both.all()
    est, got = _check(corners, _images(rng, sizes, 5), masks)
    assert est.info["pairs"] == 3
    assert any(np.any(g == 254) for g in got) and any(np.any(g == 1) for g in got) and any(np.any(g == 255) for g in got)


@pytest.mark.parametrize("name", ("chain3", "grid2x2", "grid2x2_negative", "grid3x3_sparse"))
def test_several_levels(gpu_ctx, name):
    rng = np.random.default_rng(len(name))
    if name == "chain3":  # 50-wide images 28 apart: the rois are 6 apart, within the schedule's gap -> a level each
        corners, sizes = [(0, 0), (28, 2), (56, -3)], [(50, 33)] * 3
    elif name.startswith("grid2x2"):  # every pair overlaps: pairs share images across levels
        corners, sizes = [(-9, -7), (36, -6), (-8, 25), (37, 26)], [(70, 46), (69, 45), (71, 46), (68, 44)]
        if name.endswith("negative"):
            corners = [(x - 1000, y - 37) for x, y in corners]
    else:  # a 3 x 3 grid: direct and diagonal neighbours overlap
        corners = [(60 * c + int(rng.integers(-3, 4)), 40 * r + int(rng.integers(-3, 4))) for r in range(3) for c in range(3)]
        sizes = [(75, 52)] * 9
    pairs, levels = schedule(corners, sizes)
    est, _ = _check(corners, _images(rng, sizes, 4), _masks(rng, sizes))
    assert est.info["pairs"] == len(pairs) == len(Z.pairs(corners, sizes))
    assert est.info["levels"] == int(levels.max()) + 1 and est.info["levels"] > 1
    assert est.info["device_ms"] > 0.0 and est.info["device_ms_with_copy"] >= est.info["device_ms"]


def test_a_pair_without_overlap_comes_back_as_copies(gpu_ctx):
    rng = np.random.default_rng(2)
    sizes, corners = [(20, 10), (20, 10)], [(0, 0), (20, 0)]  # touching is not overlapping
    imgs, masks = _images(rng, sizes), _masks(rng, sizes)
    est, got = _check(corners, imgs, masks)
    assert est.info["pairs"] == 0 and est.info["levels"] == 0
    assert all(np.array_equal(g, m) and g is not m for g, m in zip(got, masks))
    # one image alone
    est, got = _check([(5, 5)], imgs[:1], masks[:1])
    assert np.array_equal(got[0], masks[0])


def test_residency_and_input_protection(gpu_ctx, monkeypatch):
    rng = np.random.default_rng(3)
    corners, sizes = [(0, 0), (33, 4), (10, 30)], [(60, 45), (58, 44), (62, 40)]
    imgs, masks = _images(rng, sizes, 6), _masks(rng, sizes)
    want = Z.find(imgs, corners, masks)
    _check(corners, imgs, masks)  # numpy in, numpy out
    d_imgs = [S.DeviceImage.from_numpy(a, gpu_ctx) for a in imgs]
    d_masks = [S.DeviceImage.from_numpy(m, gpu_ctx) for m in masks]
    for a, b in ((d_imgs, d_masks), (imgs, d_masks), (d_imgs, masks)):
        got = S.ColorSeamEstimator().find(a, corners, b)
        assert all(isinstance(g, S.DeviceImage) for g in got)
        assert all(np.array_equal(g.numpy(), w) for g, w in zip(got, want))
    assert all(np.array_equal(d.numpy(), m) for d, m in zip(d_masks, masks))
    assert all(np.array_equal(d.numpy(), a) for d, a in zip(d_imgs, imgs))
    # what the reference's SeamFinder.find hands a finder: float32 images
    got = S.ColorSeamEstimator().find([a.astype(np.float32) for a in imgs], corners, masks)
    assert all(isinstance(g, np.ndarray) and np.array_equal(g, w) for g, w in zip(got, want))
    # pitched views of larger device buffers (what Cropper.crop_images hands on)
    big_i = [np.full((a.shape[0] + 9, a.shape[1] + 13, 3), 200, np.uint8) for a in imgs]
    big_m = [np.full((m.shape[0] + 9, m.shape[1] + 13), 255, np.uint8) for m in masks]
    for bi, bm, a, m in zip(big_i, big_m, imgs, masks):
        bi[5:5 + a.shape[0], 7:7 + a.shape[1]] = a
        bm[5:5 + m.shape[0], 7:7 + m.shape[1]] = m
    v_i = [S.DeviceImage.from_numpy(b, gpu_ctx)[5:5 + a.shape[0], 7:7 + a.shape[1]] for b, a in zip(big_i, imgs)]
    v_m = [S.DeviceImage.from_numpy(b, gpu_ctx)[5:5 + m.shape[0], 7:7 + m.shape[1]] for b, m in zip(big_m, masks)]
    got = S.ColorSeamEstimator().find(v_i, corners, v_m)
    assert all(np.array_equal(g.numpy(), w) for g, w in zip(got, want))
    # SeamFinder keeps device images on the device for this finder
    got = S.SeamFinder("dp_color", estimator=S.ColorSeamEstimator()).find(d_imgs, corners, d_masks)
    assert all(isinstance(g, S.DeviceImage) and np.array_equal(g.numpy(), w) for g, w in zip(got, want))
    monkeypatch.setattr(config, "_device_resident", True)
    got = S.ColorSeamEstimator().find(imgs, corners, masks)
    assert all(isinstance(g, S.DeviceImage) and np.array_equal(g.numpy(), w) for g, w in zip(got, want))


def test_errors_from_the_device_entry(gpu_ctx):
    img, m = np.zeros((4, 5, 3), np.uint8), np.full((4, 5), 255, np.uint8)
    est = S.ColorSeamEstimator()
    with pytest.raises(S.StitchingError, match="image 0"):
        est.find([S.DeviceImage.from_numpy(img[:, :, 0].copy(), gpu_ctx)], [(0, 0)], [m])
    with pytest.raises(S.StitchingError, match="u8x1"):
        est.find([img], [(0, 0)], [S.DeviceImage.from_numpy(img, gpu_ctx)])


def test_limits_are_refused_and_the_context_stays_usable(gpu_ctx):
    cap, longest = S.ColorSeamEstimator.MAX_CROSS_EXTENT, S.ColorSeamEstimator.MAX_SEAM_LENGTH
    rng = np.random.default_rng(4)
    est = S.ColorSeamEstimator()
    small = ([(0, 0), (3, 0)], [(9, 5), (8, 5)])
    s_imgs, s_masks = _images(rng, small[1]), _masks(rng, small[1])
    for sizes, what in (([(cap + 1, 2)] * 2, "across"), ([(1, longest + 1)] * 2, "u32 accumulators")):
        imgs = [np.zeros((h, w, 3), np.uint8) for w, h in sizes]
        masks = [np.full((h, w), 255, np.uint8) for w, h in sizes]
        assert Z.orientation((0, 0), sizes[0], (0, 0), sizes[1]) == (True, True)
        with pytest.raises(S.StitchingError, match=what):
            est.find(imgs, [(0, 0), (0, 0)], masks)
        _check(small[0], s_imgs, s_masks, est)  # the call after it succeeds
    # at the limits themselves (two rows at the cap: the 16-columns-per-lane kernel; all costs 0 along the longest seam)
    sizes = [(cap, 2)] * 2
    _check([(0, 0), (0, 0)], _images(rng, sizes, 3), _masks(rng, sizes))
    sizes = [(1, longest)] * 2
    _check([(0, 0), (0, 0)], _images(rng, sizes), _masks(rng, sizes))


@pytest.mark.parametrize("cross", (300, 1000, 2000, 4000))
def test_every_columns_per_lane_kernel(gpu_ctx, cross):
    """2, 4, 8 and 16 columns per lane (the kernel is chosen from the level's largest cross extent), a few rows more than a walk-back step"""
    rng = np.random.default_rng(cross)
    corners, sizes = _side_by_side(cross, 70, False)
    _check(corners, _images(rng, sizes, 3), _masks(rng, sizes))


def _rig(**kw):
    frames = synthetic.make_frames(range(4), 96, 72)
    images = S.Images.of(frames, kw.get("medium_megapix", 0.6), kw.get("low_megapix", 0.1), -1)
    mw, mh = images.get_scaled_img_sizes(R.MEDIUM)[0]
    return frames, synthetic.ring_cameras(4, mw, mh, focal_factor=0.75, span_deg=110.0)


def test_composer_with_a_seam_estimator(gpu_ctx):
    """Composer(seam_estimator=) at tests/test_gpu_composer.py's scaled settings: the plan's seam masks are the contract's on the
    low-resolution warps made by hand, and run(plan) is compose() with those masks"""
    frames, cams = _rig(**SCALED)
    comp = S.Composer(ctx=gpu_ctx, seam_estimator=S.ColorSeamEstimator(), **SCALED)
    assert comp.settings["finder"] == "dp_color"
    plan = comp.prepare(frames, cams)
    S.set_device_resident(True)
    try:
        images = S.Images.of(list(frames), SCALED["medium_megapix"], SCALED["low_megapix"], -1)
        medium = list(images.resize(R.MEDIUM))
        low = list(images.resize(R.LOW, medium))
        wp = S.Warper(comp.settings["warper_type"], ctx=gpu_ctx)
        wp.set_scale(cams)
        sizes, aspect = images.get_scaled_img_sizes(R.LOW), images.get_ratio(R.MEDIUM, R.LOW)
        imgs = list(wp.warp_images(low, cams, aspect))
        masks = list(wp.create_and_warp_masks(sizes, cams, aspect))
        corners, sizes = wp.warp_rois(sizes, cams, aspect)
        cr = S.Cropper(True)
        cr.prepare(imgs, masks, corners, sizes)
        masks, imgs = list(cr.crop_images(masks)), list(cr.crop_images(imgs))
        corners, sizes = cr.crop_rois(corners, sizes)
        final = list(images.resize(R.FINAL))
    finally:
        S.set_device_resident(False)
    h_masks = [m.numpy() for m in masks]
    want = Z.find([a.numpy() for a in imgs], corners, h_masks)
    assert len(Z.pairs(corners, sizes)) >= 3 and any(not np.array_equal(w, m) for w, m in zip(want, h_masks))
    assert all(isinstance(m, S.DeviceImage) for m in plan.seam_masks)
    assert all(np.array_equal(m.numpy(), w) for m, w in zip(plan.seam_masks, want))
    pano, mask = comp.run(plan)
    st = comp.settings
    want_pano, want_mask = compose(final, cams, warper_type=st["warper_type"], blender_type=st["blender_type"],
                                   blend_strength=st["blend_strength"], compensator=plan.compensator, seam_masks=want, ctx=gpu_ctx,
                                   cropper=cr, crop_aspect=images.get_ratio(R.LOW, R.FINAL), camera_aspect=images.get_ratio(R.MEDIUM, R.FINAL))
    assert np.array_equal(mask.numpy(), want_mask.numpy()) and np.array_equal(pano.numpy(), want_pano.numpy())
    # the seams are not the geometric ones
    voronoi = S.Composer(ctx=gpu_ctx, finder="voronoi", **SCALED).prepare(frames, cams)
    assert any(not np.array_equal(a.numpy(), b.numpy()) for a, b in zip(voronoi.seam_masks, plan.seam_masks))


CHILD = r"""
import sys
sys.modules["cv2"] = None
sys.path.insert(0, sys.argv[1])
import hashlib, json
import numpy as np
import stitching_amd as S
from stitching_amd import synthetic
try:
    import cv2
    raise SystemExit("cv2 imported")
except ImportError:
    pass
frames = synthetic.make_frames(range(4), 96, 72)
cams = synthetic.ring_cameras(4, 96, 72, focal_factor=0.75, span_deg=110.0)
comp = S.Composer(seam_estimator=S.ColorSeamEstimator())
assert comp.settings == S.Composer.DEFAULT_SETTINGS
pano = comp.compose(frames, cams).numpy()
print(json.dumps({"sha": hashlib.sha256(np.ascontiguousarray(pano).tobytes()).hexdigest(), "shape": list(pano.shape),
                  "pairs": comp.seam_estimator.info["pairs"]}))
"""


def test_default_settings_without_cv2_in_a_fresh_process(gpu_ctx):
    """a child process in which `import cv2` fails composes with every default setting plus seam_estimator="""
    frames, cams = _rig()
    want = S.Composer(ctx=gpu_ctx, seam_estimator=S.ColorSeamEstimator()).compose(frames, cams).numpy()
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["shape"] == list(want.shape) and out["sha"] == hashlib.sha256(want.tobytes()).hexdigest()
    assert out["pairs"] >= 3
