"""Composer without a GPU: the keyword rules of the reference's Stitcher, what a plan refuses, and the clipping of the cropper's
rectangles (pipeline.clip_rectangle) against the numpy slice Cropper.crop_rectangle takes."""
import numpy as np
import pytest

import stitching_amd as S
from stitching_amd.pipeline import ComposePlan, Composer, clip_rectangle, _split_cropper


def test_keywords_are_the_reference_stitchers():
    c = Composer()
    assert c.settings == {"medium_megapix": 0.6, "warper_type": "spherical", "low_megapix": 0.1, "crop": True, "compensator": "gain_blocks",
                          "nr_feeds": 1, "block_size": 32, "finder": "dp_color", "final_megapix": -1, "blender_type": "multiband",
                          "blend_strength": 5}
    c = Composer(warper_type="plane", blender_type="feather", blend_strength=7, crop=False, compensator="no", finder="voronoi", nr_feeds=2,
                 block_size=16, medium_megapix=0.5, low_megapix=0.05, final_megapix=2, ctx=None)
    assert c.settings["finder"] == "voronoi" and c.settings["block_size"] == 16 and c.settings["crop"] is False
    for bad in ("cropp", "detector", "Finder"):
        with pytest.raises(S.StitchingError, match="^Invalid Argument: " + bad + "$"):
            Composer(**{bad: 1})
    assert S.Composer is Composer and "Composer" in S.__all__


@pytest.mark.parametrize("kw", [{"finder": "watershed"}, {"compensator": "gamma"}, {"warper_type": "cube"}, {"blender_type": "poisson"},
                                {"medium_megapix": 0.05, "low_megapix": 0.1}])
def test_unknown_choices_fail_at_construction(kw):
    with pytest.raises(S.StitchingError):
        Composer(**kw)


def test_unknown_finder_message():
    with pytest.raises(S.StitchingError, match="unknown seam finder 'watershed'"):
        Composer(finder="watershed")


def test_plan_refuses_frames_of_other_sizes():
    frames = [np.zeros((30, 40, 3), np.uint8), np.zeros((30, 40, 3), np.uint8)]
    images = S.Images.of(frames)
    plan = ComposePlan(images, frames, [None, None], 1.0, S.Cropper(False), None, [], None, [], [])
    assert plan.frame_sizes == [(40, 30), (40, 30)] and plan.lir_aspect == 1.0 and plan.camera_aspect == 1.0
    plan.check_frames([np.zeros((30, 40, 3), np.uint8)] * 2)
    for other in ([np.zeros((30, 41, 3), np.uint8)] * 2, [frames[0]], frames + frames[:1], [frames[0], np.zeros((40, 30, 3), np.uint8)]):
        with pytest.raises(S.StitchingError, match="same rig, same sizes"):
            Composer(finder="voronoi").run(plan, images=other)


def test_cropper_argument_forms():
    ready = S.Cropper()
    ready.intersection_rectangles = [S.Rectangle(0, 0, 2, 2)]
    assert _split_cropper(None, 1) == (None, 1)
    assert _split_cropper(S.Cropper(False), 3.0) == (None, 3.0)
    assert _split_cropper((ready, 2.5), 1) == (ready, 2.5) and _split_cropper(ready, 2.0) == (ready, 2.0)
    with pytest.raises(S.StitchingError, match="not prepared"):
        _split_cropper(S.Cropper(), 1)


def test_clipping_is_numpys_slice_on_200_rectangles():
    rng = np.random.default_rng(2026)
    seen_clipped = seen_empty = 0
    for k in range(200):
        w, h = (int(v) for v in rng.integers(1, 40, 2))
        img = np.arange(w * h, dtype=np.int64).reshape(h, w)
        r = S.Rectangle(int(rng.integers(0, w + 6)), int(rng.integers(0, h + 6)), int(rng.integers(0, w + 8)), int(rng.integers(0, h + 8)))
        if k % 7 == 0:  # a non-integer aspect, as lir_aspect is
            r = r.times(float(rng.uniform(0.3, 2.7)))
        want = S.Cropper.crop_rectangle(img, r)
        x0, x1, y0, y1 = clip_rectangle(r, w, h)
        assert (y1 - y0, x1 - x0) == want.shape or want.size == 0 and (y1 - y0) * (x1 - x0) == 0, (r, w, h)
        assert 0 <= x0 <= x1 <= w and 0 <= y0 <= y1 <= h
        if want.size:
            assert np.array_equal(img[y0:y1, x0:x1], want) and want[0, 0] == y0 * w + x0
            seen_clipped += (x1 - x0, y1 - y0) != (r.width, r.height)
        else:
            seen_empty += 1
    assert seen_clipped >= 20 and seen_empty >= 5  # both kinds occur
