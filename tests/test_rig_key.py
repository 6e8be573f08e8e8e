"""The key a StitchJob keeps its rig geometry under (stitching_amd/pipeline.py: rig_key) and the condition of reuse
(masks_belong_to_job): host logic, no device."""
import numpy as np

from stitching_amd.cropper import Rectangle
from stitching_amd.pipeline import masks_belong_to_job, rig_key


class _Cropper:
    def __init__(self, rects):
        self.intersection_rectangles = rects


BASE = dict(cam_bytes=b"\x01\x02", camera_aspect=1, warper_type="spherical", scale=480.0, sizes=[(640, 480)] * 3, blender_type="multiband",
            num_bands=None, blend_strength=5, modes=("exact", "q15", "scalar", 4), cropper=None, crop_aspect=1)


def key(**kw):
    return rig_key(**dict(BASE, **kw))


def test_equal_inputs_give_equal_hashable_keys():
    a, b = key(), key(sizes=[[640, 480]] * 3, scale=np.float64(480.0), blend_strength=5.0)
    assert a == b and hash(a) == hash(b)


def test_every_component_changes_the_key():
    changed = [dict(cam_bytes=b"\x01\x03"), dict(camera_aspect=0.5), dict(warper_type="plane"), dict(scale=481.0), dict(sizes=[(640, 480)] * 4),
               dict(sizes=[(640, 481)] * 3), dict(blender_type="feather"), dict(blend_strength=6), dict(num_bands=3),
               dict(modes=("glibc", "q15", "scalar", 4)), dict(modes=("exact", "float", "scalar", 4)), dict(modes=("exact", "q15", "simd-hv", 8)),
               dict(modes=("exact", "q15", "simd-hv", 4)), dict(cropper=_Cropper([Rectangle(0, 0, 5, 5)] * 3)), dict(scale=None)]
    keys = [key(**c) for c in changed]
    assert all(k != key() for k in keys)
    assert len(set(keys)) == len(keys)


def test_blend_strength_counts_only_without_num_bands():
    # with num_bands the job derives blend_strength from the ROIs in its first run: the derived value must not end the reuse
    assert key(num_bands=3, blend_strength=5) == key(num_bands=3, blend_strength=1.234)
    assert key(num_bands=3) != key(num_bands=4)


def test_cropper_rectangles_and_aspect():
    r = [Rectangle(1, 2, 30, 40), Rectangle(0, 0, 31, 40), Rectangle(2, 2, 30, 39)]
    assert key(cropper=_Cropper(r), crop_aspect=2.0) == key(cropper=_Cropper([tuple(x) for x in r]), crop_aspect=np.float64(2.0))
    assert key(cropper=_Cropper(r), crop_aspect=2.0) != key(cropper=_Cropper(r), crop_aspect=2.5)
    r2 = [r[0], r[1], Rectangle(2, 2, 30, 38)]
    assert key(cropper=_Cropper(r), crop_aspect=2.0) != key(cropper=_Cropper(r2), crop_aspect=2.0)
    assert key(crop_aspect=2.0) == key(crop_aspect=3.0)  # no cropper: the aspect means nothing


def test_masks_belong_to_the_job_when_absent_or_host_arrays():
    host = [np.zeros((4, 4), np.uint8)] * 2
    device = [object(), np.zeros((4, 4), np.uint8)]  # anything that is no numpy array: the caller's buffer
    assert masks_belong_to_job(None, None)
    assert masks_belong_to_job(host, None) and masks_belong_to_job(None, host)
    assert not masks_belong_to_job(device, None) and not masks_belong_to_job(None, device)
    assert not masks_belong_to_job(device, host)  # feed_masks are the ones that are fed
