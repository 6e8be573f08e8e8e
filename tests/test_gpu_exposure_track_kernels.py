"""The three kernels of exposure tracking (csrc/stx_exposure_track.hip) on constructed rectangles, masks and images
(tests/constructed_exposure_tracks.py): statistics and self counts equal the contract (tests/numpy_exposure_track.py) integer for
integer, the scaled gain maps equal it byte for byte.  Every test asserts that its input reaches the path it names."""
import ctypes as C

import numpy as np
import pytest

import stitching_amd as S
from stitching_amd import _lib
from stitching_amd.exposure_tracking import TrackHandle, scale_gain_maps
from tests import constructed_exposure_tracks as CT
from tests import numpy_exposure_track as NT

pytestmark = pytest.mark.gpu


def measured(gpu_ctx, c, masks=None, imgs=None):
    """-> (pairs, self counts, stats, info) of the device for a constructed case"""
    h = TrackHandle(c["rects"], c["masks"] if masks is None else masks, c["stride"], gpu_ctx)
    try:
        h.measure(c["imgs"] if imgs is None else imgs)
        stats = h.collect()
        return h.pairs, h.self_counts, stats, h.info()
    finally:
        h.free()


def check(gpu_ctx, name, **kw):
    c = CT.CASES[name]()
    pairs, self_counts, stats = CT.expected(c)
    got = measured(gpu_ctx, c, **kw)
    assert got[0].tolist() == pairs.tolist()
    assert got[1].dtype == np.int64 and np.array_equal(got[1], self_counts)
    assert got[2].dtype == np.int64 and got[2].shape == stats.shape and np.array_equal(got[2], stats), (got[2], stats)
    return c, stats, got[3]


def test_one_image_has_no_pair(gpu_ctx):
    c, stats, info = check(gpu_ctx, "single")
    assert stats.shape == (0, 8) and info["pairs"] == 0 and info["tile_jobs"] == 0 and info["grid_bytes"] > 0


def test_rectangles_that_do_not_intersect(gpu_ctx):
    c, stats, info = check(gpu_ctx, "apart")
    assert stats.shape == (0, 8) and info["pairs"] == 0


def test_a_strip_narrower_than_the_stride_is_a_pair_without_samples(gpu_ctx):
    c, stats, info = check(gpu_ctx, "thin_strip")
    assert stats.shape == (1, 8) and not stats.any() and info["pairs"] == 1 and info["tile_jobs"] == 0


@pytest.mark.parametrize("name", ["negative_s3", "negative_s8"])
def test_negative_corners(gpu_ctx, name):
    c, stats, info = check(gpu_ctx, name)
    assert all(r[0] < 0 and r[1] < 0 and r[0] % c["stride"] and r[1] % c["stride"] for r in c["rects"])
    assert stats[0, 0] > 0 and info["tile_jobs"] == 1


def test_stride_one_tiles_add_into_one_pair(gpu_ctx):
    c, stats, info = check(gpu_ctx, "s1_tiles")
    assert stats[0, 0] == 150 * 40 and info["tile_jobs"] == 5 * 2 and 150 % 32 and 40 % 32   # ragged last tiles both ways


def test_zero_and_grey_mask_regions(gpu_ctx):
    c, stats, _ = check(gpu_ctx, "grey_mask")
    assert any((m == 128).any() and (m == 0).any() for m in c["masks"])
    full = CT.expected(dict(c, masks=[np.full_like(m, 255) for m in c["masks"]]))[2]
    assert 0 < stats[0, 0] < full[0, 0] and stats[0, 7] == 0


def test_saturated_pixels_in_one_image_only(gpu_ctx):
    c, stats, _ = check(gpu_ctx, "saturated_first")
    assert (c["imgs"][0] == 0).any() and (c["imgs"][0] == 255).any() and c["imgs"][1].min() >= 1 and c["imgs"][1].max() <= 254
    assert stats[0, 7] > 0 and stats[0, 0] > 0


def test_three_mutually_overlapping_images(gpu_ctx):
    c, stats, info = check(gpu_ctx, "three")
    assert stats.shape == (3, 8) and (stats[:, 0] > 0).all() and info["pairs"] == 3


def test_an_empty_pair_next_to_a_full_one(gpu_ctx):
    c, stats, _ = check(gpu_ctx, "empty_next_to_full")
    assert stats[0, 0] > 0 and not stats[1:].any()


def test_views_of_wider_parents(gpu_ctx):
    c = CT.CASES["three"]()
    rng = np.random.default_rng(77)
    masks, imgs = [], []
    for i, (m, im) in enumerate(zip(c["masks"], c["imgs"])):
        h, w = m.shape
        pm = rng.integers(0, 256, (h + 5, w + 9 + i), dtype=np.uint8)   # whatever surrounds the view must not be read as the view
        pi = rng.integers(0, 256, (h + 5, w + 9 + i, 3), dtype=np.uint8)
        pm[2:2 + h, 3 + i:3 + i + w], pi[2:2 + h, 3 + i:3 + i + w] = m, im
        dm, di = S.as_device(pm, gpu_ctx)[2:2 + h, 3 + i:3 + i + w], S.as_device(pi, gpu_ctx)[2:2 + h, 3 + i:3 + i + w]
        assert dm.stride_bytes != w and di.stride_bytes != 3 * w
        masks.append(dm)
        imgs.append(di)
    check(gpu_ctx, "three", masks=masks, imgs=imgs)


def test_two_measures_in_a_row_take_alternating_slots(gpu_ctx):
    c = CT.CASES["three"]()
    other = [np.random.default_rng(5 + i).integers(0, 256, im.shape, dtype=np.uint8) for i, im in enumerate(c["imgs"])]
    first, second = CT.expected(c)[2], CT.expected(c, imgs=other)[2]
    assert not np.array_equal(first, second) and second[:, 7].all()
    h = TrackHandle(c["rects"], c["masks"], c["stride"], gpu_ctx)
    try:
        with pytest.raises(S.StitchingError, match="pending"):
            h.collect()
        h.measure(c["imgs"])
        h.measure(other)
        with pytest.raises(S.StitchingError, match="pending"):   # both slots hold a measure nobody collected
            h.measure(other)
        assert np.array_equal(h.collect(), first)     # the oldest first
        assert np.array_equal(h.collect(), second)
        with pytest.raises(S.StitchingError, match="pending"):
            h.collect()
        h.measure(c["imgs"])                          # slot 0 again: cleared, not added to
        assert np.array_equal(h.collect(), first) and h.info()["measures"] == 3
    finally:
        h.free()


@pytest.mark.parametrize("planes", [1, 3])
@pytest.mark.parametrize("channels", [1, 3])
def test_scaled_gain_maps_equal_the_contract(gpu_ctx, planes, channels):
    rng = np.random.default_rng(10 * planes + channels)
    shapes = [(3, 5), (1, 1), (7, 2)]
    maps = [rng.uniform(0.5, 2.0, s + ((3,) if channels == 3 else ())).astype(np.float32) for s in shapes]
    r = rng.uniform(0.3, 3.0, (len(maps), planes))
    tracker_kind = "channel" if planes == 3 else "gain"
    plan_kind = "channel_blocks" if channels == 3 else "gain_blocks"
    want = NT.effective_gains(plan_kind, maps, r, tracker_kind)
    # a map given as a view of a wider parent, too
    parent = np.zeros((9, 11) + ((3,) if channels == 3 else ()), np.float32)
    parent[1:8, 4:6] = maps[2]
    dev = [S.as_device(maps[0], gpu_ctx), S.as_device(maps[1], gpu_ctx), S.as_device(parent, gpu_ctx)[1:8, 4:6]]
    got = scale_gain_maps(dev, r, gpu_ctx)
    for g, w in zip(got, want):
        g = g.numpy()
        assert g.dtype == np.float32 and g.shape == w.shape and g.tobytes() == w.tobytes()
    assert want[0].ndim == (3 if max(planes, channels) == 3 else 2)


# ---- refusals: before anything is launched, and the context stays usable --------------------------------------------------------------
def raw_create(ctx, rects, masks, stride, n=None):
    r = np.ascontiguousarray(rects, np.int32).reshape(-1)
    hs = (C.c_void_p * max(1, len(masks)))(*[getattr(m, "_h", m) for m in masks])
    out = C.c_void_p()
    rc = ctx._lib.stx_exposure_track_create(ctx.handle, len(masks) if n is None else n, r.ctypes.data_as(C.POINTER(C.c_int)), hs, stride,
                                            C.byref(out))
    return rc, out


def test_refusals_leave_the_context_usable(gpu_ctx):
    L = gpu_ctx._lib
    c = CT.CASES["three"]()
    rects = c["rects"]
    dm = [S.as_device(m, gpu_ctx) for m in c["masks"]]
    di = [S.as_device(i, gpu_ctx) for i in c["imgs"]]
    other = S.Context(gpu_ctx.device)
    try:
        foreign_mask, foreign_img = S.as_device(c["masks"][0], other), S.as_device(c["imgs"][0], other)
        bad_creates = {
            "stride 0": (rects, dm, 0, None), "stride 65": (rects, dm, 65, None), "n = 0": (rects, dm, 2, 0), "n = 1025": (rects, dm, 2, 1025),
            "null mask": (rects, [dm[0], None, dm[2]], 2, None),
            "mask of another context": (rects, [foreign_mask, dm[1], dm[2]], 2, None),
            "mask of another size": (rects, [dm[0][:, 1:], dm[1], dm[2]], 2, None),
            "mask with three channels": (rects, [di[0], dm[1], dm[2]], 2, None),
            "f32 mask": (rects, [S.as_device(np.zeros(c["masks"][0].shape, np.float32), gpu_ctx), dm[1], dm[2]], 2, None),
            # twelve times the same 1024 x 1024 rectangle at stride 1: 66 pairs of 32 x 32 tiles each, 67 584 > 65 536
            "too many tile jobs": ([(0, 0, 1024, 1024)] * 12, [S.as_device(np.zeros((1024, 1024), np.uint8), gpu_ctx)] * 12, 1, None),
        }
        for what, (r, m, s, n) in bad_creates.items():
            rc, out = raw_create(gpu_ctx, r, m, s, n)
            assert rc == -1 and not out.value, what
            assert L.stx_last_error(), what
        assert L.stx_exposure_track_create(None, 3, None, None, 2, None) == -1
        h = TrackHandle(rects, dm, 2, gpu_ctx)
        try:
            def measure(imgs):
                return L.stx_exposure_track_measure(h._h, (C.c_void_p * 3)(*[getattr(i, "_h", i) for i in imgs]))

            assert measure([di[0], None, di[2]]) == -1
            assert measure([foreign_img, di[1], di[2]]) == -1
            assert measure([di[0][1:, :], di[1], di[2]]) == -1
            assert measure([dm[0], di[1], di[2]]) == -1   # u8x1 where u8x3 belongs
            assert L.stx_exposure_track_measure(None, None) == -1 and L.stx_exposure_track_measure(h._h, None) == -1
            assert L.stx_exposure_track_collect(None, None) == -1 and L.stx_exposure_track_collect(h._h, None) == -1   # nothing pending
            assert L.stx_exposure_track_pairs(None, None, None, None) == -1 and L.stx_exposure_track_info(None, None) == -1
            assert h.info()["measures"] == 0   # none of the refused calls was queued
            h.measure(di)
            assert np.array_equal(h.collect(), CT.expected(c)[2])   # handle and context are as usable as before
        finally:
            h.free()
        assert L.stx_exposure_track_free(None) == 0
        # the scaling entry point
        maps = [S.as_device(np.ones((2, 2), np.float32), gpu_ctx)]
        f = np.ones(3, np.float32).ctypes.data_as(C.POINTER(C.c_float))
        outs = (C.c_void_p * 1)()

        def scale(ctx_h, n, ms, fp, planes):
            return L.stx_gain_maps_scale(ctx_h, n, (C.c_void_p * 1)(*[getattr(m, "_h", m) for m in ms]), fp, planes, outs)

        assert scale(None, 1, maps, f, 1) == -1 and scale(gpu_ctx.handle, 0, maps, f, 1) == -1 and scale(gpu_ctx.handle, 1, maps, f, 2) == -1
        assert scale(gpu_ctx.handle, 1, [None], f, 1) == -1 and scale(gpu_ctx.handle, 1, maps, None, 1) == -1
        assert scale(gpu_ctx.handle, 1, [dm[0]], f, 1) == -1   # u8 where f32 belongs
        assert scale(gpu_ctx.handle, 1, [S.as_device(np.ones((2, 2), np.float32), other)], f, 1) == -1
        assert not outs[0]
        assert np.array_equal(scale_gain_maps(maps, [[2.0]], gpu_ctx)[0].numpy(), np.full((2, 2), 2.0, np.float32))
    finally:
        gpu_ctx.sync()
        other.close()
