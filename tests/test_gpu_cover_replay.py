"""The image search of the packed multi-band gathers, recorded once per rig and replayed (stx_blend_fast.hip: mb_cover_kernel, the REPLAY
instantiations of mb_level0_pk_kernel / mb_level_pk_kernel; the table rides in the stx_mb_weights handle of stx_blend_keep_weights /
stx_blend_use_weights).  A replaying gather walks the same images in the same order as a searching one, so every comparison here is byte
for byte, panorama and mask, between three blenders on the same feeds: A keeps (and records the cover), B adopts and replays, C never
sees a handle.  One of them is compared with tests/numpy_blenders.py as well.  include/stitching_amd_debug.h: stx_debug_blend_replayed
tells how many gather launches of the last blend() replayed.

Shapes: a panorama of 1150 x 160 (padded 1152 x 160) has three 512-column tiles at level 0 and two at level 1, 80 / 40 tile rows = ten / five
XCD bands of four; 4 bands put level 1 through mb_level_pk_kernel, 5 bands levels 1 and 2.  The rig: corners of both signs, image 1 wholly
inside image 0's rectangle, 518 columns between image 0 and image 2 under no image (cover words 0), and a zeroed 256 x 16 corner in the
mask of image 0 — occupancy entries 0 where the rectangle test still hits."""
import ctypes as C

import numpy as np
import pytest

import stitching_amd as S
from stitching_amd import synthetic
from tests import numpy_blenders as NB

pytestmark = pytest.mark.gpu

CORNERS = [(-20, -10), (40, 10), (898, -5), (930, 50)]
SIZES = [(400, 120), (300, 80), (232, 120), (200, 100)]  # (w, h); roi (-20, -10, 1150, 160)
_cache = {}


def pixels(seed, sizes):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3)).astype(np.uint8) for w, h in sizes]


def sparse_masks(grey):
    masks = [np.full((h, w), 255, np.uint8) for w, h in SIZES]
    masks[0][:16, :256] = 0
    masks[3][-30:, :50] = 0
    if grey:  # along one edge: what a resized seam mask leaves (the DEFER instantiation of the level-0 gather)
        masks[2][:, -6:] = np.linspace(230, 20, 6).astype(np.uint8)[None, :]
    return masks


def device(ctx, arrays):
    return [S.DeviceImage.from_numpy(a, ctx) for a in arrays]


def replayed(ctx):
    n = C.c_int(-1)
    assert ctx._lib.stx_debug_blend_replayed(ctx.handle, C.byref(n)) == 0
    return n.value


def blend(ctx, bands, corners, sizes, imgs, masks, keep=False, use=None, band=None):
    """-> (panorama, mask, kept weights or None, adopted, gather launches that replayed)"""
    roi = S.Blender.result_roi(corners, sizes)
    bl = S.Blender("multiband", synthetic.blend_strength_for_bands(bands, roi[2], roi[3]), ctx=ctx)
    bl.prepare(corners, sizes)
    assert bl.blender.num_bands() == bands
    for img, mask, corner in zip(imgs, masks, corners):
        bl.feed(img, mask, corner)
    kept = bl.blender.keep_weights() if keep else None
    adopted = bl.blender.use_weights(use) if use is not None else False
    if band is not None:
        assert ctx._lib.stx_blend_set_band(bl.blender._h, band[0], band[1]) == 0
    pano, pmask = bl.blend()
    return np.asarray(pano), np.asarray(pmask), kept, adopted, replayed(ctx)


def same(a, b):
    return np.array_equal(a[1], b[1]) and np.array_equal(a[0], b[0])


def numpy_blend(bands, corners, imgs, masks, key):
    """tests/numpy_blenders.py on the same feeds, made once per key"""
    if key not in _cache:
        sizes = [(m.shape[1], m.shape[0]) for m in masks]
        b = NB.NumpyMultiBand(bands)
        b.prepare(NB.result_roi(corners, sizes))
        assert b.B == bands
        for img, mask, c in zip(imgs, masks, corners):
            b.feed(img.astype(np.int16), mask, c)
        res, m = b.blend()
        _cache[key] = (np.minimum(np.abs(res.astype(np.int32)), 255).astype(np.uint8), m)
    return _cache[key]


@pytest.mark.parametrize("bands,grey", [(4, False), (5, False), (5, True)])
def test_sparse_cover_replays_byte_for_byte(gpu_ctx, bands, grey):
    """keeper, replayer and a blender without a handle on the sparse rig; then three replays in a row on new pixels: the cover is
    read-only"""
    h_masks, h_imgs = sparse_masks(grey), pixels(1, SIZES)
    masks, imgs = device(gpu_ctx, h_masks), device(gpu_ctx, h_imgs)
    a = blend(gpu_ctx, bands, CORNERS, SIZES, imgs, masks, keep=True)
    assert a[2] is not None and a[4] == 0
    b = blend(gpu_ctx, bands, CORNERS, SIZES, imgs, masks, use=a[2])
    c = blend(gpu_ctx, bands, CORNERS, SIZES, imgs, masks)
    assert b[3] is True and b[4] == bands - 2, "levels 0 .. bands - 3 replay"
    assert c[4] == 0
    assert same(a, b) and same(b, c)
    assert same(b, numpy_blend(bands, CORNERS, h_imgs, h_masks, ("sparse", bands, grey)))
    assert a[1][:16, :40].max() == 0 and a[1][40:100, 420:890].max() == 0 and a[1][60, 200] == 255  # the hole and the gap are there
    for seed in (2, 3, 4):
        other = device(gpu_ctx, pixels(seed, SIZES))
        r = blend(gpu_ctx, bands, CORNERS, SIZES, other, masks, use=a[2])
        assert r[3] is True and r[4] == bands - 2
        assert same(r, blend(gpu_ctx, bands, CORNERS, SIZES, other, masks)), f"replay with pixels {seed}"
        assert not np.array_equal(r[0], b[0])
    assert same(blend(gpu_ctx, bands, CORNERS, SIZES, imgs, masks, use=a[2]), c)


@pytest.mark.parametrize("n", [64, 65])
def test_one_word_holds_64_images(gpu_ctx, n):
    """64 images of 32 x 32 over 640 x 96 replay with every bit of the word in use; 65 keep no cover and still adopt"""
    bands = 3
    corners = [(32 * (k % 20), 32 * (k // 20)) for k in range(60)] + [(16 + 140 * k, 16 + 10 * k) for k in range(n - 60)]
    sizes = [(32, 32)] * n
    assert S.Blender.result_roi(corners, sizes) == (0, 0, 640, 96)
    h_imgs, h_masks = pixels(5, sizes), [np.full((32, 32), 255, np.uint8) for _ in range(n)]
    imgs, masks = device(gpu_ctx, h_imgs), device(gpu_ctx, h_masks)
    a = blend(gpu_ctx, bands, corners, sizes, imgs, masks, keep=True)
    b = blend(gpu_ctx, bands, corners, sizes, imgs, masks, use=a[2])
    c = blend(gpu_ctx, bands, corners, sizes, imgs, masks)
    assert a[2] is not None and b[3] is True
    assert b[4] == (bands - 2 if n == 64 else 0) and a[4] == 0 and c[4] == 0
    assert same(a, b) and same(b, c)
    assert same(b, numpy_blend(bands, corners, h_imgs, h_masks, ("tiles", n)))


def test_a_band_set_after_adoption_searches(gpu_ctx):
    """the cover answers for the region it was recorded over: a narrower band after adoption means no replay, and the bytes of a
    blender of that band that never saw a handle"""
    bands = 5
    h_masks, h_imgs = sparse_masks(False), pixels(1, SIZES)
    masks, imgs = device(gpu_ctx, h_masks), device(gpu_ctx, h_imgs)
    a = blend(gpu_ctx, bands, CORNERS, SIZES, imgs, masks, keep=True)
    b = blend(gpu_ctx, bands, CORNERS, SIZES, imgs, masks, use=a[2], band=(0, 576))
    c = blend(gpu_ctx, bands, CORNERS, SIZES, imgs, masks, band=(0, 576))
    assert b[3] is True and b[4] == 0 and c[4] == 0
    assert b[0].shape == (160, 576, 3) and same(b, c)
    assert np.array_equal(b[0], a[0][:, :576]) and np.array_equal(b[1], a[1][:, :576])
    full = blend(gpu_ctx, bands, CORNERS, SIZES, imgs, masks, use=a[2])  # the handle itself is as good as before
    assert full[4] == bands - 2 and same(full, a)
    assert same(a, numpy_blend(bands, CORNERS, h_imgs, h_masks, ("sparse", bands, False)))
