"""What a blender that adopted a stx_mb_weights handle no longer sends to the device (stx_blend_host.cpp: mb_resident_table, mb_finish):
its descriptor table, when one of the handle's resident copies equals it byte for byte, and the panorama mask, which the blend that filled
the handle left there.  Every comparison is byte for byte, panorama and mask, with a blender that never saw a handle; one result is
compared with tests/numpy_blenders.py as well.  include/stitching_amd_debug.h: stx_debug_blend_uploads counts the descriptor tables the
last blend() copied, stx_debug_blend_mask_stored tells whether its level-0 launch stored the mask.

The rig is that of tests/test_gpu_cover_replay.py (1150 x 160, three 512-column tiles at level 0, a hole and a gap in the cover, 4 and 5
bands, with and without the grey edge that sends level 0 through the deferred pass).  A table holds buffer addresses; the allocator hands
out the lowest free block of a size, so blenders fed the same device images one after the other are given the same addresses."""
import ctypes as C
import gc

import numpy as np
import pytest

import stitching_amd as S
from stitching_amd import synthetic
from tests import numpy_blenders as NB

pytestmark = pytest.mark.gpu

CORNERS = [(-20, -10), (40, 10), (898, -5), (930, 50)]
SIZES = [(400, 120), (300, 80), (232, 120), (200, 100)]  # (w, h); roi (-20, -10, 1150, 160)


def pixels(seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3)).astype(np.uint8) for w, h in SIZES]


def sparse_masks(grey):
    masks = [np.full((h, w), 255, np.uint8) for w, h in SIZES]
    masks[0][:16, :256] = 0
    masks[3][-30:, :50] = 0
    if grey:
        masks[2][:, -6:] = np.linspace(230, 20, 6).astype(np.uint8)[None, :]
    return masks


def device(ctx, arrays):
    return [S.DeviceImage.from_numpy(a, ctx) for a in arrays]


def hook(ctx, name):
    n = C.c_int(-1)
    assert getattr(ctx._lib, name)(ctx.handle, C.byref(n)) == 0
    return n.value


class Result:
    def __init__(self, pano, mask, kept, adopted, ctx, raw_mask=None):
        self.pano, self.mask, self.kept, self.adopted, self.raw_mask = pano, mask, kept, adopted, raw_mask
        self.uploads = hook(ctx, "stx_debug_blend_uploads")
        self.mask_stored = hook(ctx, "stx_debug_blend_mask_stored")
        self.replayed = hook(ctx, "stx_debug_blend_replayed")

    def same(self, other):
        return np.array_equal(self.mask, other.mask) and np.array_equal(self.pano, other.pano)


def blend(ctx, bands, imgs, masks, keep=False, use=None, band=None, raw=False):
    roi = S.Blender.result_roi(CORNERS, SIZES)
    bl = S.Blender("multiband", synthetic.blend_strength_for_bands(bands, roi[2], roi[3]), ctx=ctx)
    bl.prepare(CORNERS, SIZES)
    assert bl.blender.num_bands() == bands
    for img, mask, corner in zip(imgs, masks, CORNERS):
        bl.feed(img, mask, corner)
    kept = bl.blender.keep_weights() if keep else None
    adopted = bl.blender.use_weights(use) if use is not None else False
    if band is not None:
        assert ctx._lib.stx_blend_set_band(bl.blender._h, band[0], band[1]) == 0
    pano, pmask = bl.blend()
    return Result(np.asarray(pano), np.asarray(pmask), kept, adopted, ctx, pmask if raw else None)


def numpy_blend(bands, imgs, masks):
    b = NB.NumpyMultiBand(bands)
    b.prepare(NB.result_roi(CORNERS, SIZES))
    assert b.B == bands
    for img, mask, c in zip(imgs, masks, CORNERS):
        b.feed(img.astype(np.int16), mask, c)
    res, m = b.blend()
    return np.minimum(np.abs(res.astype(np.int32)), 255).astype(np.uint8), m


@pytest.mark.parametrize("bands", [4, 5])
def test_the_table_is_uploaded_once_per_set_of_buffers(gpu_ctx, bands):
    h_masks = sparse_masks(False)
    masks = device(gpu_ctx, h_masks)
    sets = [device(gpu_ctx, pixels(seed)) for seed in range(1, 6)]  # five sets of image buffers, all alive: five sets of addresses
    plain = [blend(gpu_ctx, bands, imgs, masks) for imgs in sets]
    assert all(p.uploads == 1 and p.mask_stored == 1 for p in plain)
    a = blend(gpu_ctx, bands, sets[0], masks, keep=True)
    assert a.kept is not None and a.uploads == 1 and a.mask_stored == 1 and a.same(plain[0])
    # the same device images: one upload, then none
    b1 = blend(gpu_ctx, bands, sets[0], masks, use=a.kept)
    b2 = blend(gpu_ctx, bands, sets[0], masks, use=a.kept)
    assert b1.adopted and b2.adopted
    assert (b1.uploads, b2.uploads) == (1, 0)
    assert b1.same(plain[0]) and b2.same(plain[0])
    # two sets in turn: one more upload in all (the first set's table is resident)
    ups = []
    for k in range(6):
        r = blend(gpu_ctx, bands, sets[k % 2], masks, use=a.kept)
        ups.append(r.uploads)
        assert r.adopted and r.same(plain[k % 2]), k
    assert ups == [0, 1, 0, 0, 0, 0]
    # sets 2, 3 fill the four slots; the fifth evicts the least recently used (set 0's) — the bytes are the plain blender's throughout
    for k in (2, 3):
        r = blend(gpu_ctx, bands, sets[k], masks, use=a.kept)
        assert r.uploads == 1 and r.same(plain[k])
    r = blend(gpu_ctx, bands, sets[1], masks, use=a.kept)  # set 1 is now the most recent, set 0 the least
    assert r.uploads == 0
    r = blend(gpu_ctx, bands, sets[4], masks, use=a.kept)
    assert r.uploads == 1 and r.same(plain[4])
    for k, want in ((1, 0), (2, 0), (3, 0), (0, 1), (0, 0)):
        r = blend(gpu_ctx, bands, sets[k], masks, use=a.kept)
        assert r.uploads == want and r.same(plain[k]), (k, want)
    if bands == 4:
        pano, mask = numpy_blend(bands, pixels(1), h_masks)
        assert np.array_equal(a.mask, mask) and np.array_equal(a.pano, pano)


@pytest.mark.parametrize("bands", [4, 5])
def test_the_mask_of_an_adopter_is_the_keepers(gpu_ctx, bands):
    h_masks = sparse_masks(False)
    masks, imgs = device(gpu_ctx, h_masks), device(gpu_ctx, pixels(1))
    a = blend(gpu_ctx, bands, imgs, masks, keep=True)
    c = blend(gpu_ctx, bands, imgs, masks)
    assert a.mask_stored == 1 and c.mask_stored == 1
    b = blend(gpu_ctx, bands, imgs, masks, use=a.kept)
    assert b.adopted and b.replayed == bands - 2 and b.mask_stored == 0
    assert np.array_equal(b.mask, a.mask) and b.same(c) and a.same(c)
    assert a.mask[:16, :40].max() == 0 and a.mask[40:100, 420:890].max() == 0 and a.mask[60, 200] == 255
    other = device(gpu_ctx, pixels(2))
    r = blend(gpu_ctx, bands, other, masks, use=a.kept)
    assert r.mask_stored == 0 and r.same(blend(gpu_ctx, bands, other, masks)) and not np.array_equal(r.pano, b.pano)


def test_a_band_set_after_adoption_stores_the_mask(gpu_ctx):
    bands = 5
    masks, imgs = device(gpu_ctx, sparse_masks(False)), device(gpu_ctx, pixels(1))
    a = blend(gpu_ctx, bands, imgs, masks, keep=True)
    b = blend(gpu_ctx, bands, imgs, masks, use=a.kept, band=(0, 576))
    c = blend(gpu_ctx, bands, imgs, masks, band=(0, 576))
    assert b.adopted and b.replayed == 0 and b.mask_stored == 1 and c.mask_stored == 1
    assert b.mask.shape == (160, 576) and b.same(c) and np.array_equal(b.mask, a.mask[:, :576])
    full = blend(gpu_ctx, bands, imgs, masks, use=a.kept)
    assert full.mask_stored == 0 and full.same(a)


@pytest.mark.parametrize("bands", [4, 5])
def test_the_grey_edge_rig_takes_the_deferred_pass(gpu_ctx, bands):
    h_masks, h_imgs = sparse_masks(True), pixels(3)
    masks, imgs = device(gpu_ctx, h_masks), device(gpu_ctx, h_imgs)
    a = blend(gpu_ctx, bands, imgs, masks, keep=True)
    b = blend(gpu_ctx, bands, imgs, masks, use=a.kept)
    c = blend(gpu_ctx, bands, imgs, masks)
    assert b.adopted and b.replayed == bands - 2 and b.mask_stored == 0 and c.mask_stored == 1
    assert a.same(c) and b.same(c)
    if bands == 5:
        pano, mask = numpy_blend(bands, h_imgs, h_masks)
        assert np.array_equal(b.mask, mask) and np.array_equal(b.pano, pano)


def test_the_mask_outlives_handle_and_blenders(gpu_ctx):
    bands = 4
    masks, imgs = device(gpu_ctx, sparse_masks(False)), device(gpu_ctx, pixels(1))
    a = blend(gpu_ctx, bands, imgs, masks, keep=True)
    b = blend(gpu_ctx, bands, imgs, masks, use=a.kept, raw=True)
    assert b.mask_stored == 0
    want = a.mask.copy()
    a.kept.free()
    a.kept = None
    gc.collect()
    # blenders that take the blocks the handle gave back: the shared mask is none of them
    for seed in (4, 5):
        blend(gpu_ctx, bands, device(gpu_ctx, pixels(seed)), masks)
    assert np.array_equal(np.asarray(b.raw_mask), want)
