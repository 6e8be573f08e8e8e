"""Scenes for the packed pyrUp of the gathers (up_patch_pk_math / up_patch_pks_math of csrc/stx_blend_fast.hip) and for the level-0
gather's store of tiles that no image covers.  Pure numpy; tests/test_pyrup_rows_first.py asserts the facts without a GPU,
tests/test_gpu_pyrup_rows_first.py runs the scenes on the device.  Built on tests/constructed_multiband.Scene.

What a scene can and cannot reach.  A feed rectangle starts on a multiple of 2^B >= 8 columns and is a multiple of 2^B wide and high, and
the packed gathers run on the levels <= B - 3: the coarse plane under a packed pyrUp is at least 4 rows high and even, so the row rule for
coarse heights 1, 2 and odd ones is the CPU test's (as is a tap at +-500, profiles/constructed_multiband.md); here a wavefront meets the
rule at its first and last coarse row.  For the same reason it is the IMAGE, not its feed rectangle, that can start and end inside a
lane's 8 pixels (`tiny`).  Two neighbouring samples of G_1 share three of their five taps and cannot be 0 and 255; stripes 12 pixels
wide put both values into one 6-sample window."""
import numpy as np

from tests import constructed_multiband as CM

EDGE_SIZES = {3: (72, 40), 4: (80, 48)}   # (width, height) per band count: level 0 alone, and level 1 through mb_level_pk_kernel
HOLE_W = 600                              # two tile columns of 512: the last one 88 columns wide
HOLE_H = {3: 40, 4: 48}
TINY = (5, 3, 26, 7)                      # (width, height, x, y): columns 26 .. 30 lie inside the lane from 24


def stripes(h, w, seed):
    """plane 0: columns of 0 / 255 in stripes 12 wide; plane 1: rows in stripes 6 high; plane 2: 4 x 4 blocks of 0 / 255 by a seeded draw"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    blocks = rng.choice(np.array([0, 255]), ((h + 3) // 4, (w + 3) // 4)).repeat(4, 0).repeat(4, 1)[:h, :w]
    return np.stack([255 * ((xx // 12) & 1), 255 * ((yy // 6) & 1), blocks], 2).astype(np.uint8)


def edges(bands):
    """Three images: a backdrop of the panorama's size (its first lane is the left edge of its feed rectangle and of the panorama, its last
    the right edge), a second at an odd corner with a notch in its mask, and `tiny`, 5 x 3 pixels inside one lane: one, two and three
    covering images"""
    w, h = EDGE_SIZES[bands]
    m1 = CM._full(h - 9, w - 21)
    m1[:4, :7] = 0
    tw, th, tx, ty = TINY
    feeds = [(stripes(h, w, 1), CM._full(h, w), (0, 0)), (255 - stripes(h - 9, w - 21, 2), m1, (13, 5)),
             (CM._noise(3, th, tw), CM._full(th, tw), (tx, ty))]
    return CM.Scene(bands, feeds, {"covering": {1, 2, 3}, "tiny_lane": tx // 8})


def holes(bands, grey=False):
    """Two tile columns.  Rows 0 .. 9: two overlapping images in tile column 0, nothing in the last column; rows 10 .. 19: nothing at all;
    rows 20 .. : an image in the last tile column, nothing in column 0.  grey: one grey mask byte (the deferring instantiation)"""
    h = HOLE_H[bands]
    m0 = CM._full(10, 300)
    if grey:
        m0[3, 17] = 127
    feeds = [(stripes(10, 300, 4), m0, (0, 0)), (255 - stripes(8, 100, 5), CM._full(8, 100), (250, 2)),
             (stripes(h - 20, 40, 6), CM._full(h - 20, 40), (560, 20))]
    return CM.Scene(bands, feeds, {"uncovered": {"last column": (0, 10), "both": (10, 20), "column 0": (20, h)}, "grey": grey})


def coverage(scene):
    """number of images whose mask covers each pixel of the roi"""
    x0, y0, w, h = scene.roi
    cnt = np.zeros((h, w), np.int64)
    for _, m, (cx, cy) in scene.feeds:
        cnt[cy - y0:cy - y0 + m.shape[0], cx - x0:cx - x0 + m.shape[1]] += m != 0
    return cnt


def uncovered_tiles(scene):
    """[(tile column, first row)] of the 512 x 2 tiles that no image's rectangle touches (mb_tile_hit's rectangle test at level 0)"""
    x0, y0, w, h = scene.roi
    out = []
    for ty in range(0, h, CM.TILE_H):
        for tx in range(0, w, CM.TILE_W):
            hit = any(cx - x0 < tx + CM.TILE_W and cx - x0 + m.shape[1] > tx and cy - y0 < ty + CM.TILE_H and cy - y0 + m.shape[0] > ty
                      for _, m, (cx, cy) in scene.feeds)
            if not hit:
                out.append((tx // CM.TILE_W, ty))
    return out
