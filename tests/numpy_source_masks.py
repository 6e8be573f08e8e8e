"""The contract of source validity masks, in numpy, on top of tests/numpy_warper.py: the warped mask of a frame
that carries a mask M is remapNearest(M, xmap, ymap) with a constant 0 border over the maps of the frame's rectangle, and the masks of
the lower resolutions are a conservative shrink.  TEST INFRASTRUCTURE: no product code, no GPU.

`remap_nearest_variant` holds the one-mistake versions of the nearest sample that tests/test_source_masks_contract.py tells from the
contract: each is what a kernel would compute after one plausible slip."""
import numpy as np

from tests import numpy_warper as NW

F = np.float32


def warp_source_mask(kind, scale, K, R, mask, rect):
    """the warped mask of rectangle `rect` (x, y, w, h in warp coordinates) of a frame whose validity mask is `mask`"""
    return NW.remap_nearest_constant(np.asarray(mask), *NW.map_backward(kind, scale, K, R, rect))


VARIANTS = ("floor", "ties_half_up", "index_from_s", "interior_255", "border_replicated", "xy_swapped", "pitch_is_width")


def remap_nearest_variant(mask, xmap, ymap, variant, wide=None, x_off=0):
    """The nearest sample with ONE mistake.  `mask` is the frame's mask; for "pitch_is_width" it is the slice wide[:, x_off:x_off + W]
    of the wider array `wide`, and the mistake addresses the slice's memory with its width instead of its pitch."""
    mask = np.asarray(mask)
    H, W = mask.shape
    x64, y64 = np.asarray(xmap, np.float32).astype(np.float64), np.asarray(ymap, np.float32).astype(np.float64)
    ix, iy = NW._sat16(NW._cv_round(xmap)), NW._sat16(NW._cv_round(ymap))
    inside = (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)   # the inside test is the contract's in every variant but the two below
    with np.errstate(invalid="ignore", over="ignore"):
        if variant == "floor":
            ix, iy = np.floor(x64).astype(np.int64), np.floor(y64).astype(np.int64)
            inside = (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)
        elif variant == "ties_half_up":
            ix, iy = np.floor(x64 + 0.5).astype(np.int64), np.floor(y64 + 0.5).astype(np.int64)
            inside = (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)
        elif variant == "index_from_s":   # the index read off the 1/32 pattern s = cvRound(32 v) of the image samples
            sx, sy = NW._cv_round(np.asarray(xmap, np.float32) * F(32)), NW._cv_round(np.asarray(ymap, np.float32) * F(32))
            ix, iy = np.clip((sx + 16) >> 5, 0, W - 1), np.clip((sy + 16) >> 5, 0, H - 1)
    out = np.zeros(np.shape(xmap), np.uint8)
    if variant == "interior_255":   # wavefronts whose four taps are inside store 255 without a look at the mask
        sx, sy = NW._cv_round(np.asarray(xmap, np.float32) * F(32)), NW._cv_round(np.asarray(ymap, np.float32) * F(32))
        interior = (sx >= 0) & (sx <= 32 * (W - 1) - 1) & (sy >= 0) & (sy <= 32 * (H - 1) - 1)
        out[inside] = mask[iy[inside], ix[inside]]
        out[interior] = 255
    elif variant == "border_replicated":
        out[...] = mask[np.clip(iy, 0, H - 1), np.clip(ix, 0, W - 1)]
    elif variant == "xy_swapped":
        out[inside] = mask[ix[inside] % H, iy[inside] % W]
    elif variant == "pitch_is_width":
        flat = np.asarray(wide).reshape(-1)[x_off:]
        out[inside] = flat[iy[inside] * W + ix[inside]]
    else:
        out[inside] = mask[iy[inside], ix[inside]]
    return out


def footprint(i, src_n, dst_n):
    """[first, end) of the source pixels under pixel i of an axis shrunk from src_n to dst_n"""
    return i * src_n // dst_n, ((i + 1) * src_n + dst_n - 1) // dst_n


def shrink_mask(mask, size):
    """Conservative shrink to size = (w, h), w <= mask width, h <= mask height: 255 where EVERY pixel of the footprint is non-zero, else 0.
    Separable: an axis at a time, the minimum of the 0 / 1 image over each footprint."""
    m = (np.asarray(mask) != 0).astype(np.uint8)
    sh, sw = m.shape
    dw, dh = int(size[0]), int(size[1])
    if not (0 < dw <= sw and 0 < dh <= sh):
        raise ValueError(f"shrink of {sw}x{sh} to {dw}x{dh}")
    cols = np.stack([m[:, slice(*footprint(x, sw, dw))].min(axis=1) for x in range(dw)], axis=1)
    rows = np.stack([cols[slice(*footprint(y, sh, dh)), :].min(axis=0) for y in range(dh)], axis=0)
    return (rows * 255).astype(np.uint8)


def shrink_mask_brute(mask, size):
    """the same, pixel by pixel, straight from the sentence"""
    mask = np.asarray(mask)
    sh, sw = mask.shape
    dw, dh = int(size[0]), int(size[1])
    out = np.zeros((dh, dw), np.uint8)
    for y in range(dh):
        y0, y1 = footprint(y, sh, dh)
        for x in range(dw):
            x0, x1 = footprint(x, sw, dw)
            out[y, x] = 255 if all(mask[sy, sx] != 0 for sy in range(y0, y1) for sx in range(x0, x1)) else 0
    return out
