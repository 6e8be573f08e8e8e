"""The tuned warp kernel writes an image, a mask or both (csrc/stx_warp.hip: warp_fast_kernel<TYPE, IMG, MASK, ...>), with or without the
block gain in its epilogue, through one of two stores: the unpredicated full-tile store, or the predicated one of the tiles whose rows
end with the image or whose columns end with the row pitch.  Which of the two a wavefront takes may depend only on the outputs its
launch writes.  Every output selection, with rectangles that give full tiles, partial last columns, partial last rows and nothing but
edge tiles, on both launch grids — against the oracle's warp_image / create_and_warp_mask / block_gain_apply cut to the rectangle, byte
for byte; and the image-only images against those of the image + mask call, the mask-only masks against its masks.
These tests pin the BYTES of both stores in every instantiation; which store a launch takes changes its time and not its bytes, and is
pinned by the measurement (profiles/warp_full_tiles.md), not here."""
import numpy as np
import pytest

import stitching_amd as S
from stitching_amd import synthetic

pytestmark = pytest.mark.gpu

WTYPES = ["spherical", "cylindrical", "plane"]
# source size, (yaw, pitch, roll) in degrees of the three cameras
SHAPES = {
    "tiles": ((720, 405), [(-14.0, 2.0, 0.0), (0.0, -3.0, 3.0), (15.0, 1.0, -2.0)]),   # ROIs of more than 512 columns
    "edge": ((333, 251), [(-10.0, 0.0, 1.0), (0.0, 5.0, 0.0), (12.0, -2.0, -3.0)]),
    "pitched": ((333, 251), [(20.0, 50.0, 7.0), (-15.0, -50.0, -5.0), (5.0, 50.0, 0.0)]),  # mirror, periodic and generic wavefronts
}
_cache = {}


def camera(w, h, yaw, pitch, roll):
    R = synthetic.rot_y(np.radians(yaw)) @ synthetic.rot_x(np.radians(pitch)) @ synthetic.rot_z(np.radians(roll))
    return S.CameraParams(focal=0.75 * w, aspect=1.0, ppx=w / 2.0, ppy=h / 2.0, R=R.astype(np.float32))


def gain_maps(sizes):
    """one fp32 block-gain map per warped image (blocks of 32 pixels): smooth maps within [0.7, 1.4]; the last one also holds a patch
    of 2.5, where the products leave 0..255 and cvt_pk_u8 has to saturate"""
    maps = []
    for k, (w, h) in enumerate(sizes):
        gh, gw = (h + 31) // 32 + 1, (w + 31) // 32 + 1
        yy, xx = np.mgrid[0:gh, 0:gw]
        maps.append((1.05 + 0.35 * np.sin(0.9 * xx + k) * np.cos(0.6 * yy - k)).astype(np.float32))
    assert all(m.min() >= 0.7 and m.max() <= 1.4 for m in maps)
    maps[-1][1:3, 1:4] = np.float32(2.5)
    return maps


def expected(oracle, wtype, shape, mode):
    """The oracle's whole warped images, masks and compensated images of a shape's three cameras, made once per (warper, shape, remap
    model) and shared by the tests (read only)."""
    key = (wtype, shape, mode)
    if key not in _cache:
        (w, h), angles = SHAPES[shape]
        cams = [camera(w, h, *a) for a in angles]
        imgs = [synthetic.make_frame(50 + i, w, h) for i in range(3)]
        o = oracle.Warper(wtype)
        o.set_scale(cams)
        rois = [o.warp_roi((w, h), c) for c in cams]
        gmaps = gain_maps([r[2:4] for r in rois])
        oi = [o.warp_image(im, c) for im, c in zip(imgs, cams)]
        om = [o.create_and_warp_mask((w, h), c) for c in cams]
        og = [oracle.block_gain_apply(a, g) for a, g in zip(oi, gmaps)]
        for a in oi + om + og:
            a.setflags(write=False)
        _cache[key] = dict(size=(w, h), cams=cams, imgs=imgs, rois=rois, gmaps=gmaps, oi=oi, om=om, og=og)
    return _cache[key]


@pytest.fixture()
def model(oracle, request):
    """the remap model of the case on both sides, the previous ones back afterwards"""
    prev_p, prev_o = S.remap_mode(), oracle.set_model()
    mode = request.param
    S.set_remap_mode(mode)
    oracle.set_model(**{**prev_o, "remap": mode})
    yield mode
    S.set_remap_mode(prev_p)
    oracle.set_model(**prev_o)


# ---------------------------------------------------------------------------------------------------------------- rectangles
def whole(roi):
    return tuple(roi)


def trimmed(roi, w=None, h=None):
    """The ROI (or its top-left w x h) cut to a width of 37 modulo 64 and a height of 3 modulo 4: a buffer's row pitch is its width
    rounded up to 8 pixels, then to 64 bytes, so it ends inside the last 64-column tile (partial last column), and the last block of 4
    rows ends with the image (partial last row)."""
    x, y, rw, rh = roi
    rw, rh = min(rw, w or rw), min(rh, h or rh)
    return (x, y, rw - (rw - 37) % 64, rh - (rh - 3) % 4)


def off_grid(roi, w=401):
    """strictly inside the ROI, at an odd offset, with a width that is no multiple of 4"""
    x, y, rw, rh = roi
    return (x + 37, y + 5, min(w, rw - 37 - 3), rh - 5 - 6)


def sliver(roi):
    """narrower than one 64-column tile AND than its pitch (37 columns -> 128 bytes of the tile's 192), 7 rows: edge tiles only"""
    x, y, rw, rh = roi
    return (x + 37, y + 5, 37, 7)


def pitch_bytes(w):
    return ((w + 7) // 8 * 8 * 3 + 63) // 64 * 64


def tile_kinds(rect):
    """(full tiles, tiles with a partial last column, tiles with a partial last row) of the image output of a rectangle"""
    _, _, w, h = rect
    cols = [(xw * 3 + 192 <= pitch_bytes(w)) for xw in range(0, w, 64)]
    rows = [(y0 + 4 <= h) for y0 in range(0, h, 4)]
    full = sum(cols) * sum(rows)
    return full, (len(cols) - sum(cols)) * len(rows), (len(rows) - sum(rows)) * len(cols)


def flat_grid(rects):
    """launch_typed's choice (csrc/stx_warp.hip): the 1-D grid when the (largest image, 1, images) grid would launch more than 5 % empty
    workgroups.  An image owns 8 x (bands of 4 tile rows per XCD, whole bands) x 4 x (tiles per row) workgroups."""
    own = [8 * ((((h + 3) // 4 + 3) // 4 + 7) // 8) * 4 * ((w + 63) // 64) for _, _, w, h in rects]
    return sum(own) < 0.95 * max(own) * len(own)


def cut(a, roi, rect):
    x0, y0 = rect[0] - roi[0], rect[1] - roi[1]
    assert 0 <= x0 and 0 <= y0 and x0 + rect[2] <= roi[2] and y0 + rect[3] <= roi[3], (roi, rect)
    return a[y0:y0 + rect[3], x0:x0 + rect[2]]


def batches(shape, rois):
    """name -> three rectangles (one per camera).  "mixed": unequal sizes, the flat grid; "equal": one size, the z grid."""
    if shape == "tiles":
        mixed = [trimmed(rois[0]), whole(rois[1]), off_grid(rois[2])]
    elif shape == "edge":
        mixed = [sliver(rois[0]), whole(rois[1]), trimmed(rois[2])]
    else:
        mixed = [off_grid(rois[0]), off_grid(rois[1], 203), sliver(rois[2])]
    w, h = min(r[2] for r in rois), min(r[3] for r in rois)
    if shape == "pitched":
        equal = [off_grid((r[0], r[1], w, h)) for r in rois]
    else:
        equal = [trimmed(r, w, h) for r in rois]
    return {"mixed": mixed, "equal": equal}


def same(a, b, what):
    a = np.asarray(a)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(a, b), f"{what}: {int(np.count_nonzero(a != b))} differing bytes"


CASES = [("tiles", "q15"), ("edge", "q15"), ("pitched", "q15"), ("tiles", "float"), ("edge", "float")]


@pytest.mark.parametrize("gain", [False, True], ids=["plain", "gain"])
@pytest.mark.parametrize("shape,model", CASES, indirect=["model"], ids=[f"{s}-{m}" for s, m in CASES])
@pytest.mark.parametrize("wtype", WTYPES)
def test_image_only_equals_image_and_mask_and_the_oracle(oracle, gpu_ctx, wtype, shape, model, gain):
    e = expected(oracle, wtype, shape, model)
    rois, (w, h) = e["rois"], e["size"]
    g = S.Warper(wtype)
    g.set_scale(e["cams"])
    assert [g.warp_roi((w, h), c) for c in e["cams"]] == rois
    comp = None
    if gain:
        comp = S.ExposureErrorCompensator("gain_blocks")
        comp.set_gains(e["gmaps"])
    want_img = e["og"] if gain else e["oi"]
    sets = batches(shape, rois)
    # the shapes reach what they were chosen for
    assert flat_grid(sets["mixed"]) and not flat_grid(sets["equal"])
    kinds = np.array([tile_kinds(r) for r in sets["mixed"] + sets["equal"]])
    if shape == "tiles":
        assert all(r[2] > 512 for r in rois) and (kinds[0] > 0).all() and sets["mixed"][0][3] % 4 != 0
    if shape == "edge":
        assert kinds[0][0] == 0 and kinds[0][1] > 0 and kinds[0][2] > 0  # the sliver: no full tile at all
    if shape == "pitched":
        assert all(r[2] % 4 != 0 and (r[0] - q[0], r[1] - q[1]) == (37, 5) for r, q in zip(sets["mixed"], rois))
        assert sets["mixed"][0][2] == 401
    for name, rects in sets.items():
        both_i, both_m, out_rects = g.warp_images_and_masks(e["imgs"], e["cams"], rects=rects, compensator=comp)
        only_i, none, _ = g.warp_images_and_masks(e["imgs"], e["cams"], rects=rects, compensator=comp, masks=False)
        assert none is None and [tuple(r) for r in out_rects] == [tuple(r) for r in rects]
        for k, rect in enumerate(rects):
            what = f"{wtype} {shape} {model} {name}[{k}] {rect}"
            same(both_i[k], cut(want_img[k], rois[k], rect), what + " image of image + mask")
            same(both_m[k], cut(e["om"][k], rois[k], rect), what + " mask of image + mask")
            same(only_i[k], cut(want_img[k], rois[k], rect), what + " image-only")
            same(only_i[k], np.asarray(both_i[k]), what + " image-only against image + mask")
    # one image, no rectangle: the whole ROI through the single-image entry points
    if gain:
        one_i, one_m, _ = g.warp_images_and_masks(e["imgs"][2:], e["cams"][2:], compensator=_one(e["gmaps"][2]))
        same(one_i[0], want_img[2], f"{wtype} {shape} whole image with the 2.5 patch")
        same(one_m[0], e["om"][2], f"{wtype} {shape} whole mask")
    else:
        same(g.warp_image(e["imgs"][1], e["cams"][1]), e["oi"][1], f"{wtype} {shape} warp_image")


def _one(gmap):
    comp = S.ExposureErrorCompensator("gain_blocks")
    comp.set_gains([gmap])
    return comp


def test_the_gain_saturates(oracle):
    """the 2.5 patch of the last map does drive bytes to 255 in the oracle's compensated image (what the gain cases compare against)"""
    e = expected(oracle, "spherical", "tiles", "q15")
    assert np.count_nonzero((e["og"][2] == 255) & (e["oi"][2] < 255) & (e["oi"][2] > 102)) > 100


@pytest.mark.parametrize("shape", ["tiles", "edge"])
@pytest.mark.parametrize("wtype", WTYPES)
def test_mask_only_equals_the_oracle_and_image_and_mask(oracle, gpu_ctx, wtype, shape):
    e = expected(oracle, wtype, shape, "q15")
    g = S.Warper(wtype)
    g.set_scale(e["cams"])
    sizes = [e["size"]] * 3
    only = [np.asarray(m) for m in g.create_and_warp_masks(sizes, e["cams"])]
    _, both, rois = g.warp_images_and_masks(e["imgs"], e["cams"])
    assert [tuple(r) for r in rois] == [tuple(r) for r in e["rois"]]
    # a mask's row pitch is its width rounded up to 64 bytes, so every tile column is a full one: the predicated store is reached through
    # the last block of rows alone, where the ROI's height is no multiple of 4 — next to blocks of 4 whole rows (the full-tile store)
    assert any(r[3] % 4 != 0 for r in rois) and all(r[3] >= 8 for r in rois)
    for k in range(3):
        same(only[k], e["om"][k], f"{wtype} {shape} mask-only {k}")
        same(only[k], np.asarray(both[k]), f"{wtype} {shape} mask-only against image + mask {k}")
        assert 0 < np.count_nonzero(only[k]) <= only[k].size
