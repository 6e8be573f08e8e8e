"""The column / row tables of the typed projectors kept per rig (stx_warp.hip: launch_typed with a stx_warp_tables handle;
the `tables` argument of stx_warp_batch).  The tables follow from the cameras, the
rectangles, the scale and the trig mode: a call whose record equals the handle's launches no table kernel and reads the kept block, any
difference makes the tables again.  Every comparison is byte for byte with a call that takes no handle.
include/stitching_amd_debug.h: stx_debug_warp_table_launches tells how many table kernels the last batched warp launched.

Shapes: three frames of different sizes (203 x 150, 160 x 121, 96 x 64) warped into rectangles whose widths and heights are no multiples
of 4 — the table block's layout rounds every column table up to 4 entries and every row table to 4 rows, and aligns the row blocks to 64
bytes, so each image's tables start at an offset the sizes before it decide; and nine 96 x 64 frames: two launch batches (8 + 1), the
second one's tables behind the first's in the same block."""
import ctypes as C
import math

import numpy as np
import pytest

import stitching_amd as S
from stitching_amd import config, synthetic
from stitching_amd.camera import CameraParams
from stitching_amd.warper import WarpTables

pytestmark = pytest.mark.gpu

SIZES3 = [(203, 150), (160, 121), (96, 64)]
SIZES9 = [(96, 64)] * 9


def cameras(kind, sizes):
    if kind == "affine":
        return synthetic.affine_scan_cameras(len(sizes), 90, 60)
    cams = []
    for i, (w, h) in enumerate(sizes):
        yaw = -14.0 + 28.0 * i / max(len(sizes) - 1, 1)
        R = synthetic.rot_y(math.radians(yaw)) @ synthetic.rot_x(math.radians(2.0 * math.sin(1.7 * i))) @ synthetic.rot_z(math.radians(math.cos(2.3 * i)))
        cams.append(CameraParams(focal=150.0 + 3.0 * i, aspect=1.0, ppx=w / 2.0, ppy=h / 2.0, R=R.astype(np.float32)))
    return cams


def frames(seed, sizes):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3)).astype(np.uint8) for w, h in sizes]


def odd_rects(warper, sizes, cams):
    """a rectangle inside every ROI, one pixel in from its corner, with a width and a height that are no multiples of 4"""
    corners, wsizes = warper.warp_rois(sizes, cams)
    rects = []
    for (x, y), (w, h) in zip(corners, wsizes):
        rw, rh = w - 2, h - 2
        rw -= 1 if rw % 4 == 0 else 0
        rh -= 1 if rh % 4 == 0 else 0
        assert rw > 8 and rh > 8 and rw % 4 and rh % 4
        rects.append((x + 1, y + 1, rw, rh))
    return rects


def table_launches(ctx):
    n = C.c_int(-1)
    assert ctx._lib.stx_debug_warp_table_launches(ctx.handle, C.byref(n)) == 0
    return n.value


def warp(ctx, warper, imgs, cams, rects, tables=None, compensator=None):
    """-> (the warped images as arrays, table kernels launched)"""
    prev = config.device_resident()
    config.set_device_resident(True)
    try:
        out, masks, _ = warper.warp_images_and_masks([S.DeviceImage.from_numpy(a, ctx) for a in imgs], cams, rects=rects, masks=False,
                                                     tables=tables, compensator=compensator)
    finally:
        config.set_device_resident(prev)
    assert masks is None
    return [np.asarray(o) for o in out], table_launches(ctx)


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def make(ctx, kind, sizes):
    warper = S.Warper(kind, ctx=ctx)
    cams = cameras(kind, sizes)
    warper.set_scale(cams)
    return warper, cams, odd_rects(warper, sizes, cams)


@pytest.mark.parametrize("kind", ["spherical", "cylindrical", "plane", "affine", "mercator"])
@pytest.mark.parametrize("sizes", [SIZES3, SIZES9], ids=["three", "nine"])
def test_kept_tables_are_made_once(gpu_ctx, kind, sizes):
    """the first call fills the handle, the next two (new pixels) launch no table kernel; all three equal a call without a handle"""
    warper, cams, rects = make(gpu_ctx, kind, sizes)
    batches = (len(sizes) + 7) // 8
    t = WarpTables()
    for k, seed in enumerate((1, 2, 3)):
        imgs = frames(seed, sizes)
        plain, n_plain = warp(gpu_ctx, warper, imgs, cams, rects)
        kept, n_kept = warp(gpu_ctx, warper, imgs, cams, rects, tables=t)
        assert n_plain == batches
        assert n_kept == (batches if k == 0 else 0), f"call {k}"
        assert same(plain, kept), f"call {k}"
        assert [p.shape[:2] for p in plain] == [(r[3], r[2]) for r in rects]
    t.free()


def test_whatever_the_tables_depend_on_makes_them_again(gpu_ctx):
    """another camera, rectangle, scale or trig mode: tables again, and the bytes of a fresh call; the same call after it: kept"""
    sizes = SIZES3
    warper, cams, rects = make(gpu_ctx, "spherical", sizes)
    imgs = frames(4, sizes)
    t = WarpTables()
    assert warp(gpu_ctx, warper, imgs, cams, rects, tables=t)[1] == 1
    assert warp(gpu_ctx, warper, imgs, cams, rects, tables=t)[1] == 0

    def check(what, warper, cams, rects):
        plain, _ = warp(gpu_ctx, warper, imgs, cams, rects)
        kept, n = warp(gpu_ctx, warper, imgs, cams, rects, tables=t)
        assert n == 1 and same(plain, kept), what
        again, n = warp(gpu_ctx, warper, imgs, cams, rects, tables=t)
        assert n == 0 and same(plain, again), what
        return plain

    base = warp(gpu_ctx, warper, imgs, cams, rects)[0]
    # a camera pitched by 1.5 degrees: kr[1], kr[4], kr[7] of that image
    turned = list(cams)
    c = cams[1]
    R2 = (np.asarray(c.R, np.float64) @ synthetic.rot_x(math.radians(1.5))).astype(np.float32)
    turned[1] = CameraParams(focal=c.focal, aspect=1.0, ppx=c.ppx, ppy=c.ppy, R=R2)
    assert not same(check("camera", warper, turned, rects), base)
    # the three factors of the row products one at a time (kr = K R^T: kr[1] = fx R[1][0] + skew R[1][1] + ppx R[1][2], kr[4] = fy R[1][1] +
    # ppy R[1][2], kr[7] = R[1][2]): ppx moves kr[1] alone, ppy kr[4] alone, a roll kr[1] and kr[4] but not kr[7]
    def cam(c, **kw):
        a = dict(focal=c.focal, aspect=1.0, ppx=c.ppx, ppy=c.ppy, R=np.asarray(c.R, np.float32).copy())
        a.update(kw)
        return CameraParams(**a)

    for what, other in (("ppx: kr[1]", cam(c, ppx=c.ppx + 0.5)), ("ppy: kr[4]", cam(c, ppy=c.ppy + 0.5)),
                        ("roll: kr[1], kr[4]", cam(c, R=(np.asarray(c.R, np.float64) @ synthetic.rot_z(math.radians(0.7))).astype(np.float32)))):
        one = list(cams)
        one[1] = other
        check(what, warper, one, rects)
    # kr[7] alone: with the principal point at the origin R[1][2] reaches neither kr[1] nor kr[4]
    one = list(cams)
    one[1] = cam(c, ppx=0.0, ppy=0.0)
    check("principal point at the origin", warper, one, rects)
    R3 = np.asarray(c.R, np.float32).copy()
    R3[1, 2] += np.float32(0.002)
    one[1] = cam(c, ppx=0.0, ppy=0.0, R=R3)
    check("R[1][2]: kr[7]", warper, one, rects)
    check("cameras back", warper, cams, rects)
    # a rectangle moved by one column (the same size: the block's layout stays, its content does not), then a narrower one
    moved = list(rects)
    moved[2] = (rects[2][0] + 1,) + tuple(rects[2][1:])
    check("rectangle moved", warper, cams, moved)
    moved[2] = (rects[2][0], rects[2][1], rects[2][2] - 4, rects[2][3])
    check("rectangle narrowed", warper, cams, moved)
    # the scale
    scaled = S.Warper("spherical", ctx=gpu_ctx)
    scaled.scale = warper.scale * 1.01
    check("scale", scaled, cams, rects)
    check("scale back", warper, cams, rects)
    # the trig mode
    prev = config.trig_mode()
    try:
        config.set_trig_mode("glibc" if prev != "glibc" else "exact")
        check("trig mode", warper, cams, rects)
    finally:
        config.set_trig_mode(prev)
    check("trig mode back", warper, cams, rects)
    # the projector: the sphere's tables do not answer for the cylinder
    cyl = S.Warper("cylindrical", ctx=gpu_ctx)
    cyl.scale = warper.scale
    check("projector", cyl, cams, rects)
    t.free()


def test_the_affine_translations_one_at_a_time(gpu_ctx):
    """t[0] and t[1] of the plane projector's tables (the affine warper: T = -(H' (tx, ty, 0)) with H' the transposed linear part): with
    an unrotated H, tx reaches t[0] alone and ty t[1] alone"""
    sizes = SIZES3

    def cams_of(shifts):
        out = []
        for tx, ty in shifts:
            Hm = np.array([[1, 0, tx], [0, 1, ty], [0, 0, 1]], np.float32)
            out.append(CameraParams(focal=1.0, aspect=1.0, ppx=0.0, ppy=0.0, R=Hm))
        return out

    shifts = [(0.0, 0.0), (150.25, 3.5), (290.5, -2.25)]
    warper = S.Warper("affine", ctx=gpu_ctx)
    cams = cams_of(shifts)
    warper.set_scale(cams)
    rects = odd_rects(warper, sizes, cams)
    imgs = frames(11, sizes)
    t = WarpTables()
    assert warp(gpu_ctx, warper, imgs, cams, rects, tables=t)[1] == 1
    for what, k, d in (("tx: t[0]", 1, (0.75, 0.0)), ("ty: t[1]", 2, (0.0, 0.75))):
        moved = list(shifts)
        moved[k] = (shifts[k][0] + d[0], shifts[k][1] + d[1])
        plain, _ = warp(gpu_ctx, warper, imgs, cams_of(moved), rects)
        kept, n = warp(gpu_ctx, warper, imgs, cams_of(moved), rects, tables=t)
        assert n == 1 and same(plain, kept), what
        again, n = warp(gpu_ctx, warper, imgs, cams_of(moved), rects, tables=t)
        assert n == 0 and same(plain, again), what
        back, n = warp(gpu_ctx, warper, imgs, cams, rects, tables=t)
        assert n == 1 and same(back, warp(gpu_ctx, warper, imgs, cams, rects)[0]) and not same(back, plain), what
    t.free()


def test_the_fused_gain_reads_the_kept_tables(gpu_ctx):
    sizes = SIZES3
    warper, cams, rects = make(gpu_ctx, "spherical", sizes)
    comp = S.ExposureErrorCompensator("gain_blocks", estimator=object())
    rng = np.random.default_rng(7)
    comp.set_gains([(0.8 + 0.4 * rng.random((5, 7))).astype(np.float32) for _ in sizes])
    t = WarpTables()
    for k, seed in enumerate((5, 6)):
        imgs = frames(seed, sizes)
        plain, _ = warp(gpu_ctx, warper, imgs, cams, rects, compensator=comp)
        kept, n = warp(gpu_ctx, warper, imgs, cams, rects, tables=t, compensator=comp)
        assert n == (1 if k == 0 else 0) and same(plain, kept)
    # the handle a gain call filled answers a call without gains, and the other way round
    imgs = frames(8, sizes)
    kept, n = warp(gpu_ctx, warper, imgs, cams, rects, tables=t)
    assert n == 0 and same(kept, warp(gpu_ctx, warper, imgs, cams, rects)[0])
    assert not same(kept, warp(gpu_ctx, warper, imgs, cams, rects, compensator=comp)[0])
    t.free()


def test_another_contexts_handle_is_refused(gpu_ctx):
    sizes = SIZES3
    warper, cams, rects = make(gpu_ctx, "spherical", sizes)
    imgs = frames(9, sizes)
    t = WarpTables()
    warp(gpu_ctx, warper, imgs, cams, rects, tables=t)
    other = S.Context(gpu_ctx.device)
    w2 = S.Warper("spherical", ctx=other)
    w2.scale = warper.scale
    with pytest.raises(S.StitchingError, match="another context"):
        warp(other, w2, imgs, cams, rects, tables=t)
    assert warp(gpu_ctx, warper, imgs, cams, rects, tables=t)[1] == 0  # and is as good as before
    t.free()
