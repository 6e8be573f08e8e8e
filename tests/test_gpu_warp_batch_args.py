"""The argument rules of stx_warp_batch (include/stitching_amd.h), called through ctypes: every refusal returns STX_ERR_INVALID with a
message that names the rule, before the device is touched — no output slot is filled, the table handle stays as it was and no table
kernel is launched (include/stitching_amd_debug.h: stx_debug_warp_table_launches does not move).  And the positive case the rules
protect: the first panorama of a rig (STX_WARP_FRESH_ROIS with a table handle), then its ROIs as the rectangles of the second.

Shapes: two 64 x 48 u8x3 frames, a plane and a spherical warper (both typed projectors: one table launch per call of up to 8 images)."""
import ctypes as C
import math

import numpy as np
import pytest

import stitching_amd as S
from stitching_amd import _lib, synthetic
from stitching_amd.camera import CameraParams

pytestmark = pytest.mark.gpu

W, H, N = 64, 48, 2
IP = C.POINTER(C.c_int)


def table_launches(ctx):
    n = C.c_int(-1)
    assert ctx._lib.stx_debug_warp_table_launches(ctx.handle, C.byref(n)) == 0
    return n.value


class Rig:
    """two frames on `ctx` and the arguments every stx_warp_batch call of this file shares"""

    def __init__(self, ctx, kind):
        self.ctx = ctx
        self.warper = S.Warper(kind, ctx=ctx)
        self.cams = [CameraParams(focal=150.0 + 3.0 * i, aspect=1.0, ppx=W / 2.0, ppy=H / 2.0,
                                  R=(synthetic.rot_y(math.radians(-7.0 + 14.0 * i)) @ synthetic.rot_x(math.radians(1.5 * i))).astype(np.float32))
                     for i in range(N)]
        self.warper.set_scale(self.cams)
        self.Ks, self.Rs = self.warper.camera_arrays(self.cams)
        rng = np.random.default_rng(3)
        self.srcs = [S.DeviceImage.from_numpy(rng.integers(0, 256, (H, W, 3)).astype(np.uint8), ctx) for _ in range(N)]
        self.h_src = (C.c_void_p * N)(*[s._h for s in self.srcs])
        self.gains = [S.DeviceImage.from_numpy(np.full((3, 4), 1.25, np.float32), ctx) for _ in range(N)]
        self.h_gain = (C.c_void_p * N)(*[g._h for g in self.gains])
        corners, sizes = self.warper.warp_rois([(W, H)] * N, self.cams)
        self.rois = np.ascontiguousarray([c + s for c, s in zip(corners, sizes)], np.int32)

    def call(self, rects=None, gain_maps=None, flags=0, imgs=True, masks=True, xywh=True, tables=None):
        """-> (rc, out_imgs or None, out_masks or None, out_xywh or None)"""
        fp = C.POINTER(C.c_float)
        h_img = (C.c_void_p * N)() if imgs else None
        h_mask = (C.c_void_p * N)() if masks else None
        out = np.full((N, 4), -1, np.int32) if xywh else None
        rc = self.ctx._lib.stx_warp_batch(self.ctx.handle, self.warper._type_id(), float(self.warper.scale), N, self.Ks.ctypes.data_as(fp),
                                          self.Rs.ctypes.data_as(fp), self.h_src, None if rects is None else rects.ctypes.data_as(IP),
                                          gain_maps, None, flags, h_img, h_mask, None if out is None else out.ctypes.data_as(IP),
                                          None if tables is None else C.byref(tables))
        return rc, h_img, h_mask, out

    def take(self, handles):
        """the buffers a successful call handed out, as arrays (and freed)"""
        return [S.DeviceImage(self.ctx, C.c_void_p(h)).numpy() for h in handles]


@pytest.fixture(scope="module", params=["plane", "spherical"])
def rig(request, gpu_ctx):
    return Rig(gpu_ctx, request.param)


REFUSALS = [
    ("nothing requested", dict(imgs=False, masks=False)),
    ("gains without images", dict(gains=True, imgs=False)),
    ("needs out_xywh", dict(flags=_lib.WARP_FRESH_ROIS, xywh=False)),
    ("with rects_xywh", dict(flags=_lib.WARP_FRESH_ROIS, rects=True)),
    ("kept tables belong to given rectangles", dict(tables=True)),
    ("unknown flags", dict(flags=2)),
    ("unknown flags", dict(flags=_lib.WARP_FRESH_ROIS | 4)),
]


@pytest.mark.parametrize("rule,args", REFUSALS, ids=[f"{r[0]}-{i}" for i, r in enumerate(REFUSALS)])
def test_refused_before_the_device_is_touched(rig, rule, args):
    rc, h_img, h_mask, _ = rig.call()  # a call that launches tables: the counter now holds 1, and a refusal must leave it there
    assert rc == 0
    rig.take(h_img), rig.take(h_mask)
    before = table_launches(rig.ctx)
    assert before == 1
    args = dict(args)
    tables = C.c_void_p() if args.pop("tables", False) else None
    if args.pop("rects", False):
        args["rects"] = rig.rois
    if args.pop("gains", False):
        args["gain_maps"] = rig.h_gain
    rc, h_img, h_mask, _ = rig.call(tables=tables, **args)
    assert rc == -1  # STX_ERR_INVALID
    assert rule in rig.ctx._lib.stx_last_error().decode()
    for handles in (h_img, h_mask):
        assert handles is None or all(h is None for h in handles)
    assert tables is None or not tables.value
    assert table_launches(rig.ctx) == before


def test_another_contexts_handle_is_refused_and_left_alone(rig):
    tables = C.c_void_p()
    rc, h_img, h_mask, _ = rig.call(rects=rig.rois, tables=tables)
    assert rc == 0 and tables.value
    rig.take(h_img), rig.take(h_mask)
    held = tables.value
    other = Rig(S.Context(rig.ctx.device), rig.warper.warper_type)
    rc, h_img, h_mask, _ = other.call()
    assert rc == 0
    other.take(h_img), other.take(h_mask)
    before = table_launches(other.ctx)
    assert before == 1
    rc, h_img, h_mask, _ = other.call(rects=rig.rois, tables=tables)
    assert rc == -1
    assert "another context" in other.ctx._lib.stx_last_error().decode()
    assert all(h is None for h in h_img) and all(h is None for h in h_mask)
    assert tables.value == held
    assert table_launches(other.ctx) == before
    assert rig.ctx._lib.stx_warp_tables_free(tables) == 0


def test_first_panorama_then_its_rois_as_rectangles(rig):
    tables = C.c_void_p()
    rc, h_img, h_mask, rois = rig.call(flags=_lib.WARP_FRESH_ROIS, tables=tables)
    assert rc == 0, rig.ctx._lib.stx_last_error()
    assert tables.value
    assert np.array_equal(rois, rig.rois)
    assert table_launches(rig.ctx) == 1
    first = rig.take(h_img)
    rig.take(h_mask)
    assert [a.shape for a in first] == [(r[3], r[2], 3) for r in rois]
    rc, h_img, h_mask, echo = rig.call(rects=rois, masks=False, tables=tables)
    assert rc == 0, rig.ctx._lib.stx_last_error()
    assert h_mask is None
    assert np.array_equal(echo, rois)
    assert table_launches(rig.ctx) == 0  # the kept tables answered
    second = rig.take(h_img)
    assert all(np.array_equal(a, b) for a, b in zip(first, second))
    assert rig.ctx._lib.stx_warp_tables_free(tables) == 0
