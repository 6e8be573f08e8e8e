"""The constructed blend families (tests/constructed_blends.py) on the MI355X: every scene through the feather or the "no" blender
of the C ABI (`_BlenderHandle`, as S.Blender drives it), the u8 panorama, its mask and the int16 panorama of blend(want_s16=True)
against the oracle's with 0 differing bytes, and the inputs read back unmodified.  For the probe scenes the int16 panorama IS the
distance transform (constructed_blends.probe_value is strictly increasing).  What each family reaches, that its facts hold, and that
it tells the contract from a subtly wrong variant is asserted without a GPU in tests/test_constructed_blends.py; here only the device
is asked."""
import functools

import numpy as np
import pytest

import stitching_amd as S
from oracle import oracle as O
from stitching_amd import _lib
from stitching_amd.blender import _BlenderHandle
from tests import constructed_blends as CB

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case(builder, *args):
    """(scene, the oracle's int16 panorama, u8 panorama and mask): built once per case, never written to"""
    scene = getattr(CB, builder)(*args)
    b = O._OracleBlenderHandle(scene.kind, 0, scene.sharpness)
    b.prepare(scene.roi)
    for img, mask, corner in scene.feeds:
        b.feed(np.asarray(img).astype(np.int16), mask, corner)
    out16, mask = b.blend()
    for a in (out16, mask):
        a.setflags(write=False)
    return scene, out16, O.convert_scale_abs(out16), mask


def _pitched(a, ctx, fill, xoff=7):
    """`a` as a view, `xoff` columns into a larger device buffer whose surroundings hold `fill` ("random": seeded bytes).
    -> (view, check): check() reads the whole buffer back and asserts that neither the view nor its surroundings changed"""
    shape = (a.shape[0] + 9, a.shape[1] + xoff + 13) + a.shape[2:]
    if isinstance(fill, str):
        big = np.random.default_rng(a.shape[1]).integers(0, 256, shape).astype(a.dtype)
    else:
        big = np.full(shape, fill, a.dtype)
    big[5:5 + a.shape[0], xoff:xoff + a.shape[1]] = a
    dev = S.DeviceImage.from_numpy(big, ctx)

    def check():
        assert np.array_equal(dev.numpy(), big)

    return dev[5:5 + a.shape[0], xoff:xoff + a.shape[1]], check


def _plain(a, ctx):
    dev = S.DeviceImage.from_numpy(a, ctx)
    before = a.copy()

    def check():
        assert np.array_equal(dev.numpy(), before) and np.array_equal(a, before)

    return dev, check


def _run(ctx, case, views=None):
    """the scene on the device against the oracle.  views: {feed index: (image fill, mask fill, x offset)} — those feeds as views into
    larger buffers; the others as buffers of their own (one upload per distinct array)"""
    scene, want16, want8, wantm = case
    up, checks = {}, []

    def dev(a, spec):
        key = (id(a), spec)
        if key not in up:
            up[key], check = _plain(a, ctx) if spec is None else _pitched(a, ctx, *spec)
            checks.append(check)
        return up[key]

    b = _BlenderHandle(ctx, scene.kind, 0, scene.sharpness, scene.roi)
    for k, (img, mask, corner) in enumerate(scene.feeds):
        v = (views or {}).get(k)
        b.feed(dev(img, v and (v[0], v[2])), dev(mask, v and (v[1], v[2])), corner)
    pano, mask, p16 = (d.numpy() for d in b.blend(want_s16=True))
    assert pano.dtype == np.uint8 and mask.dtype == np.uint8 and p16.dtype == np.int16
    assert pano.shape == want8.shape and mask.shape == wantm.shape and p16.shape == want16.shape
    differing = [int(np.count_nonzero(g != w)) for g, w in ((p16, want16), (pano, want8), (mask, wantm))]
    assert differing == [0, 0, 0], differing
    for check in checks:
        check()


# ---------------------------------------------------------------------------------------------------------------------------------
# the distance transform, through the probe
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rot", range(len(CB.CHUNK_EDGE_ROWS)))
@pytest.mark.parametrize("h", CB.CHUNK_EDGE_H)
def test_chunk_edges(gpu_ctx, h, rot):
    """zero rows on 0, 31 / 32, 63 / 64 and the last row, another one in every column of a lane's group; heights around 8, 32, 64, 128"""
    _run(gpu_ctx, _case("chunk_edges", h, rot))


@pytest.mark.parametrize("where", CB.FAR_LINK_WHERE)
def test_far_links(gpu_ctx, where):
    """four or five empty chunks between a pixel and its nearest zero row"""
    _run(gpu_ctx, _case("far_links", where))


@pytest.mark.parametrize("where", CB.COLUMN_CAP_WHERE)
def test_column_cap(gpu_ctx, where):
    """8261 rows: distances of 8191, 8192 and what would be 8193 in the column pass"""
    _run(gpu_ctx, _case("column_cap", where))


@pytest.mark.parametrize("rot", range(len(CB.ROW_STEP_COLS)))
@pytest.mark.parametrize("w", CB.ROW_STEP_W)
def test_row_steps(gpu_ctx, w, rot):
    """three rows (a dead wavefront), widths around 8, 16, 512 and 1024, zero columns on 0, 7 / 8, 511 / 512 and the last"""
    _run(gpu_ctx, _case("row_steps", w, rot))


@pytest.mark.parametrize("where", CB.LONE_WHERE)
def test_lone_zero_carries_over_three_step_edges(gpu_ctx, where):
    _run(gpu_ctx, _case("lone_zero", where))


@pytest.mark.parametrize("w", CB.LDS_W)
def test_lds_rows(gpu_ctx, w):
    """4, 2 and 1 rows per workgroup of the row pass (8193 and 16385: the first widths of the 2- and 1-row launches), 64 KB of LDS and
    the cap of the row pass at 32768"""
    _run(gpu_ctx, _case("lds_rows", w))


def test_unequal_batch(gpu_ctx):
    """700 x 3, 3 x 700, 1 x 1 and 520 x 130 in one blender: one grid for all, every image as the oracle has it alone"""
    _run(gpu_ctx, _case("unequal_batch"))


@pytest.mark.parametrize("surround", CB.VIEW_SURROUND)
@pytest.mark.parametrize("xoff", CB.VIEW_OFFSETS)
@pytest.mark.parametrize("density", CB.VIEW_DENSITY)
def test_views(gpu_ctx, density, xoff, surround):
    """the mask starts 1, 2, 3 bytes past a dword; zeros, or 255, lie all around it in its buffer"""
    _run(gpu_ctx, _case("views", density), views={0: (1234, surround, 4 + xoff)})


# ---------------------------------------------------------------------------------------------------------------------------------
# the gathers
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("as_views", (False, True))
@pytest.mark.parametrize("pano_w", CB.PLACE_PANO_W)
@pytest.mark.parametrize("dtype", (np.uint8, np.int16))
@pytest.mark.parametrize("kind", (CB.FEATHER, CB.NO))
def test_placement(gpu_ctx, kind, dtype, pano_w, as_views):
    """images 1 .. 8 wide starting on columns 0 .. 3 and 253 .. 257, as row 0 of buffers of their own and as views amid random bytes"""
    case = _case("placement", kind, dtype, pano_w)
    _run(gpu_ctx, case, views={k: ("random", "random", 5 + k % 4) for k in case[0].facts["small"]} if as_views else None)


def test_ones_path_one_lane_leaves_it(gpu_ctx):
    _run(gpu_ctx, _case("ones_path"))


@pytest.mark.parametrize("which", CB.WRAP_KINDS)
def test_accumulator_wrap(gpu_ctx, which):
    """140 x 255 on the integer path and 140 x 244 on the float path pass 32767, and so do two int16 images of 32767: wrap, not saturation"""
    _run(gpu_ctx, _case("accumulator_wrap", which))


def test_weight_sum_order(gpu_ctx):
    _run(gpu_ctx, _case("weight_sum_order"))


@pytest.mark.parametrize("dtype", (np.uint8, np.int16))
@pytest.mark.parametrize("grey", (0, 1))
def test_no_stack(gpu_ctx, grey, dtype):
    """the early exit one lane short of firing, firing, and kept from firing by grey masks that must OR to 7"""
    _run(gpu_ctx, _case("no_stack", grey, dtype))


# ---------------------------------------------------------------------------------------------------------------------------------
# the width limit
# ---------------------------------------------------------------------------------------------------------------------------------
def test_feather_refuses_an_image_wider_than_the_row_pass_can_hold(gpu_ctx):
    """32769 columns are refused at feed, by name of the limit; the blender then takes and blends a valid feed as if nothing had been"""
    w = CB.LDS_WIDTHS[2] + 1
    assert CB.rows_per_block(w) == 0
    wide = S.DeviceImage.from_numpy(np.zeros((1, w, 3), np.uint8), gpu_ctx), S.DeviceImage.from_numpy(np.full((1, w), 255, np.uint8), gpu_ctx)
    scene, want16, want8, wantm = _case("ones_path")
    b = _BlenderHandle(gpu_ctx, _lib.BLEND_FEATHER, 0, scene.sharpness, (0, 0, w, scene.roi[3]))
    with pytest.raises(S.StitchingError, match=r"\[-1\].*feather blender takes images up to %d columns wide, this one has %d" % (w - 1, w)):
        b.feed(wide[0], wide[1], (0, 0))
    for img, mask, corner in scene.feeds:
        b.feed(S.DeviceImage.from_numpy(img, gpu_ctx), S.DeviceImage.from_numpy(mask, gpu_ctx), corner)
    pano, mask, p16 = (d.numpy() for d in b.blend(want_s16=True))
    rh, rw = wantm.shape
    assert np.array_equal(p16[:rh, :rw], want16) and np.array_equal(pano[:rh, :rw], want8) and np.array_equal(mask[:rh, :rw], wantm)
    assert not mask[:, rw:].any() and not pano[:, rw:].any()
    # the "no" blender has no such limit
    n = _BlenderHandle(gpu_ctx, _lib.BLEND_NO, 0, 0.0, (0, 0, w, 1))
    n.feed(wide[0], wide[1], (0, 0))
    pano, mask = (d.numpy() for d in n.blend())
    assert mask.all() and not pano.any()
