"""The constructed multi-band families (tests/constructed_multiband.py) on the MI355X: every scene through the multi-band blender of the
C ABI (`_BlenderHandle`, as S.Blender drives it), the u8 panorama, its mask and the int16 panorama of blend(want_s16=True) against the
oracle's with 0 differing bytes, the inputs read back unmodified and the surroundings of pitched views unchanged.  Which path of the
kernels each scene reaches, that its facts hold, and that it tells the contract from a subtly wrong variant is asserted without a GPU in
tests/test_constructed_multiband.py; here only the device is asked — and, through the profiler's scope names and the replay counter,
whether the launches that classify() expects are the ones that ran."""
import ctypes as C
import functools

import numpy as np
import pytest

import stitching_amd as S
from oracle import oracle as O
from stitching_amd import _lib
from stitching_amd.blender import _BlenderHandle
from tests import constructed_multiband as CM

pytestmark = pytest.mark.gpu

MB_SCOPES = ("mb_down0", "mb_down", "mb_coarse", "mb_level", "mb_level0", "mb_level0_deferred")


@functools.lru_cache(maxsize=None)
def _case(builder, *args):
    """(scene, the oracle's int16 panorama, u8 panorama and mask): built once per case, never written to"""
    scene = getattr(CM, builder)(*args)
    b = O._OracleBlenderHandle(CM.MULTIBAND, scene.bands, 0.0)
    b.prepare(scene.roi)
    assert b.num_bands() == scene.B
    for img, mask, corner in scene.feeds:
        b.feed(np.asarray(img).astype(np.int16), mask, corner)
    out16, mask = b.blend()
    for a in (out16, mask):
        a.setflags(write=False)
    return scene, out16, O.convert_scale_abs(out16), mask


def _pitched(a, ctx, fill, xoff):
    """`a` as a view, `xoff` columns into a larger device buffer whose surroundings hold `fill` ("random": seeded bytes).
    -> (view, check): check() reads the whole buffer back and asserts that neither the view nor its surroundings changed"""
    shape = (a.shape[0] + 9, a.shape[1] + xoff + 13) + a.shape[2:]
    if isinstance(fill, str):
        big = np.random.default_rng(a.shape[1]).integers(1, 255, shape).astype(a.dtype)
    else:
        big = np.full(shape, fill, a.dtype)
    big[5:5 + a.shape[0], xoff:xoff + a.shape[1]] = a
    dev = S.DeviceImage.from_numpy(big, ctx)

    def check():
        assert np.array_equal(dev.numpy(), big), "a pitched buffer changed"

    return dev[5:5 + a.shape[0], xoff:xoff + a.shape[1]], check


def _plain(a, ctx):
    dev = S.DeviceImage.from_numpy(a, ctx)
    before = a.copy()

    def check():
        assert np.array_equal(dev.numpy(), before) and np.array_equal(a, before), "an input changed"

    return dev, check


def _upload(ctx, scene):
    """-> ([(device image, device mask, corner)], checks): one upload per distinct array; scene.pitched feeds as views"""
    up, checks = {}, []

    def dev(a, spec):
        key = (id(a), spec)
        if key not in up:
            up[key], check = _plain(a, ctx) if spec is None else _pitched(a, ctx, *spec)
            checks.append(check)
        return up[key]

    feeds = []
    for k, (img, mask, corner) in enumerate(scene.feeds):
        v = scene.pitched.get(k)
        feeds.append((dev(img, v and (v[0], v[2])), dev(mask, v and (v[1], v[2])), corner))
    return feeds, checks


def _replayed(ctx):
    n = C.c_int(-1)
    assert ctx._lib.stx_debug_blend_replayed(ctx.handle, C.byref(n)) == 0
    return n.value


def _blend(ctx, scene, feeds, keep=False, use=None, prof=False):
    """-> ((int16 panorama, u8 panorama, mask), kept weights, adopted, replaying launches, {scope: calls} of the multi-band scopes)"""
    b = _BlenderHandle(ctx, _lib.BLEND_MULTIBAND, scene.bands, 0.0, scene.roi)
    assert b.num_bands() == scene.B
    for img, mask, corner in feeds:
        b.feed(img, mask, corner)
    kept = b.keep_weights() if keep else None
    adopted = b.use_weights(use) if use is not None else False
    calls = None
    if prof:
        ctx.prof_enable(True)
        ctx.prof_reset()
    try:
        pano, mask, p16 = (d.numpy() for d in b.blend(want_s16=True))
        if prof:
            calls = {r["kernel"]: r["calls"] for r in ctx.prof_results() if r["kernel"] in MB_SCOPES and r["calls"]}
    finally:
        if prof:
            ctx.prof_enable(False)
    return (p16, pano, mask), kept, adopted, _replayed(ctx), calls


def _assert_bytes(got, case, what=""):
    _, want16, want8, wantm = case
    for name, g, w in (("int16 panorama", got[0], want16), ("u8 panorama", got[1], want8), ("mask", got[2], wantm)):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        diff = np.argwhere(g != w)
        assert len(diff) == 0, "%s %s: %d differing values, the first at %s: %s against the oracle's %s" % (
            what, name, len(diff), tuple(int(v) for v in diff[0]), g[tuple(diff[0])], w[tuple(diff[0])])


def _run(ctx, case, prof=False):
    scene = case[0]
    feeds, checks = _upload(ctx, scene)
    got, _, _, replayed, calls = _blend(ctx, scene, feeds, prof=prof)
    _assert_bytes(got, case)
    assert replayed == 0
    for check in checks:
        check()
    if prof:
        assert calls == CM.expected_launches(scene)[1], (calls, CM.expected_launches(scene)[0])


def _run_rig(ctx, case):
    """keeper, adopter (replays with at most 64 images) and adopter again: all three the oracle's bytes"""
    scene = case[0]
    feeds, checks = _upload(ctx, scene)
    a = _blend(ctx, scene, feeds, keep=True)
    assert a[1] is not None and a[3] == 0
    _assert_bytes(a[0], case, "keeper")
    want = CM.expected_launches(scene, adopted=True)
    for turn in ("first adopter", "second adopter"):
        b = _blend(ctx, scene, feeds, use=a[1], prof=True)
        assert b[2] is True
        _assert_bytes(b[0], case, turn)
        assert b[3] == want[2] == (scene.B - 2 if len(scene.feeds) <= CM.COVER_IMAGES else 0), (turn, b[3], want)
        assert b[4] == want[1], (turn, b[4], want)
    a[1].free()
    for check in checks:
        check()


# ---------------------------------------------------------------------------------------------------------------------------------
# the families
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", CM.WRAP_N)
def test_accumulator_wrap(gpu_ctx, n):
    """n copies over the same pixels: the packed int16 sums of mb_level0_pk_kernel and mb_level_pk_kernel pass +32767 and -32768"""
    _run(gpu_ctx, _case("accumulator_wrap", n))


def test_sums_exactly_on_the_ends_of_int16(gpu_ctx):
    """138 images whose level-0 sums are 32767, 32768 (wrapping to -32768) and -32768 at three pixels"""
    _run(gpu_ctx, _case("acc_extremes"), prof=True)


@pytest.mark.parametrize("s16", ("same", "big"))
def test_accumulator_wrap_with_an_int16_image(gpu_ctx, s16):
    """the same sums through the int accumulators and (short) casts of mb_level_kernel and mb_level_fast_kernel"""
    _run(gpu_ctx, _case("accumulator_wrap", 255, s16), prof=True)


@pytest.mark.parametrize("n", CM.COUNT_N)
def test_count_edges(gpu_ctx, n):
    """coverage counts 0, 1, 2, 3, 15, 16, 17 and n with every tier limit between every two pixels and the two rows of a lane's patch;
    n = 256 through the generic kernels"""
    _run(gpu_ctx, _case("count_edges", n), prof=True)


@pytest.mark.parametrize("n", (3, 17, 64, 65))
def test_count_edges_on_a_kept_rig(gpu_ctx, n):
    _run_rig(gpu_ctx, _case("count_edges", n))


@pytest.mark.parametrize("which,value", CM.GREY_CASES)
def test_grey_bytes(gpu_ctx, which, value):
    """single grey bytes under lanes 0 and 63, whole wavefronts, 64 and 65 queued patches, and masks that are binary without being
    declared so: mb_level0_deferred runs (possibly over an empty queue), the bytes are the oracle's"""
    _run(gpu_ctx, _case("grey_bytes", which, value), prof=True)


@pytest.mark.parametrize("which", ("lane63_px7", "n65", "views"))
def test_grey_bytes_on_a_kept_rig(gpu_ctx, which):
    _run_rig(gpu_ctx, _case("grey_bytes", which))


def test_grey_bytes_in_tile_columns_0_and_256_share_a_segment(gpu_ctx):
    """131088 columns: tile columns 0 and 256 queue into segment 0 of the deferral list"""
    _run(gpu_ctx, _case("grey_wide"), prof=True)


@pytest.mark.parametrize("grey", (False, True))
def test_down0_runs(gpu_ctx, grey):
    """images 1 .. 25 pixels wide and high at the corners that put an 11-pixel run on each side of every limit of dn_task_level0"""
    _run(gpu_ctx, _case("down0_runs", grey), prof=True)


@pytest.mark.parametrize("grey", (False, True))
def test_down0_batched(gpu_ctx, grey):
    """7 bands: tile columns of the level-0 pyrDown wholly in a border one mirror image away and wholly inside the image — the batched
    branch of mb_down0_lds_kernel, its mirrored byte picks and its own grey ballot"""
    _run(gpu_ctx, _case("down0_batched", grey), prof=True)


@pytest.mark.parametrize("grey", (False, True))
def test_down0_batched_on_a_kept_rig_build_no_weights(gpu_ctx, grey):
    _run_rig(gpu_ctx, _case("down0_batched", grey))


@pytest.mark.parametrize("grey", (False, True))
def test_down0_runs_on_a_kept_rig_build_no_weights(gpu_ctx, grey):
    """the WEIGHTS = false instantiations of the level-0 pyrDown"""
    _run_rig(gpu_ctx, _case("down0_runs", grey))


@pytest.mark.parametrize("builder,args", [("down0_runs", (False,)), ("down0_runs", (True,)), ("down0_batched", (False,)), ("down0_batched", (True,)), ("grey_bytes", ("run_bytes", 254)),
                                          ("occupancy_edges", (1040, "middle"))])
def test_weight_pyramids_level_by_level(gpu_ctx, builder, args):
    """every image's W_0 .. W_B read back through its exported contribution, bit for bit against pyrDown(CV_32F) of the bordered weight
    map: a pyrDown fault is named at its image and level instead of as a panorama difference"""
    from stitching_amd.distributed import make_shard_blender
    from tests.helpers import weight_pyramid_of_export as _weight_pyramid_of_export

    scene = _case(builder, *args)[0]
    feeds, checks = _upload(gpu_ctx, scene)
    b = make_shard_blender(gpu_ctx, scene.roi, scene.bands)
    assert b.num_bands() == scene.B
    for k, (img, mask, corner) in enumerate(feeds):
        b.feed_ex(img, mask, corner, k)
    for k, (_, mask, corner) in enumerate(scene.feeds):
        packed, rect = b.export_contrib(k, (0, scene.roi[2]))
        got = _weight_pyramid_of_export(packed, rect, scene.B)
        (fx, fy, fw, fh), (left, top) = CM.feed_rect(scene.B, scene.proi, mask.shape[1], mask.shape[0], corner)
        assert (rect[1], rect[3]) == (fy, fh) and fx <= rect[0] and rect[0] + rect[2] <= fx + fw
        W = np.zeros((fh, fw), np.float32)
        W[top:top + mask.shape[0], left:left + mask.shape[1]] = mask.astype(np.float32) * np.float32(1.0 / 255.0)
        want = [W]
        for _ in range(scene.B):
            want.append(O.pyr_down_32f(want[-1]))
        for i, (g_, o_) in enumerate(zip(got, want)):
            o_ = o_[:, (rect[0] - fx) >> i:(rect[0] - fx + rect[2]) >> i]
            assert g_.shape == o_.shape, (k, i, g_.shape, o_.shape)
            diff = np.argwhere(g_.view(np.uint32) != o_.view(np.uint32))
            assert len(diff) == 0, "image %d, W_%d: %d weights differ, the first at %s" % (k, i, len(diff), tuple(int(v) for v in diff[0]))
    for check in checks:
        check()


@pytest.mark.parametrize("w,bands", CM.UP_CASES)
def test_up_borders(gpu_ctx, w, bands):
    """panoramas 8, 16 and 40 columns wide as views amid seeded bytes: the first strip of a row is also its last, at level 0 and (16
    columns, 4 bands) at level 1 in mb_level_pk_kernel"""
    _run(gpu_ctx, _case("up_borders", w, bands), prof=True)


@pytest.mark.parametrize("zero_at", CM.OCC_ZERO_AT)
@pytest.mark.parametrize("w", CM.OCC_W)
def test_occupancy_edges(gpu_ctx, w, zero_at):
    """single mask pixels whose weights lie in the last column of an occupancy cell, the first of the next, and under the neighbouring
    tile; an all-zero image first, in the middle and last"""
    _run(gpu_ctx, _case("occupancy_edges", w, zero_at), prof=True)


@pytest.mark.parametrize("w", (520, 1040))
def test_occupancy_edges_on_a_kept_rig(gpu_ctx, w):
    _run_rig(gpu_ctx, _case("occupancy_edges", w, "middle"))


@pytest.mark.parametrize("which", CM.OVERSHOOT_CASES)
def test_collapse_overshoot(gpu_ctx, which):
    """taps of the finished coarser level on 500 and 501: the packed collapse and its 32-bit fallback, also in one plane alone"""
    _run(gpu_ctx, _case("collapse_overshoot", which), prof=True)


def test_feed_order(gpu_ctx):
    """six int16 images under grey masks everywhere: the fp32 weight sums in feed order"""
    _run(gpu_ctx, _case("feed_order"), prof=True)


@pytest.mark.parametrize("case", CM.LAUNCH_CASES)
def test_launch_matrix(gpu_ctx, case):
    """0 .. 5 bands, int16 and mixed images, grey masks, 256 images: the scopes that ran are the ones the host rules promise"""
    _run(gpu_ctx, _case("launch_matrix", case), prof=True)


@pytest.mark.parametrize("case", ("bands3", "bands5", "grey"))
def test_launch_matrix_on_a_kept_rig(gpu_ctx, case):
    _run_rig(gpu_ctx, _case("launch_matrix", case))


def test_an_int16_rig_keeps_nothing(gpu_ctx):
    """int16 images are not eligible for kept weights: no handle, no replay, the oracle's bytes"""
    case = _case("launch_matrix", "mixed_s16")
    feeds, _ = _upload(gpu_ctx, case[0])
    got, kept, _, replayed, _ = _blend(gpu_ctx, case[0], feeds, keep=True)
    assert kept is None and replayed == 0
    _assert_bytes(got, case)


@pytest.mark.parametrize("exchange", ("strips", "contribs"))
@pytest.mark.parametrize("case", CM.SHARDED_CASES)
def test_sharded(gpu_ctx, case, exchange):
    """two ranks in one process: received strips, exported and received contributions (the emit and contribution launches)"""
    from stitching_amd.distributed import owners_contiguous, virtual_sharded_blend

    scene, _, want8, wantm = _case("sharded", case)
    imgs, masks, corners = zip(*scene.feeds)
    sizes = [(m.shape[1], m.shape[0]) for m in masks]
    if case == "s16" and exchange == "strips":  # image strips are u8: an int16 image travels as a contribution or not at all
        with pytest.raises(S.StitchingError, match="strip: u8x3 image with a u8 mask of the same size"):
            virtual_sharded_blend(gpu_ctx, list(imgs), list(masks), list(corners), sizes, scene.facts["world"], scene.bands, exchange)
        return
    gpu_ctx.prof_enable(True)
    gpu_ctx.prof_reset()
    try:
        pano, mask, plan = virtual_sharded_blend(gpu_ctx, list(imgs), list(masks), list(corners), sizes, scene.facts["world"], scene.bands, exchange)
        calls = {r["kernel"]: r["calls"] for r in gpu_ctx.prof_results() if r["kernel"] in MB_SCOPES + ("mb_contrib",) and r["calls"]}
    finally:
        gpu_ctx.prof_enable(False)
    assert plan.num_bands == scene.B and len(plan.messages) >= 1
    for name, g, w in (("u8 panorama", pano, want8), ("mask", mask, wantm)):
        diff = np.argwhere(g != w)
        assert g.shape == w.shape and len(diff) == 0, "%s: %d differing bytes, the first at %s" % (name, len(diff), tuple(int(v) for v in diff[0]) if len(diff) else None)
    # the scopes of both ranks' blenders together: pyramids, exports ("mb_contrib": one batched export per message), gathers, deferral
    kernels, want = CM.expected_sharded(scene, owners_contiguous(len(imgs), scene.facts["world"]), plan.messages, exchange)
    assert calls == want, (calls, want, kernels)
