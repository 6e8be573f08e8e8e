"""The warp through the lens on the GPU (stx_warp_lens_batch, Warper.warp_images_through_lenses, StitchJob(lenses=), lens_mode="fused"):
the device equals tests/numpy_lens_warp.py byte for byte.  The contract takes the warp's fp32 backward map as an input; here it is the
device's own map (stx_debug_warp_maps, which tests/test_gpu_maps.py holds to the CPU checker's at 0 ULP), so that what is compared is the
sampler behind it.  All frames are 96 x 72 BGR (or smaller), focal 70 px, two or three cameras: the smallest shapes at which the kernel
takes each of its paths — more than one tile row in every ROI; more than one 256-pixel tile column only in a given rectangle, since
no ROI at this focal length is that wide.

Every test of this file fails without the feature (a missing export or keyword)."""
import ctypes as C
import math

import numpy as np
import pytest

import stitching_amd as S
from stitching_amd import _lib, config, synthetic
from stitching_amd.camera import CameraParams
from stitching_amd.pipeline import StitchJob, _LensWarper
from tests import numpy_lens_warp as LW
from tests import numpy_rectify as NR
from tests.test_gpu_maps import device_maps
from tests.test_rectify_contract import FISH, K as LENS_K, SRC, WIDE, image

pytestmark = pytest.mark.gpu
FOCAL = 70.0
STX_ERR_INVALID = -1
TABLED = ["plane", "affine", "cylindrical", "spherical", "mercator"]
GROUPS = ["fisheye", "compressedPlaneA2B1", "paniniPortraitA1.5B1", "transverseMercator"]  # one family per group of warp_general_kernel


def cameras(n, size, kind="spherical"):
    w, h = size
    if kind == "affine":  # R carries the affine map of the plane (K passes through)
        return [CameraParams(focal=FOCAL, aspect=1.0, ppx=w / 2.0, ppy=h / 2.0,
                             R=np.array([[1.0, 0.02 * (i + 1), 0.1 * i], [-0.02, 1.0 - 0.01 * i, 0.05], [0, 0, 1]], np.float32)) for i in range(n)]
    return [CameraParams(focal=FOCAL + i, aspect=1.0, ppx=w / 2.0 + 0.3 * i, ppy=h / 2.0,
                         R=(synthetic.rot_y(math.radians(-14.0 + 28.0 * i / max(n - 1, 1))) @ synthetic.rot_x(math.radians(2.5 * i - 3.0))).astype(np.float32))
            for i in range(n)]


def brown(dst_size=None):
    return S.LensMap.brown(LENS_K, WIDE, SRC, dst_size=dst_size)


def fisheye():
    return S.LensMap.fisheye(LENS_K, FISH, SRC, fit="inside")


def warper_for(ctx, kind, cams):
    w = S.Warper(kind, ctx=ctx)
    w.set_scale(cams)
    return w


def contract(ctx, warper, cam, host, lens, rect=None):
    """the contract on the device's own map over `rect` (None: the ROI of the rectified frame) -> (image, rectangle)"""
    xm, ym, roi = device_maps(ctx, warper.warper_type, warper.scale, S.Warper.get_K(cam), cam.R, lens.dst_size, 1, rect)
    return LW.lens_warp(host, lens.nodes, lens.dst_size, xm, ym), roi


def fused(ctx, warper, frames, lenses, cams, rects=None, tables=None):
    prev = config.device_resident()
    config.set_device_resident(True)
    try:
        imgs, rois = warper.warp_images_through_lenses(frames, lenses, cams, rects=rects, tables=tables)
    finally:
        config.set_device_resident(prev)
    return [np.asarray(i) for i in imgs], rois


def check(ctx, kind, hosts, lenses, frames=None, cams=None):
    cams = cams or cameras(len(hosts), lenses[0].dst_size, kind)
    warper = warper_for(ctx, kind, cams)
    got, rois = fused(ctx, warper, hosts if frames is None else frames, lenses, cams)
    assert rois == [warper.warp_roi(lens.dst_size, cam) for lens, cam in zip(lenses, cams)]
    for k, (host, lens, cam) in enumerate(zip(hosts, lenses, cams)):
        want, roi = contract(ctx, warper, cam, host, lens)
        assert roi == rois[k] and got[k].shape == want.shape and got[k].dtype == np.uint8
        assert np.array_equal(got[k], want), (kind, k, np.argwhere((got[k] != want).any(-1))[:4])
    return got, rois


# ---- 1: byte equality with the contract ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", TABLED + GROUPS)
def test_every_kernel_equals_the_contract_on_a_brown_and_a_fisheye_lens(gpu_ctx, kind):
    got, rois = check(gpu_ctx, kind, [image(SRC, 3, 21), image(SRC, 3, 22)], [brown(), fisheye()])
    assert all(r[3] > 16 for r in rois)  # more than one tile row of either kernel


def test_a_lens_whose_rectified_size_is_not_the_source_size(gpu_ctx):
    lens = brown(dst_size=(80, 60))
    assert lens.dst_size == (80, 60) and lens.src_size == SRC
    for kind in ("spherical", "fisheye"):
        check(gpu_ctx, kind, [image(SRC, 3, 23), image(SRC, 3, 24)], [lens, lens])


def test_a_crop_view_source_is_read_inside_its_rectangle_and_left_unchanged(gpu_ctx):
    """the view starts 5 pixels and 3 rows into its parent: an unaligned base and the parent's pitch"""
    parent = image((128, 90), 3, 25)
    dev = S.DeviceImage.from_numpy(parent, gpu_ctx)
    view = dev[3:3 + SRC[1], 5:5 + SRC[0]]
    assert view.stride_bytes == dev.stride_bytes != 3 * SRC[0] and view.device_ptr() % 4 != 0
    host = parent[3:3 + SRC[1], 5:5 + SRC[0]]
    check(gpu_ctx, "spherical", [host, host], [brown(), fisheye()], frames=[view, view])
    assert np.array_equal(dev.numpy(), parent)


def test_nine_images_of_unequal_sizes_go_in_two_groups(gpu_ctx):
    sizes = [(96, 72), (80, 60), (53, 41), (64, 48), (96, 72), (33, 70), (70, 33), (17, 19), (96, 72)]
    lenses = [S.LensMap.brown(np.array([[FOCAL, 0, w / 2.0], [0, FOCAL, h / 2.0], [0, 0, 1.0]]), WIDE, (w, h)) for w, h in sizes]
    hosts = [image(z, 3, 30 + k) for k, z in enumerate(sizes)]
    cams = [CameraParams(focal=FOCAL, aspect=1.0, ppx=w / 2.0, ppy=h / 2.0,
                         R=(synthetic.rot_y(math.radians(-20.0 + 5.0 * k)) @ synthetic.rot_x(math.radians(k - 4.0))).astype(np.float32))
            for k, (w, h) in enumerate(sizes)]
    for kind in ("spherical", "plane"):
        check(gpu_ctx, kind, hosts, lenses, cams=cams)


# ---- 2: rectangles ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["spherical", "cylindrical", "compressedPlaneA2B1"])
def test_rectangles_equal_the_whole_warp_cut(gpu_ctx, kind):
    hosts, lenses = [image(SRC, 3, 41), image(SRC, 3, 42), image(SRC, 3, 43)], [brown(), fisheye(), brown()]
    cams = cameras(3, SRC, kind)
    warper = warper_for(gpu_ctx, kind, cams)
    whole, rois = fused(gpu_ctx, warper, hosts, lenses, cams)
    # x offsets and widths that are no multiples of 4 (the last lane of a row), heights that are no multiples of either tile; 1 x 1
    cuts = [(3, 5, 41, 23), (1, 0, 1, 1), (6, 17, 30, 17)]
    rects = [(r[0] + c[0], r[1] + c[1], c[2], c[3]) for r, c in zip(rois, cuts)]
    assert all(c[0] + c[2] <= r[2] and c[1] + c[3] <= r[3] for r, c in zip(rois, cuts))
    got, out = fused(gpu_ctx, warper, hosts, lenses, cams, rects=rects)
    assert out == rects
    for k, (c, host, lens, cam) in enumerate(zip(cuts, hosts, lenses, cams)):
        assert got[k].shape == (c[3], c[2], 3)
        assert np.array_equal(got[k], whole[k][c[1]:c[1] + c[3], c[0]:c[0] + c[2]]), (kind, k)
        assert np.array_equal(got[k], contract(gpu_ctx, warper, cam, host, lens, rects[k])[0]), (kind, k)
    # a rectangle that leaves the ROI on every side: positions far outside the rectified frame
    wide = (rois[0][0] - 9, rois[0][1] - 7, rois[0][2] + 21, rois[0][3] + 13)
    got, _ = fused(gpu_ctx, warper, hosts[:1], lenses[:1], cams[:1], rects=[wide])
    assert np.array_equal(got[0], contract(gpu_ctx, warper, cams[0], hosts[0], lenses[0], wide)[0])
    # wider than one 256-pixel tile: a second block along x, whose last lane is a tail lane too (no ROI of these cameras is that wide)
    long = (rois[0][0] - 90, rois[0][1] + 11, 301, 9)
    got, _ = fused(gpu_ctx, warper, hosts[:1], lenses[:1], cams[:1], rects=[long])
    assert got[0].shape == (9, 301, 3)
    assert np.array_equal(got[0], contract(gpu_ctx, warper, cams[0], hosts[0], lenses[0], long)[0])


# ---- 3: an identity lens is the existing warp ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["spherical", "plane", "stereographic"])
def test_identity_lens_equals_the_batched_warp_under_the_mask(gpu_ctx, kind):
    ident = S.LensMap(NR.quantise(*NR.node_pixels(*SRC)), SRC, SRC)
    hosts = [image(SRC, 3, 51), image(SRC, 3, 52)]
    cams = cameras(2, SRC, kind)
    warper = warper_for(gpu_ctx, kind, cams)
    got, rois = fused(gpu_ctx, warper, hosts, [ident, ident], cams)
    want, masks, wrois = warper.warp_images_and_masks(hosts, cams)
    assert rois == wrois
    for g, w, m in zip(got, want, masks):
        under = np.asarray(m) != 0
        assert under.any() and np.array_equal(g[under], np.asarray(w)[under])


# ---- 4: nodes that point far outside the source -------------------------------------------------------------------------------------------
def test_nodes_far_outside_the_source_give_clamped_taps(gpu_ctx):
    nx, ny = NR.node_counts(*SRC)
    i, j = np.meshgrid(np.arange(nx), np.arange(ny))
    nodes = np.empty((ny, nx, 2), np.int32)
    nodes[..., 0] = np.where((i + j) % 3 == 0, NR.Q6_MIN, np.where((i + j) % 3 == 1, NR.Q6_MAX, 64 * 16 * i))
    nodes[..., 1] = np.where((i + 2 * j) % 3 == 0, NR.Q6_MAX, np.where((i + 2 * j) % 3 == 1, 64 * 16 * j, NR.Q6_MIN))
    lens = S.LensMap(nodes, SRC, SRC)
    check(gpu_ctx, "spherical", [image(SRC, 3, 61), image(SRC, 3, 62)], [lens, lens])
    check(gpu_ctx, "paniniA2B1", [image(SRC, 3, 61), image(SRC, 3, 62)], [lens, lens])


# ---- 5 - 7: StitchJob(lenses=) ------------------------------------------------------------------------------------------------------------
def table_launches(ctx):
    n = C.c_int(-1)
    assert ctx._lib.stx_debug_warp_table_launches(ctx.handle, C.byref(n)) == 0
    return n.value


def rig(seed=70, n=3):
    lenses = [brown(), fisheye(), brown()][:n]
    return [image(SRC, 3, seed + k) for k in range(n)], lenses, cameras(n, SRC)


@pytest.mark.parametrize("blender,bands", [("multiband", 2), ("feather", None), ("no", None)])
def test_job_with_lenses(gpu_ctx, oracle, blender, bands):
    hosts, lenses, cams = rig()
    nxt = [image(SRC, 3, 80 + k) for k in range(3)]
    kw = dict(warper_type="spherical", blender_type=blender, num_bands=bands, ctx=gpu_ctx)
    job = StitchJob(hosts, cams, lenses=lenses, **kw)
    pano, pmask = (np.asarray(a) for a in job.run())
    # the masks: those of a job over rectified frames, with and without the lens's validity masks
    rect, lens_masks = S.rectify_all(hosts, lenses, masks=True, ctx=gpu_ctx)
    plain = StitchJob(rect, cams, **kw)
    assert np.array_equal(np.asarray(plain.run()[1]), pmask)
    assert job.corners == plain.corners and job.warped_sizes == plain.warped_sizes
    own = [np.asarray(m) for m in lens_masks]
    want_mask = np.asarray(StitchJob(rect, cams, source_masks=own, **kw).run()[1])
    assert np.array_equal(np.asarray(StitchJob(hosts, cams, lenses=lenses, source_masks="lens", **kw).run()[1]), want_mask)
    assert np.array_equal(np.asarray(StitchJob(hosts, cams, lenses=lenses, source_masks=own, **kw).run()[1]), want_mask)
    with pytest.raises(S.StitchingError, match="with lenses"):
        StitchJob(rect, cams, source_masks="lens", **kw)
    # the panorama: the oracle's blend of the contract's warped images
    warper = warper_for(gpu_ctx, "spherical", cams)
    _, wmasks, rois = warper.warp_images_and_masks(rect, cams)
    ob = oracle.Blender(blender, job.blend_strength)
    ob.prepare([r[0:2] for r in rois], [r[2:4] for r in rois])
    for host, lens, cam, m, r in zip(hosts, lenses, cams, wmasks, rois):
        ob.feed(contract(gpu_ctx, warper, cam, host, lens)[0], np.asarray(m), r[0:2])
    opano, omask = ob.blend()
    assert np.array_equal(pmask, omask) and np.array_equal(pano, opano)
    # the next panorama of the rig: no table kernel, the bytes of a fresh job
    pano2, pmask2 = (np.asarray(a) for a in job.run(frames=nxt))
    assert job.last_reused
    fresh = StitchJob(nxt, cams, lenses=lenses, **kw)
    fpano, fmask = (np.asarray(a) for a in fresh.run())
    assert np.array_equal(pano2, fpano) and np.array_equal(pmask2, fmask) and not np.array_equal(pano2, pano)
    job.run(frames=hosts)
    assert table_launches(gpu_ctx) == 0
    # another lens is another rig
    other = StitchJob(hosts, cams, lenses=[fisheye(), fisheye(), fisheye()], **kw)
    assert other.geometry_key() != job.geometry_key()


@pytest.mark.parametrize("ctype", ["gain_blocks", "gain"])
def test_job_gains_equal_apply_on_the_ungained_fused_warp(gpu_ctx, ctype):
    hosts, lenses, cams = rig(90)
    warper = warper_for(gpu_ctx, "spherical", cams)
    plain, rois = fused(gpu_ctx, warper, hosts, lenses, cams)
    comp = S.ExposureErrorCompensator(ctype, 1, 32)
    rng = np.random.default_rng(5)
    if ctype == "gain":
        comp.set_gains([np.array([g]) for g in (0.8, 1.1, 1.3)])
    else:
        comp.set_gains([(0.7 + 0.6 * rng.random((-(-r[3] // 32), -(-r[2] // 32)))).astype(np.float32) for r in rois])
    want = [np.asarray(a) for a in comp.apply_all([r[0:2] for r in rois], [p.copy() for p in plain], None, ctx=gpu_ctx)]
    assert any(not np.array_equal(w, p) for w, p in zip(want, plain))
    lw = _LensWarper(warper, lenses, None)
    prev = config.device_resident()
    config.set_device_resident(True)
    try:
        got, _, out = lw.warp_images_and_masks(hosts, cams, compensator=comp, masks=False, rects=rois)
        cut = [(r[0] + 5, r[1] + 9, 37, 22) for r in rois]
        part, _, _ = lw.warp_images_and_masks(hosts, cams, compensator=comp, masks=False, rects=cut)
    finally:
        config.set_device_resident(prev)
    for g, w, p in zip(got, want, part):
        assert np.array_equal(np.asarray(g), w)
        assert np.array_equal(np.asarray(p), w[9:31, 5:42])
    # and through the job: the panorama of a job with the compensator is the blend of these images
    a = StitchJob(hosts, cams, lenses=lenses, blender_type="no", compensator=comp, ctx=gpu_ctx).run()
    b = StitchJob(hosts, cams, lenses=lenses, blender_type="no", ctx=gpu_ctx).run()
    assert not np.array_equal(np.asarray(a[0]), np.asarray(b[0])) and np.array_equal(np.asarray(a[1]), np.asarray(b[1]))


def test_job_with_a_cropper_equals_the_uncropped_fused_warp_cut(gpu_ctx, oracle):
    hosts, lenses, cams = rig(100)
    warper = warper_for(gpu_ctx, "spherical", cams)
    whole, rois = fused(gpu_ctx, warper, hosts, lenses, cams)
    rect = S.rectify_all(hosts, lenses, ctx=gpu_ctx)
    wmasks = [np.asarray(m) for m in warper.warp_images_and_masks(rect, cams)[1]]
    corners, sizes = [r[0:2] for r in rois], [r[2:4] for r in rois]
    cropper = S.Cropper(True)
    cropper.prepare(whole, wmasks, corners, sizes)
    job = StitchJob(hosts, cams, lenses=lenses, blender_type="no", cropper=cropper, ctx=gpu_ctx)
    pano, pmask = (np.asarray(a) for a in job.run())
    # warp whole, cut, feed: the reference's order, on the uncropped fused warp
    ccorners, csizes = cropper.crop_rois(corners, sizes)
    ob = oracle.Blender("no", job.blend_strength)
    ob.prepare(ccorners, csizes)
    for img, mask, corner in zip(cropper.crop_images(whole), cropper.crop_images(wmasks), ccorners):
        ob.feed(np.ascontiguousarray(img), np.ascontiguousarray(mask), corner)
    opano, omask = ob.blend()
    assert np.array_equal(pmask, omask) and np.array_equal(pano, opano)
    pano2, _ = job.run(frames=hosts)
    assert job.last_reused and np.array_equal(np.asarray(pano2), pano)


# ---- 8: Composer ------------------------------------------------------------------------------------------------------------------------
def test_composer_fused_runs_end_to_end_with_the_masks_of_rectify(gpu_ctx, monkeypatch):
    """96 x 72 frames are below every megapixel setting: MEDIUM, LOW and FINAL are the frames' own size, the cameras' scale"""
    hosts, lenses, cams = rig(130)
    kw = dict(finder="voronoi", ctx=gpu_ctx)
    comp = S.Composer(**kw)
    plan = comp.prepare(hosts, cams, lenses=lenses, lens_mode="fused")
    assert plan.lenses == lenses and len(plan.distorted) == 3 and [f.shape for f in plan.distorted] == [h.shape for h in hosts]
    pano, mask = (np.asarray(a) for a in comp.run(plan))
    comp_r = S.Composer(**kw)
    pano_r, mask_r = (np.asarray(a) for a in comp_r.run(comp_r.prepare(hosts, cams, lenses=lenses)))
    assert np.array_equal(mask, mask_r) and pano.shape == pano_r.shape and not np.array_equal(pano, pano_r)
    assert np.array_equal(np.asarray(S.Composer(**kw).compose(hosts, cams, lenses=lenses, lens_mode="fused")), pano)
    # the next distorted frames on the plan: the job's second run, pixels only
    nxt = [image(SRC, 3, 140 + k) for k in range(3)]
    pano2, mask2 = (np.asarray(a) for a in comp.run(plan, images=nxt, lenses=lenses))
    assert plan.job.last_reused and np.array_equal(mask2, mask) and not np.array_equal(pano2, pano)
    with pytest.raises(S.StitchingError, match="with their lenses"):
        comp.run(plan, images=nxt)
    # the lens's own validity masks, in both modes
    a = S.Composer(**kw)
    b = S.Composer(**kw)
    ma = np.asarray(a.run(a.prepare(hosts, cams, lenses=lenses, source_masks="lens", lens_mode="fused"))[1])
    mb = np.asarray(b.run(b.prepare(hosts, cams, lenses=lenses, source_masks="lens"))[1])
    assert np.array_equal(ma, mb)
    # "rectify" and no lenses take none of the new paths: with those booby-trapped they give what they gave

    def trap(*args, **kwargs):
        raise AssertionError("the rectify mode reached the warp through the lens")

    monkeypatch.setattr(S.Warper, "warp_images_through_lenses", trap)
    monkeypatch.setattr(_LensWarper, "__init__", trap)
    assert np.array_equal(np.asarray(S.Composer(**kw).compose(hosts, cams, lenses=lenses)), pano_r)
    assert np.array_equal(np.asarray(S.Composer(**kw).compose(hosts, cams, lenses=lenses, lens_mode="rectify")), pano_r)
    S.Composer(**kw).compose(hosts, cams)
    with pytest.raises(AssertionError, match="reached the warp through the lens"):
        S.Composer(**kw).compose(hosts, cams, lenses=lenses, lens_mode="fused")


# ---- 9: refusals of the C entry -----------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_context_usable(gpu_ctx):
    ctx, L = gpu_ctx, gpu_ctx._lib
    hosts, lenses, cams = rig(110, 2)
    warper = warper_for(ctx, "spherical", cams)
    before = [np.asarray(a) for a in warper.warp_images_and_masks(hosts, cams)[0]]
    Ks, Rs = warper.camera_arrays(cams)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    dev = [S.DeviceImage.from_numpy(h, ctx) for h in hosts]
    gray, small = S.DeviceImage.from_numpy(image(SRC, 1, 1), ctx), S.DeviceImage.from_numpy(image((80, 60), 3, 2), ctx)
    other = S.Context(0)
    foreign_img, foreign_lens = S.DeviceImage.from_numpy(hosts[0], other), brown()
    maps = [lens.handle(ctx).value for lens in lenses]
    wide = S.DeviceImage.from_numpy(np.zeros((2, (1 << 24) // 3 + 40, 3), np.uint8), ctx)
    wide_view = wide[0:2, 0:SRC[0]]  # a view of a very wide parent: its pitch is 2^24 or more
    assert wide_view.stride_bytes >= 1 << 24
    thin = S.LensMap.brown(np.array([[FOCAL, 0, 48.0], [0, FOCAL, 1.0], [0, 0, 1.0]]), (0.0, 0.0, 0.0, 0.0), (SRC[0], 2))

    def call(srcs=None, lens_handles=None, rects=None, out=True, n=2, ctx_h=ctx.handle, Kp=True):
        srcs = [d._h.value for d in dev] if srcs is None else srcs
        lens_handles = maps if lens_handles is None else lens_handles
        o = (C.c_void_p * 2)()
        r = None if rects is None else np.ascontiguousarray(rects, np.int32)
        rc = L.stx_warp_lens_batch(ctx_h, _lib.WARP_TYPE_IDS["spherical"], float(warper.scale), n, Ks.ctypes.data_as(fp) if Kp else None,
                                   Rs.ctypes.data_as(fp), (C.c_void_p * 2)(*srcs), (C.c_void_p * 2)(*lens_handles),
                                   None if r is None else r.ctypes.data_as(ip), o if out else None, None, None)
        assert o[0] is None and o[1] is None or rc == 0
        return rc

    ok = [(10, 10, 20, 20), (10, 10, 20, 20)]
    refused = {
        "null context": lambda: call(ctx_h=None),
        "null cameras": lambda: call(Kp=False),
        "null outputs": lambda: call(out=False),
        "null image handle": lambda: call(srcs=[dev[0]._h.value, None]),
        "null lens handle": lambda: call(lens_handles=[maps[0], None]),
        "not u8x3": lambda: call(srcs=[dev[0]._h.value, gray._h.value]),
        "not the map's source size": lambda: call(srcs=[dev[0]._h.value, small._h.value]),
        "image of another context": lambda: call(srcs=[foreign_img._h.value, dev[1]._h.value]),
        "map of another context": lambda: call(lens_handles=[foreign_lens.handle(other).value, maps[1]]),
        "pitch of 2^24": lambda: call(srcs=[wide_view._h.value, dev[1]._h.value], lens_handles=[thin.handle(ctx).value, maps[1]]),
        "zero width": lambda: call(rects=[ok[0], (10, 10, 0, 20)]),
        "negative height": lambda: call(rects=[(10, 10, 20, -3), ok[1]]),
    }
    for what, fn in refused.items():
        assert fn() == STX_ERR_INVALID, what
        assert L.stx_last_error()
    prev = config.remap_mode()
    config.set_remap_mode("float")
    try:
        assert call() == STX_ERR_INVALID
    finally:
        config.set_remap_mode(prev)
    after = [np.asarray(a) for a in warper.warp_images_and_masks(hosts, cams)[0]]
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    del refused, foreign_img  # what lives on the other context goes before it does
    foreign_lens.release()
    other.close()


def test_trig_mode_is_honoured(gpu_ctx):
    prev = config.trig_mode()
    config.set_trig_mode("glibc")
    try:
        check(gpu_ctx, "spherical", [image(SRC, 3, 120), image(SRC, 3, 121)], [brown(), fisheye()])
    finally:
        config.set_trig_mode(prev)
