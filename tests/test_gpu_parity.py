"""GPU parity: HIP path (through the C ABI) vs the CPU oracle on the same seeded inputs.
Bar: bit-exact on u8 / int16 / int ROI; fp32 warp coordinates are never stored by the HIP path,
so they are checked through the 1/32-px quantised samples they produce (also bit-exact)."""
import numpy as np
import pytest

import stitching_amd as S
from stitching_amd import synthetic
from tests import helpers

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("wtype", ["spherical", "cylindrical", "plane"])
def test_warp_roi_matches_oracle(oracle, gpu_ctx, wtype):
    cams = synthetic.ring_cameras(5, 640, 480, span_deg=150.0 if wtype != "plane" else 60.0)
    g = S.Warper(wtype)
    o = oracle.Warper(wtype)
    g.set_scale(cams)
    o.set_scale(cams)
    sizes = [(640, 480)] * len(cams)
    assert g.warp_rois(sizes, cams) == o.warp_rois(sizes, cams)
    for cam in cams:
        assert g.warp_roi((640, 480), cam) == o.warp_roi((640, 480), cam)
        assert g.warp_roi((640, 480), cam, 0.37) == o.warp_roi((640, 480), cam, 0.37)


@pytest.mark.parametrize("wtype", ["spherical", "cylindrical", "plane"])
def test_warp_image_and_mask_bit_exact(oracle, gpu_ctx, wtype):
    imgs, cams = helpers.small_ring(4, 517, 389, span=140.0 if wtype != "plane" else 50.0)
    g = S.Warper(wtype)
    o = oracle.Warper(wtype)
    g.set_scale(cams)
    o.set_scale(cams)
    for img, cam in zip(imgs, cams):
        gi, oi = g.warp_image(img, cam), o.warp_image(img, cam)
        assert gi.shape == oi.shape
        assert np.array_equal(gi, oi), f"{np.count_nonzero(gi != oi)} differing bytes"
        gm, om = g.create_and_warp_mask((517, 389), cam), o.create_and_warp_mask((517, 389), cam)
        assert np.array_equal(gm, om)
        fi, fm, roi = g.warp_image_and_mask(img, cam)
        assert np.array_equal(fi, oi) and np.array_equal(fm, om)
        assert roi == o.warp_roi((517, 389), cam)


@pytest.mark.parametrize("wtype", ["spherical", "cylindrical", "plane", "fisheye"])
def test_roi_pass_and_warps_in_one_call(oracle, gpu_ctx, wtype):
    """stx_warp_batch with STX_WARP_FRESH_ROIS (the ROI pass polled from pinned memory, the warps launched behind it) == the oracle's rois, images,
    masks — twice, the second time with every ROI already in the cache of earlier calls (the pass must run again and agree)."""
    imgs, cams = helpers.small_ring(5, 431, 297, span=130.0 if wtype not in ("plane", "fisheye") else 50.0)
    g, o = S.Warper(wtype), oracle.Warper(wtype)
    g.set_scale(cams)
    o.set_scale(cams)
    want = [(o.warp_image(im, c), o.create_and_warp_mask((431, 297), c), o.warp_roi((431, 297), c)) for im, c in zip(imgs, cams)]
    ka = g.camera_arrays(cams)
    for _ in range(2):
        gi, gm, rois = g.warp_images_and_masks(imgs, cams, with_rois=True, camera_arrays=ka)
        assert rois == [w[2] for w in want]
        for a, b, w in zip(gi, gm, want):
            assert np.array_equal(a, w[0]) and np.array_equal(b, w[1])


def test_affine_warp_bit_exact(oracle, gpu_ctx):
    cams = synthetic.affine_scan_cameras(4, 300, 200)
    imgs = [synthetic.make_frame(i, 300, 200) for i in range(4)]
    g, o = S.Warper("affine"), oracle.Warper("affine")
    g.set_scale(cams)
    o.set_scale(cams)
    for img, cam in zip(imgs, cams):
        assert g.warp_roi((300, 200), cam) == o.warp_roi((300, 200), cam)
        assert np.array_equal(g.warp_image(img, cam), o.warp_image(img, cam))
        assert np.array_equal(g.create_and_warp_mask((300, 200), cam), o.create_and_warp_mask((300, 200), cam))


@pytest.mark.parametrize("aspect", [0.4, 2.5])
def test_affine_warp_at_another_resolution(oracle, gpu_ctx, aspect):
    """AffineStitcher warps low-res and final-res images with K and the warper scale multiplied by `aspect`
    (stitching/warper.py:44,59,80,86-93); cv::AffineWarper keeps that scale (detail::AffineWarper(scale))."""
    cams = synthetic.affine_scan_cameras(4, 300, 200)
    w, h = int(round(300 * aspect)), int(round(200 * aspect))
    imgs = [synthetic.make_frame(10 + i, w, h) for i in range(4)]
    g, o = S.Warper("affine"), oracle.Warper("affine")
    g.set_scale(cams)
    o.set_scale(cams)
    for img, cam in zip(imgs, cams):
        assert g.warp_roi((w, h), cam, aspect) == o.warp_roi((w, h), cam, aspect)
        assert np.array_equal(g.warp_image(img, cam, aspect), o.warp_image(img, cam, aspect))
        assert np.array_equal(g.create_and_warp_mask((w, h), cam, aspect), o.create_and_warp_mask((w, h), cam, aspect))
    # the tiles land `aspect` times as far apart as at the registration resolution
    c1, _ = o.warp_rois([(300, 200)] * 4, cams)
    ca, _ = o.warp_rois([(w, h)] * 4, cams, aspect)
    for (x1, y1), (xa, ya) in zip(c1, ca):
        assert abs(xa - x1 * aspect) <= 2 and abs(ya - y1 * aspect) <= 2


@pytest.mark.parametrize("btype,strength", [("multiband", 5), ("multiband", 20), ("feather", 5), ("no", 5)])
def test_blend_bit_exact(oracle, gpu_ctx, btype, strength):
    imgs, cams = helpers.small_ring(4, 400, 300, span=160.0)
    g = helpers.run_pipeline(S.Warper, S.Blender, imgs, cams, blender_type=btype, blend_strength=strength)
    o = helpers.run_pipeline(oracle.Warper, oracle.Blender, imgs, cams, blender_type=btype, blend_strength=strength)
    assert g["corners"] == o["corners"] and g["sizes"] == o["sizes"]
    assert g["pano"].shape == o["pano"].shape
    assert np.array_equal(g["pmask"], o["pmask"])
    d = np.abs(g["pano"].astype(int) - o["pano"].astype(int))
    assert d.max() == 0, f"max diff {d.max()}, {np.count_nonzero(d)} bytes differ"


def test_blend_voronoi_masks_bit_exact(oracle, gpu_ctx):
    imgs, cams = helpers.small_ring(5, 400, 300, span=180.0)
    g = helpers.run_pipeline(S.Warper, S.Blender, imgs, cams, blend_strength=10, masks_fn=synthetic.voronoi_seam_masks)
    o = helpers.run_pipeline(oracle.Warper, oracle.Blender, imgs, cams, blend_strength=10,
                             masks_fn=synthetic.voronoi_seam_masks)
    assert np.array_equal(g["pmask"], o["pmask"])
    assert np.array_equal(g["pano"], o["pano"])


def test_blend_int16_input_and_int16_result(oracle, gpu_ctx):
    """stitching/blender.py:41 feeds int16; values outside 0..255 (e.g. after exposure gain) must
    follow the int16 path bit-exactly; stx_blend_finish_ex also returns blender.blend()'s int16."""
    import ctypes as C

    from stitching_amd import _lib
    from stitching_amd.device import DeviceImage

    imgs, cams = helpers.small_ring(3, 333, 251, span=110.0)
    ow, gw = oracle.Warper("spherical"), S.Warper("spherical")
    ow.set_scale(cams)
    gw.set_scale(cams)
    sizes = [(333, 251)] * 3
    wi = [ow.warp_image(i, c).astype(np.int16) * 3 - 200 for i, c in zip(imgs, cams)]
    wm = [ow.create_and_warp_mask(s, c) for s, c in zip(sizes, cams)]
    corners, wsz = ow.warp_rois(sizes, cams)
    ob, gb = oracle.Blender("multiband", 15), S.Blender("multiband", 15)
    ob.prepare(corners, wsz)
    gb.prepare(corners, wsz)
    for a, m, c in zip(wi, wm, corners):
        ob.blender.feed(a, m, c)
        gb.feed(a, m, c)
    o16, omask = ob.blender.blend()
    pano, mask, p16 = gb.blender.blend(want_s16=True)
    assert np.array_equal(np.asarray(mask), omask)
    assert np.array_equal(np.asarray(p16), o16)
    assert np.array_equal(np.asarray(pano), oracle.convert_scale_abs(o16))


@pytest.mark.parametrize("strength,n", [(15, 4), (40, 5)])
def test_blend_mixed_u8_and_int16_images(oracle, gpu_ctx, strength, n):
    """One blender fed u8 AND int16 images: the Gaussian pyramid of a u8 image is stored as bytes, that of an int16 image as
    int16 (StxMbImage::g_u8, round 3) — the gather kernels take a wave-uniform branch per image.  int16 images with values
    outside 0..255, u8 images as the warper returns them; every level kernel (generic, register-blocked, coarse fusion)."""
    imgs, cams = helpers.small_ring(n, 517, 389, span=35.0 * n)
    ow = oracle.Warper("spherical")
    ow.set_scale(cams)
    sizes = [(517, 389)] * n
    wu8 = [ow.warp_image(i, c) for i, c in zip(imgs, cams)]
    wm = [ow.create_and_warp_mask(s, c) for s, c in zip(sizes, cams)]
    corners, wsz = ow.warp_rois(sizes, cams)
    fed = [w if k % 2 == 0 else (w.astype(np.int16) * 2 - 100) for k, w in enumerate(wu8)]  # even: u8, odd: int16 beyond 0..255
    ob, gb = oracle.Blender("multiband", strength), S.Blender("multiband", strength)
    ob.prepare(corners, wsz)
    gb.prepare(corners, wsz)
    for a, m, c in zip(fed, wm, corners):
        ob.blender.feed(a.astype(np.int16), m, c)
        gb.feed(a, m, c)
    assert gb.blender.num_bands() == ob.blender.num_bands() >= 3
    o16, omask = ob.blender.blend()
    pano, mask, p16 = gb.blender.blend(want_s16=True)
    assert np.array_equal(np.asarray(mask), omask)
    assert np.array_equal(np.asarray(p16), o16)
    assert np.array_equal(np.asarray(pano), oracle.convert_scale_abs(o16))


@pytest.mark.parametrize("wtype,strength", [("spherical", 30), ("cylindrical", 12)])
def test_blend_larger_odd_sizes(oracle, gpu_ctx, wtype, strength):
    """Sizes that are not multiples of anything, 5-6 bands: exercises the register-blocked kernels
    (levels <= B-3), the generic coarse-level kernels and every border path."""
    imgs, cams = helpers.small_ring(3, 1203, 907, span=120.0)
    g = helpers.run_pipeline(S.Warper, S.Blender, imgs, cams, warper_type=wtype, blend_strength=strength)
    o = helpers.run_pipeline(oracle.Warper, oracle.Blender, imgs, cams, warper_type=wtype, blend_strength=strength)
    assert g["blender"].blender.num_bands() == o["blender"].blender.num_bands() >= 5
    assert np.array_equal(g["pmask"], o["pmask"])
    d = g["pano"].astype(int) - o["pano"].astype(int)
    assert not d.any(), f"{np.count_nonzero(d)} bytes differ, max {np.abs(d).max()}"


def test_device_resident_views_and_feed(oracle, gpu_ctx):
    """DeviceImage slicing (stitching/cropper.py:150-151 on device) and device-resident feed."""
    imgs, cams = helpers.small_ring(2, 400, 300, span=60.0)
    S.set_device_resident(True)
    try:
        w = S.Warper()
        w.set_scale(cams)
        d = w.warp_image(imgs[0], cams[0])
        assert isinstance(d, S.DeviceImage) and d.dtype == np.uint8
        host = d.numpy()
        v = d[10:200, 33:301]
        assert isinstance(v, S.DeviceImage) and v.shape == (190, 268, 3)
        assert np.array_equal(np.asarray(v), host[10:200, 33:301])
        m = w.create_and_warp_mask((400, 300), cams[0])
        b = S.Blender("multiband", 10)
        b.prepare([(0, 0)], [(268, 190)])
        b.feed(v, m[10:200, 33:301], (0, 0))
        pano, pm = b.blend()
        ob = oracle.Blender("multiband", 10)
        ob.prepare([(0, 0)], [(268, 190)])
        ob.feed(host[10:200, 33:301], np.asarray(m)[10:200, 33:301], (0, 0))
        op, om = ob.blend()
        assert np.array_equal(np.asarray(pano), op) and np.array_equal(np.asarray(pm), om)
    finally:
        S.set_device_resident(False)


def test_error_paths(gpu_ctx):
    b = S.Blender("multiband")
    b.prepare([(0, 0)], [(64, 64)])
    with pytest.raises(S.StitchingError):  # image leaves the prepared roi
        b.feed(np.zeros((64, 64, 3), np.uint8), np.zeros((64, 64), np.uint8), (10, 0))
    with pytest.raises(S.StitchingError):  # mask / image size mismatch
        b.feed(np.zeros((64, 64, 3), np.uint8), np.zeros((32, 64), np.uint8), (0, 0))
    b.feed(np.zeros((64, 64, 3), np.uint8), np.full((64, 64), 255, np.uint8), (0, 0))
    b.blend()
    with pytest.raises(S.StitchingError):  # blend() consumes the blender
        b.blend()
    w = S.Warper()
    w.set_scale([S.CameraParams(focal=100.0)])
    with pytest.raises(S.StitchingError):  # float64 R (the reference needs camera_estimator.py:25-26)
        w.warp_roi((10, 10), S.CameraParams(focal=100.0, R=np.eye(3)))
    with pytest.raises(S.StitchingError):
        w.warp_image(np.zeros((10, 10), np.uint8), S.CameraParams(focal=100.0))


@pytest.mark.parametrize("exchange", ["strips", "strips+bits", "contribs"])
@pytest.mark.parametrize("world,strength,n", [(2, 30, 4), (3, 12, 6), (2, 4, 4)])
def test_sharded_blend_equals_single_gpu(oracle, gpu_ctx, world, strength, n, exchange):
    """Column bands + strips (the multi-GPU data path, all ranks simulated on one GPU; both exchange forms: warped image
    strips, per-level contributions) give the bit-identical panorama of the single blender — and of the oracle."""
    from stitching_amd.distributed import virtual_sharded_blend

    imgs, cams = helpers.small_ring(n, 1203, 907, span=40.0 * n)
    o = helpers.run_pipeline(oracle.Warper, oracle.Blender, imgs, cams, blend_strength=strength)
    nb = o["blender"].blender.num_bands()
    req = int(np.log(np.sqrt(o["pano"].shape[0] * o["pano"].shape[1]) * strength / 100) / np.log(2.0) - 1.0)
    pano, mask, plan = virtual_sharded_blend(gpu_ctx, o["w_imgs"], o["w_masks"], o["corners"], o["sizes"], world, req,
                                             exchange.split("+")[0], mask_bits=exchange.endswith("+bits"))
    assert plan.mask_bits == exchange.endswith("+bits")
    assert plan.num_bands == nb and len(plan.messages) >= world - 1
    assert pano.shape == o["pano"].shape
    assert np.array_equal(mask, o["pmask"])
    d = pano.astype(int) - o["pano"].astype(int)
    assert not d.any(), f"{np.count_nonzero(d)} bytes differ, max {np.abs(d).max()}, bands {plan.edges}"


@pytest.mark.timeout(180)
def test_rccl_transport_self_exchange(gpu_ctx):
    """The RCCL strip transport (dlopen'd librccl, ncclSend/ncclRecv grouped on the ctx stream) on a
    1-rank communicator: a strip sent to self arrives intact.  Multi-rank behaviour is the same code
    path with peers != rank (8-GPU node only)."""
    import os

    from stitching_amd.distributed import RcclTransport, call_with_timeout, loopback_bootstrap
    from stitching_amd.device import DeviceImage

    env_before = os.environ.get("NCCL_SOCKET_IFNAME")
    with loopback_bootstrap(True):  # one rank, one host: bootstrap over the loopback interface; the environment is restored
        try:
            # librccl's bootstrap does not come up on every box of the pool (round 5: ncclGetUniqueId waited > 180 s on one): that is the
            # library's environment, not this code path — the product falls back to the host-staged transport (default_transport)
            uid = call_with_timeout(RcclTransport.unique_id, 60.0, "ncclGetUniqueId")
        except S.StitchingError as e:
            pytest.skip(f"librccl does not initialise on this box: {e}")
        tr = RcclTransport(gpu_ctx, 0, 1, uid)
    assert os.environ.get("NCCL_SOCKET_IFNAME") == env_before
    rng = np.random.default_rng(7)
    host = rng.integers(0, 256, size=(1, 1 << 20), dtype=np.uint8)
    src = DeviceImage.from_numpy(host, gpu_ctx)
    (dst,) = tr.exchange([(0, src, host.size)], [(0, host.size)])
    assert np.array_equal(np.asarray(dst), host)
    # a second context (second panorama in flight) shares the communicator: begin_on / end_on
    ctx2 = S.Context(gpu_ctx.device)
    try:
        for rep in range(3):
            for c in (gpu_ctx, ctx2):
                h2 = rng.integers(0, 256, size=(1, 300001), dtype=np.uint8)
                s2 = DeviceImage.from_numpy(h2, c)
                tr.start([(0, s2, h2.size)], [(0, h2.size)], c)
                (d2,) = tr.finish()
                assert d2.ctx is c and np.array_equal(np.asarray(d2), h2)
                del s2, d2
        # two exchanges in flight at once, one per context, finished in the opposite order: each context waits for its own
        ha, hb = (rng.integers(0, 256, size=(1, 500000 + 7 * i), dtype=np.uint8) for i in range(2))
        sa, sb = DeviceImage.from_numpy(ha, gpu_ctx), DeviceImage.from_numpy(hb, ctx2)
        tr.start([(0, sa, ha.size)], [(0, ha.size)], gpu_ctx)
        tr.start([(0, sb, hb.size)], [(0, hb.size)], ctx2)
        (db,) = tr.finish(ctx2)
        (da,) = tr.finish(gpu_ctx)
        assert np.array_equal(np.asarray(da), ha) and np.array_equal(np.asarray(db), hb)
    finally:
        tr.close()
        ctx2.sync()
        ctx2.close()


@pytest.mark.parametrize("wtype", ["spherical", "cylindrical", "plane"])
def test_batched_warp_equals_per_image(oracle, gpu_ctx, wtype):
    """stx_warp_batch (one table launch + one remap launch per 8 images) against the oracle, with more
    images than one launch holds and images of different sizes."""
    n = 11
    cams = synthetic.ring_cameras(n, 517, 389, span_deg=200.0 if wtype != "plane" else 60.0)
    sizes = [(517, 389) if i % 3 else (401, 277) for i in range(n)]
    for c, s in zip(cams, sizes):
        c.ppx, c.ppy = s[0] / 2.0, s[1] / 2.0
    imgs = [synthetic.make_frame(i, s[0], s[1]) for i, s in enumerate(sizes)]
    g, o = S.Warper(wtype), oracle.Warper(wtype)
    g.set_scale(cams)
    o.set_scale(cams)
    gi, gm, rois = g.warp_images_and_masks(imgs, cams)
    assert len(gi) == len(gm) == len(rois) == n
    for i in range(n):
        assert rois[i] == o.warp_roi(sizes[i], cams[i])
        assert np.array_equal(np.asarray(gi[i]), o.warp_image(imgs[i], cams[i])), f"image {i}"
        assert np.array_equal(np.asarray(gm[i]), o.create_and_warp_mask(sizes[i], cams[i])), f"mask {i}"


@pytest.mark.parametrize("exchange", ["strips", "contribs"])
@pytest.mark.parametrize("split", [True, False])
def test_sharded_job_bands_equal_single_job(oracle, gpu_ctx, split, exchange):
    """ShardedStitchJob.run() as bench.py drives it for N > 1 (split: boundary images first, exchange in flight while
    the interior images are warped; not split: one warp launch and one pyramid build for all local images, as with
    several panoramas in flight), both ranks executed one after the other on this GPU: pass 1 records
    every rank's outgoing strips, pass 2 replays them as the incoming ones.  The concatenated bands are the
    single-job panorama bit for bit."""
    from stitching_amd.distributed import ShardedStitchJob, flat_device_buffer
    from stitching_amd.pipeline import StitchJob

    world, n, w, h = 2, 6, 803, 601
    cams = synthetic.ring_cameras(n, w, h, span_deg=40.0 * n)
    frames = [synthetic.make_frame(i, w, h) for i in range(n)]
    single = StitchJob(frames, cams, num_bands=4)
    pano, pmask = (np.asarray(a) for a in single.run())

    sp, sm, jobs = helpers.run_sharded_job_in_one_process(gpu_ctx, frames, cams, world, n // world, num_bands=4, split_boundary=split,
                                                          exchange=exchange)
    assert jobs[0].last_num_bands == single.last_num_bands
    assert sp.shape == pano.shape
    assert np.array_equal(sm, pmask) and np.array_equal(sp, pano)


def test_two_contexts_interleaved(oracle, gpu_ctx):
    """bench.py keeps two panoramas in flight on two contexts (= two HIP streams) that share the source frames:
    interleaved runs give the panorama of a single run, and both contexts stay independent."""
    from stitching_amd.pipeline import StitchJob

    imgs, cams = helpers.small_ring(4, 640, 480, span=150.0)
    a = StitchJob(imgs, cams, num_bands=4, ctx=gpu_ctx)
    ref_pano, ref_mask = (np.asarray(x) for x in a.run())
    ctx2 = S.Context(gpu_ctx.device)
    try:
        b = StitchJob(a.frames, cams, num_bands=4, ctx=ctx2)  # frames live in the first context
        outs = []
        for i in range(6):
            outs.append((a if i % 2 == 0 else b).run())
        for pano, mask in outs:
            assert np.array_equal(np.asarray(pano), ref_pano) and np.array_equal(np.asarray(mask), ref_mask)
        del outs, b
    finally:
        ctx2.sync()
        ctx2.close()


def test_panorama_vs_libm_trig_oracle(oracle, gpu_ctx):
    """The HIP path evaluates sin / cos correctly rounded ("exact" trig); OpenCV calls the host's libm,
    which is not correctly rounded everywhere.  A 1-ULP coordinate difference moves a sample by 1/32 px where it flips
    cvRound(32 x): measured on the +-24-noise texture of the synthetic frames (tools/oracle_sensitivity.py,
    profiles/r02_oracle_sensitivity.md) that is <= 2 LSB in a warped image and <= 3 LSB in the blended panorama, at
    fewer than 1e-5 of the bytes; every other byte is within +-1 and > 99.9 % are identical.  Same ROIs, same masks."""
    w, h = 1600, 1200
    cams = synthetic.ring_cameras(4, w, h, span_deg=170.0)
    imgs = [synthetic.make_frame(40 + i, w, h) for i in range(4)]
    g = helpers.run_pipeline(S.Warper, S.Blender, imgs, cams, blend_strength=2)

    class LibmWarper(oracle.Warper):
        def __init__(self, warper_type="spherical"):
            super().__init__(warper_type, trig=oracle.TRIG_LIBM)

    o = helpers.run_pipeline(LibmWarper, oracle.Blender, imgs, cams, blend_strength=2)
    assert g["blender"].blender.num_bands() == o["blender"].blender.num_bands() >= 4
    assert g["corners"] == o["corners"] and g["sizes"] == o["sizes"]
    assert np.array_equal(g["pmask"], o["pmask"])
    for a, b in zip(g["w_imgs"], o["w_imgs"]):
        d = np.abs(a.astype(np.int16) - b.astype(np.int16))
        assert d.max() <= 2 and np.count_nonzero(d) < 1e-3 * d.size
    d = np.abs(g["pano"].astype(np.int16) - o["pano"].astype(np.int16))
    assert d.max() <= 3
    assert np.count_nonzero(d > 1) <= 1e-5 * d.size
    assert np.count_nonzero(d) < 1e-3 * d.size


@pytest.mark.parametrize("wtype,pitch", [("spherical", 62.0), ("spherical", -75.0), ("cylindrical", 40.0)])
def test_warp_far_outside_the_source(oracle, gpu_ctx, wtype, pitch):
    """A steeply pitched frame: large parts of its ROI lie several mirror images (BORDER_REFLECT periods) away from the
    source — the warp kernel's periodic path (position reduced modulo 2 n pixels, then mirrored) — and, close to the
    horizon of the camera, beyond 2^21 / 32 pixels (generic path).  Image and mask bit for bit."""
    w, h = 331, 207
    img = synthetic.make_frame(77, w, h)
    R = (synthetic.rot_y(np.radians(20.0)) @ synthetic.rot_x(np.radians(pitch)) @ synthetic.rot_z(np.radians(7.0))).astype(np.float32)
    cam = S.CameraParams(focal=0.55 * w, aspect=1.0, ppx=w / 2.0, ppy=h / 2.0, R=R)
    g, o = S.Warper(wtype), oracle.Warper(wtype)
    g.set_scale([cam])
    o.set_scale([cam])
    roi = o.warp_roi((w, h), cam)
    assert g.warp_roi((w, h), cam) == roi and roi[2] * roi[3] > 2 * w * h
    gi, oi = g.warp_image(img, cam), o.warp_image(img, cam)
    assert np.array_equal(gi, oi), f"{np.count_nonzero(gi != oi)} differing bytes"
    gm = g.create_and_warp_mask((w, h), cam)
    assert np.array_equal(gm, o.create_and_warp_mask((w, h), cam)) and 0 < np.count_nonzero(gm) < gm.size


@pytest.mark.parametrize("btype", ["no", "feather"])
@pytest.mark.parametrize("s16", [False, True])
def test_simple_blenders_gather_int16_and_grey_masks(oracle, gpu_ctx, btype, s16):
    """The "no" / feather blenders are deferred gathers over the fed images: int16 inputs outside 0..255 (negative values
    go through |x| of convertScaleAbs), masks with values other than 0 / 255 (the "no" blender ORs them), widths that are no
    multiple of 4, an image fed twice, and the int16 result of blender.blend()."""
    imgs, cams = helpers.small_ring(4, 301, 227, span=130.0)
    ow = oracle.Warper("spherical")
    ow.set_scale(cams)
    sizes = [(301, 227)] * 4
    wi = [ow.warp_image(i, c) for i, c in zip(imgs, cams)]
    if s16:
        wi = [a.astype(np.int16) * 2 - 180 for a in wi]
    wm = [ow.create_and_warp_mask(s, c) for s, c in zip(sizes, cams)]
    rng = np.random.default_rng(3)
    wm[1] = np.where(wm[1] > 0, rng.integers(1, 256, wm[1].shape), 0).astype(np.uint8)  # grey values
    wm[2][::3, ::5] = 0                                                                   # holes
    corners, wsz = ow.warp_rois(sizes, cams)
    order = [0, 1, 2, 3, 1]
    ob, gb = oracle.Blender(btype, 7), S.Blender(btype, 7)
    ob.prepare(corners, wsz)
    gb.prepare(corners, wsz)
    for k in order:
        ob.blender.feed(wi[k].astype(np.int16), wm[k], corners[k])
        gb.feed(wi[k], wm[k], corners[k])
    o16, omask = ob.blender.blend()
    pano, mask, p16 = gb.blender.blend(want_s16=True)
    assert np.array_equal(np.asarray(mask), omask)
    assert np.array_equal(np.asarray(p16), o16)
    assert np.array_equal(np.asarray(pano), oracle.convert_scale_abs(o16))


@pytest.mark.parametrize("kind", ["islands", "empty_and_dots", "grey_islands", "edges"])
def test_blend_sparse_masks_bit_exact(oracle, gpu_ctx, kind):
    """Masks that are zero over most of their feed rectangle: the gather kernels pass over an image wherever the recorded
    row spans of its weight pyramid (StxMbImage::span) say that nothing of it is under a wavefront's 512 x 2 pixels.
    Islands at the 512-column tile seams, single pixels in the corners, one mask entirely zero, grey (non-binary) values
    and one-pixel lines along the rectangle's edges — every panorama is the oracle's bit for bit."""
    imgs, cams = helpers.small_ring(4, 1500, 420, span=150.0)
    rng = np.random.default_rng(31)

    def fn(masks, corners, sizes):
        return helpers.sparse_masks(kind, masks, rng)  # (rng: the closure's current binding, re-seeded before the device's run)

    o = helpers.run_pipeline(oracle.Warper, oracle.Blender, imgs, cams, blend_strength=6, masks_fn=fn)
    rng = np.random.default_rng(31)
    g = helpers.run_pipeline(S.Warper, S.Blender, imgs, cams, blend_strength=6, masks_fn=fn)
    assert np.array_equal(g["pmask"], o["pmask"])
    assert np.array_equal(g["pano"], o["pano"]), int(np.count_nonzero(g["pano"] != o["pano"]))


@pytest.mark.parametrize("n", [1, 2, 3, 15, 16, 17, 40])
def test_blend_many_images_over_the_same_pixels(oracle, gpu_ctx, n):
    """n images stacked over the same panorama pixels with binary masks: the weight sum under a level-0 sample is an integer count up
    to n, and level0_epilogue_pk (csrc/stx_blend_fast.hip, round 6) normalises without a division — a packed shift for counts <= 2, one
    multiplication by v_rcp_f32's reciprocal below 16, the shared-reciprocal IEEE expansion from 16 on.  Extreme pixel values (0 / 255
    checkerboards against flat images) drive the int16 Laplacian sums to both ends of their range; every tier against the oracle's
    plain fp32 division, with counts that change inside a lane's 8 x 2 patch (ragged mask edges)."""
    imgs, masks, corners = helpers.many_images_feeds(n)
    w, h = masks[0].shape[1], masks[0].shape[0]
    sizes = [(w, h)] * n
    ob, gb = oracle.Blender("multiband", 10), S.Blender("multiband", 10)  # 5 bands
    ob.prepare(corners, sizes)
    gb.prepare(corners, sizes)
    for im, m, c in zip(imgs, masks, corners):
        ob.blender.feed(im.astype(np.int16), m, c)
        gb.feed(im, m, c)
    o16, omask = ob.blender.blend()
    pano, mask, p16 = gb.blender.blend(want_s16=True)
    assert np.array_equal(np.asarray(mask), omask)
    assert np.array_equal(np.asarray(p16), o16), int(np.count_nonzero(np.asarray(p16) != o16))
    assert np.array_equal(np.asarray(pano), oracle.convert_scale_abs(o16))
