"""Lens rectification on the GPU: the device equals tests/numpy_rectify.py byte for byte, images and masks, at the smallest shapes at
which the kernel can go wrong — sides that are no multiple of the 16-pixel cell or of a lane's four pixels, one pixel past a tile edge,
single rows and columns, unaligned crop views, several images of unequal sizes in one launch, maps that leave the source or sit at the
clip limits — for numpy, DeviceImage and foreign sources alike; the refusals of the C entry points; and Composer with `lenses=`.

The foreign array is a small class of this file over memory the test owns, as in tests/test_gpu_ingest.py."""
import ctypes as C

import numpy as np
import pytest

import stitching_amd as S
from stitching_amd import _lib, synthetic
from tests import numpy_rectify as N

pytestmark = pytest.mark.gpu
FILL = 0xA5


class Foreign:
    def __init__(self, owner, ptr, shape, strides):
        self.owner = owner
        self.__cuda_array_interface__ = {"version": 3, "shape": tuple(shape), "typestr": "|u1", "data": (ptr, False), "strides": strides}


def put(ctx, arr, pitch=None, offset=0):
    """`arr` in device memory at `offset` bytes into an allocation of the test's own, rows `pitch` bytes apart -> Foreign"""
    a = np.ascontiguousarray(arr)
    rows, row_bytes = a.shape[0], a[0].nbytes
    pitch = row_bytes if pitch is None else pitch
    flat = np.full(offset + rows * pitch + 8, FILL, np.uint8)
    np.lib.stride_tricks.as_strided(flat[offset:], (rows, row_bytes), (pitch, 1))[...] = a.reshape(rows, row_bytes)
    dev = S.DeviceImage.from_numpy(flat.reshape(1, -1), ctx)
    return Foreign(dev, dev.device_ptr() + offset, a.shape, (pitch,) + a.strides[1:])


def image(size, c, seed):
    w, h = size
    return np.random.default_rng(seed).integers(0, 256, (h, w) if c == 1 else (h, w, c), dtype=np.uint8)


def wavy_lens(dst, src, seed=0):
    """a smooth map from dst to src that leaves the source on every side by a few pixels and bends inside"""
    (w, h), (sw, sh) = dst, src
    x, y = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    mx = (x + 0.37) * (sw + 5.0) / w - 2.6 + 1.7 * np.sin(y / 5.0 + seed)
    my = (y + 0.21) * (sh + 4.0) / h - 2.2 + 1.3 * np.cos(x / 7.0 - seed)
    return S.LensMap.from_maps(mx, my, src)


def check(ctx, srcs, hosts, lenses, border):
    """one call with masks, one without: images and masks equal the contract"""
    outs, masks = S.rectify_all(srcs, lenses, border=border, masks=True, ctx=ctx)
    plain = S.rectify_all(srcs, lenses, border=border, ctx=ctx)
    lenses = [lenses] * len(hosts) if isinstance(lenses, S.LensMap) else lenses
    assert len(outs) == len(masks) == len(plain) == len(hosts)
    for k, (host, lens) in enumerate(zip(hosts, lenses)):
        want, want_mask = N.rectify(host, lens.nodes, lens.dst_size, border)
        got, got_mask = outs[k].numpy(), masks[k].numpy()
        assert got.shape == want.shape and got.dtype == np.uint8 and got_mask.shape == want_mask.shape
        assert np.array_equal(got, want), (k, border, np.argwhere(got != want)[:4])
        assert np.array_equal(got_mask, want_mask), (k, border)
        assert np.array_equal(plain[k].numpy(), want), (k, border)


SHAPES = [((70, 37), (53, 41)), ((16, 16), (16, 16)), ((17, 1), (9, 5)), ((1, 17), (5, 9)), ((129, 33), (100, 40))]


@pytest.mark.parametrize("border", N.BORDERS)
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("dst,src", SHAPES, ids=[f"{d[0]}x{d[1]}" for d, _ in SHAPES])
def test_shapes_equal_the_contract(gpu_ctx, dst, src, c, border):
    host, lens = image(src, c, 5), wavy_lens(dst, src)
    mask = N.rectify(host, lens.nodes, dst, border)[1]
    if dst[0] > 1 and dst[1] > 1:
        assert mask.any() and not mask.all()  # the map reaches both sides of the source's edge
    check(gpu_ctx, [host], [host], [lens], border)


@pytest.mark.parametrize("border", N.BORDERS)
@pytest.mark.parametrize("c", [1, 3])
def test_crop_view_source_is_read_inside_its_rectangle_and_left_unchanged(gpu_ctx, c, border):
    """the view starts 5 pixels and 3 rows into its parent: an unaligned base for both channel counts, the parent's pitch"""
    parent = image((64, 50), c, 7)
    dev = S.DeviceImage.from_numpy(parent, gpu_ctx)
    view = dev[3:44, 5:58]
    assert view.shape[:2] == (41, 53) and view.stride_bytes == dev.stride_bytes and view.device_ptr() % 4 != 0
    check(gpu_ctx, [view], [parent[3:44, 5:58]], [wavy_lens((70, 37), (53, 41))], border)
    assert np.array_equal(dev.numpy(), parent)


@pytest.mark.parametrize("border", N.BORDERS)
def test_three_unequal_images_with_three_maps_in_one_launch(gpu_ctx, border):
    specs = [((70, 37), (53, 41), 3), ((129, 33), (100, 40), 1), ((16, 16), (21, 19), 3)]
    hosts = [image(src, c, 11 + k) for k, (_, src, c) in enumerate(specs)]
    lenses = [wavy_lens(dst, src, seed=k) for k, (dst, src, _) in enumerate(specs)]
    check(gpu_ctx, hosts, hosts, lenses, border)
    gpu_ctx.sync()
    gpu_ctx.prof_enable()
    gpu_ctx.prof_reset()
    try:
        S.rectify_all(hosts, lenses, border=border, masks=True, ctx=gpu_ctx)
        gpu_ctx.sync()
        calls = {r["kernel"]: r["calls"] for r in gpu_ctx.prof_results() if r["calls"]}
    finally:
        gpu_ctx.prof_enable(False)
    assert calls.get("rectify") == 1, calls


def test_one_lens_for_a_list(gpu_ctx):
    hosts = [image((53, 41), 3, k) for k in range(3)]
    check(gpu_ctx, hosts, hosts, wavy_lens((70, 37), (53, 41)), "constant")


def test_map_wholly_outside_the_source(gpu_ctx):
    size = (37, 21)
    host = image(size, 3, 13)
    x, y = np.meshgrid(np.arange(37.0), np.arange(21.0))
    lens = S.LensMap.from_maps(x - 500.0, y, size)
    out, mask = S.rectify(host, lens, masks=True, ctx=gpu_ctx)
    assert not out.numpy().any() and not mask.numpy().any()
    out, mask = S.rectify(host, lens, border="replicate", masks=True, ctx=gpu_ctx)
    assert np.array_equal(out.numpy(), np.broadcast_to(host[:, :1], host.shape)) and not mask.numpy().any()
    check(gpu_ctx, [host], [host], [lens], "replicate")


@pytest.mark.parametrize("border", N.BORDERS)
def test_coordinates_at_the_clip_limits(gpu_ctx, border):
    """every combination of the two limits and an inside coordinate over the nodes of a 33 x 33 destination"""
    rng = np.random.default_rng(17)
    host = image((23, 19), 3, 19)
    nodes = rng.choice(np.array([N.Q6_MIN, N.Q6_MAX, 0, 11 * 64 + 13], np.int32), size=(4, 4, 2))
    assert (nodes == N.Q6_MIN).any() and (nodes == N.Q6_MAX).any()
    lens = S.LensMap(nodes, (23, 19), (33, 33))
    check(gpu_ctx, [host], [host], [lens], border)
    far = np.empty((4, 4, 2), np.int32)
    far[..., 0], far[..., 1] = N.Q6_MAX, N.Q6_MIN
    check(gpu_ctx, [host], [host], [S.LensMap(far, (23, 19), (33, 33))], border)


def test_numpy_device_and_foreign_sources_give_the_same_bytes(gpu_ctx):
    host, lens = image((53, 41), 3, 23), wavy_lens((70, 37), (53, 41))
    want, want_mask = N.rectify(host, lens.nodes, (70, 37), "constant")
    dev = S.DeviceImage.from_numpy(host, gpu_ctx)
    foreign = put(gpu_ctx, host, 53 * 3 + 7, 1)  # an odd base and an odd pitch
    before = foreign.owner.numpy()
    for src in (host, dev, foreign):
        out, mask = S.rectify(src, lens, masks=True, ctx=gpu_ctx)
        assert np.array_equal(out.numpy(), want) and np.array_equal(mask.numpy(), want_mask), type(src).__name__
    assert np.array_equal(dev.numpy(), host) and np.array_equal(foreign.owner.numpy(), before)  # the sources are unchanged
    gray = image((53, 41), 1, 29)
    assert np.array_equal(S.rectify(put(gpu_ctx, gray, 64, 3), lens, ctx=gpu_ctx).numpy(), N.rectify(gray, lens.nodes, (70, 37))[0])


def test_lens_models_on_the_device(gpu_ctx):
    """a Brown and a fisheye LensMap through the device: what the host constructors make is what the kernel takes"""
    K = np.array([[70.0, 0.0, 47.3], [0.0, 70.0, 35.6], [0.0, 0.0, 1.0]])
    host = image((96, 72), 3, 31)
    lenses = [S.LensMap.brown(K, (-0.25, 0.06, 0.001, -0.0008, -0.01), (96, 72), fit="inside"),
              S.LensMap.fisheye(K, (-0.03, 0.01, -0.004, 0.001), (96, 72), dst_size=(70, 37)),
              S.LensMap.brown(K, (0.25, 0.05, 0.0, 0.0), (96, 72))]
    check(gpu_ctx, [host] * 3, [host] * 3, lenses, "constant")
    _, masks = S.rectify_all([host] * 3, lenses, masks=True, ctx=gpu_ctx)
    assert masks[0].numpy().all() and not masks[2].numpy().all()


def test_c_entry_points_refuse_on_the_host(gpu_ctx):
    L, ctx = gpu_ctx._lib, gpu_ctx.handle
    nodes = np.zeros((4, 6, 2), np.int32)
    ptr = nodes.ctypes.data_as(C.POINTER(C.c_int))

    def refused(rc, text):
        assert rc != 0 and text in L.stx_last_error().decode(), L.stx_last_error()

    h = C.c_void_p()
    refused(L.stx_lens_map_create(ctx, 70, 37, 53, 41, 5, 4, ptr, C.byref(h)), "6 x 4")         # the node count does not match (W, H)
    refused(L.stx_lens_map_create(ctx, 70, 37, 53, 41, 6, 3, ptr, C.byref(h)), "6 x 4")
    refused(L.stx_lens_map_create(ctx, 16385, 37, 53, 41, 6, 4, ptr, C.byref(h)), "1 .. 16384")  # a side above 16 384
    refused(L.stx_lens_map_create(ctx, 70, 37, 53, 16385, 6, 4, ptr, C.byref(h)), "1 .. 16384")
    refused(L.stx_lens_map_create(ctx, 70, 37, 53, 41, 6, 4, None, C.byref(h)), "null")
    wild = nodes.copy()
    wild[1, 1, 0] = 1 << 22
    refused(L.stx_lens_map_create(ctx, 70, 37, 53, 41, 6, 4, wild.ctypes.data_as(C.POINTER(C.c_int)), C.byref(h)), "clip limits")
    assert h.value is None
    assert L.stx_lens_map_create(ctx, 70, 37, 53, 41, 6, 4, ptr, C.byref(h)) == 0 and h.value
    good = S.DeviceImage.from_numpy(image((53, 41), 3, 1), gpu_ctx)
    one, out = (C.c_void_p * 1)(h.value), (C.c_void_p * 1)()

    def call(img, m=one, border=0, masks=0, n=1):
        return L.stx_rectify(ctx, n, (C.c_void_p * 1)(img), m, border, masks, out, None)

    refused(call(None), "image 0 is a null handle")
    refused(call(good._h.value, (C.c_void_p * 1)()), "lens map 0 is a null handle")
    narrow = S.DeviceImage.from_numpy(image((52, 41), 3, 1), gpu_ctx)
    four = S.DeviceImage.from_numpy(np.zeros((41, 53, 4), np.uint8), gpu_ctx)
    real = S.DeviceImage.from_numpy(np.zeros((41, 53), np.float32), gpu_ctx)
    refused(call(narrow._h.value), "52x41")           # not the map's source size
    refused(call(four._h.value), "1 or 3 channels")
    refused(call(real._h.value), "1 or 3 channels")  # not u8
    refused(call(good._h.value, border=2), "border")
    refused(call(good._h.value, masks=1), "null")  # masks wanted, nowhere to put them
    refused(call(good._h.value, n=0), "0 images")
    assert out[0] is None
    assert call(good._h.value) == 0 and out[0]  # the context stays usable
    img = S.DeviceImage(gpu_ctx, C.c_void_p(out[0]))
    assert np.array_equal(img.numpy(), N.rectify(good.numpy(), nodes, (70, 37))[0])
    gpu_ctx.sync()
    assert L.stx_lens_map_free(h) == 0
    # the Python layer's own refusals reach the same ground: the counts differ
    with pytest.raises(S.StitchingError, match="2 lenses for 1 frames"):
        S.rectify_all([good], [wavy_lens((70, 37), (53, 41))] * 2, ctx=gpu_ctx)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def undistort_points(K, dist, u, v, iters=20):
    """Brown: distorted pixel (u, v) -> ideal pixel of the same K, by the usual fixed-point iteration"""
    k1, k2, p1, p2, k3 = dist
    xd, yd = (u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1]
    x, y = xd.copy(), yd.copy()
    for _ in range(iters):
        r2 = x * x + y * y
        radial = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
        x = (xd - (2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x))) / radial
        y = (yd - (p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y)) / radial
    return K[0, 0] * x + K[0, 2], K[1, 1] * y + K[1, 2]


@pytest.fixture(scope="module")
def rig():
    """three frames of 160 x 120, their cameras, a Brown lens per camera, and the frames as that lens would have taken them"""
    n, w, h = 3, 160, 120
    kw = dict(finder="voronoi", medium_megapix=0.005, low_megapix=0.002)
    frames = synthetic.make_frames(range(n), w, h)
    mw, mh = S.Images.of(frames, kw["medium_megapix"], kw["low_megapix"], -1).get_scaled_img_sizes(S.Images.Resolution.MEDIUM)[0]
    cams = synthetic.ring_cameras(n, mw, mh, focal_factor=0.75, span_deg=100.0)
    lenses, distorted = [], []
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    for i, f in enumerate(frames):
        K = np.array([[0.75 * w, 0.0, w / 2.0 - 1.5 + i], [0.0, 0.75 * w, h / 2.0 + 1.0 - i], [0.0, 0.0, 1.0]])
        dist = (-0.18 - 0.02 * i, 0.04, 0.0006, -0.0004, -0.004)
        lenses.append(S.LensMap.brown(K, dist, (w, h)))
        inverse = S.LensMap.from_maps(*undistort_points(K, dist, u, v), (w, h))  # where in the ideal frame a distorted pixel looks
        distorted.append(N.rectify(f, inverse.nodes, (w, h), "replicate")[0])
    return kw, frames, cams, lenses, distorted


def test_the_lens_and_its_inverse_undo_each_other(gpu_ctx, rig):
    """sanity of the fixture: distorting and rectifying a smooth image brings it back, to resampling error, where the source covers it"""
    _, _, _, lenses, _ = rig
    w, h = 160, 120
    yy, xx = np.mgrid[0:h, 0:w]
    smooth = np.clip(128 + 60 * np.sin(xx / 17.0) + 50 * np.cos(yy / 13.0), 0, 255).astype(np.uint8)
    K, dist = lenses[0].new_K, (-0.18, 0.04, 0.0006, -0.0004, -0.004)
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    inverse = S.LensMap.from_maps(*undistort_points(K, dist, u, v), (w, h))
    distorted = N.rectify(smooth, inverse.nodes, (w, h), "replicate")[0]
    back, mask = S.rectify(distorted, lenses[0], masks=True, ctx=gpu_ctx)
    back, mask = back.numpy().astype(int), mask.numpy() == 255
    assert mask.all()  # a barrel lens samples inwards
    assert np.abs(distorted.astype(int) - smooth).max() > 8          # the lens moves things
    assert np.abs(back - smooth)[8:-8, 8:-8].max() <= 3               # and rectification puts them back


def test_composer_with_lenses_equals_rectify_then_compose(gpu_ctx, rig):
    kw, frames, cams, lenses, distorted = rig
    want = S.Composer(ctx=gpu_ctx, **kw).compose(S.rectify_all(distorted, lenses, ctx=gpu_ctx), cams).numpy()
    got = S.Composer(ctx=gpu_ctx, **kw).compose(distorted, cams, lenses=lenses).numpy()
    assert want.shape == got.shape and np.array_equal(want, got)
    assert not np.array_equal(S.Composer(ctx=gpu_ctx, **kw).compose(distorted, cams).numpy(), got)  # the lenses did something
    # new distorted frames on a prepared plan
    comp = S.Composer(ctx=gpu_ctx, **kw)
    plan = comp.prepare(distorted, cams, lenses=lenses)
    again = distorted[::-1]
    pano, mask = comp.run(plan, images=again, lenses=lenses[::-1])
    pano2, mask2 = comp.run(plan, images=S.rectify_all(again, lenses[::-1], ctx=gpu_ctx))
    assert np.array_equal(pano.numpy(), pano2.numpy()) and np.array_equal(mask.numpy(), mask2.numpy())
    with pytest.raises(S.StitchingError, match="the lenses were made for"):
        comp.run(plan, images=[d[:, :-1] for d in distorted], lenses=lenses)


def test_composer_without_lenses_is_unchanged(gpu_ctx, rig):
    kw, frames, cams, _, _ = rig
    comp = S.Composer(ctx=gpu_ctx, **kw)
    present = [x.numpy() for x in comp.run(comp.prepare(frames, cams))]
    comp2 = S.Composer(ctx=gpu_ctx, **kw)
    none = [x.numpy() for x in comp2.run(comp2.prepare(frames, cams, lenses=None), lenses=None)]
    assert np.array_equal(present[0], none[0]) and np.array_equal(present[1], none[1])
    assert np.array_equal(S.Composer(ctx=gpu_ctx, **kw).compose(frames, cams, lenses=None).numpy(), present[0])
