"""Device frame ingest on the GPU: foreign device arrays in every pixel format equal tests/numpy_ingest.py byte for byte, on the wide and
on the byte path of the kernel, in one launch per list; export through `__cuda_array_interface__`; foreign frames through StitchJob and
Composer; refusals decided on the host.

The foreign array is a small class of this file over memory the test owns: a flat u8 DeviceImage and `device_ptr() + offset`, which
gives any base offset and any pitch.  No second GPU framework enters the process."""
import ctypes as C

import numpy as np
import pytest

import stitching_amd as S
from stitching_amd import _lib, synthetic
from tests import numpy_ingest as N

pytestmark = pytest.mark.gpu
FILL = 0xA5  # what lies between and around the rows of a padded source


class Foreign:
    """A pointer, a shape, strides and an owner: all a consumer of `__cuda_array_interface__` sees of another framework's array."""

    def __init__(self, owner, ptr, shape, strides, typestr="|u1", stream="absent"):
        self.owner = owner
        self.__cuda_array_interface__ = {"version": 3, "shape": tuple(shape), "typestr": typestr, "data": (ptr, False), "strides": strides}
        if stream != "absent":
            self.__cuda_array_interface__["stream"] = stream


def put(ctx, arr, pitch=None, offset=0, stream="absent"):
    """`arr` in device memory at `offset` bytes into an allocation of the test's own, rows `pitch` bytes apart -> Foreign"""
    a = np.ascontiguousarray(arr)
    rows, row_bytes = a.shape[0], a[0].nbytes
    pitch = row_bytes if pitch is None else pitch
    flat = np.full(offset + rows * pitch + 8, FILL, np.uint8)
    np.lib.stride_tricks.as_strided(flat[offset:], (rows, row_bytes), (pitch, 1))[...] = a.view(np.uint8).reshape(rows, row_bytes)
    dev = S.DeviceImage.from_numpy(flat.reshape(1, -1), ctx)
    return Foreign(dev, dev.device_ptr() + offset, a.shape, (pitch,) + a.strides[1:], a.dtype.str if a.itemsize > 1 else "|u1", stream)


def same(img, want):
    got = img.numpy()
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want)


def source(fmt, h, w, rng, dtype=np.uint8, c=None):
    c = {"bgr": 3, "rgb": 3, "bgra": 4, "rgba": 4, "gray": 1}.get(fmt, c)
    shape = (h, w) if c == 1 else (h, w, c)
    if dtype == np.float32:
        return rng.standard_normal(shape).astype(np.float32)
    return rng.integers(np.iinfo(dtype).min, int(np.iinfo(dtype).max) + 1, shape, dtype=dtype)


# ---- packed formats ---------------------------------------------------------------------------------------------------------------
PACKED_SIZES = [(1, 1), (2, 3), (5, 7), (4, 64), (3, 257)]
PACKED = [("bgr", np.uint8, None), ("rgb", np.uint8, None), ("bgra", np.uint8, None), ("rgba", np.uint8, None), ("gray", np.uint8, None),
          (None, np.uint8, 1), (None, np.uint8, 2), (None, np.uint8, 3), (None, np.uint8, 4), (None, np.int16, 3), (None, np.float32, 1),
          (None, np.float32, 4)]


@pytest.mark.parametrize("fmt,dtype,c", PACKED, ids=[f"{f}-{np.dtype(d).name}-{c}" for f, d, c in PACKED])
def test_packed_formats_equal_the_contract(gpu_ctx, fmt, dtype, c):
    """every size x pitch (tight, tight + 5) x base offset (0: words, 1: bytes) — one list, one launch — and one frame on its own"""
    rng = np.random.default_rng(11)
    hosts, frames = [], []
    for h, w in PACKED_SIZES:
        for pad in (0, 5):
            for offset in (0, 1):
                a = source(fmt, h, w, rng, dtype, c)
                hosts.append(a)
                frames.append(put(gpu_ctx, a, a[0].nbytes + pad, offset))
    outs = S.ingest_all(frames, format=fmt, ctx=gpu_ctx)
    assert len(outs) == len(hosts)
    for a, out in zip(hosts, outs):
        assert same(out, N.to_bgr(a, fmt)), (fmt, a.shape)
    assert same(S.ingest(frames[-1], format=fmt, ctx=gpu_ctx), N.to_bgr(hosts[-1], fmt))
    assert same(S.DeviceImage.from_device(frames[4], format=fmt, ctx=gpu_ctx), N.to_bgr(hosts[4], fmt))


# ---- nv12 and i420 ----------------------------------------------------------------------------------------------------------------
YUV_SIZES = [(1, 1), (2, 2), (3, 5), (6, 8), (7, 259)]


def yuv_planes(h, w, rng):
    ch, cw = N.chroma_shape(h, w)
    return (rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (ch, cw), dtype=np.uint8),
            rng.integers(0, 256, (ch, cw), dtype=np.uint8))


def yuv_frames(ctx, fmt, y, u, v, pitches, offset):
    """pitches: None (tight), "padded" (Y: w + 3; UV: 2 ceil(w / 2) + 2; U, V: ceil(w / 2) + 1) or a number for every plane"""
    h, w = y.shape
    cw = u.shape[1]
    if fmt == "nv12":
        planes, padded = (y, np.stack([u, v], axis=-1)), (w + 3, 2 * cw + 2)
    else:
        planes, padded = (y, u, v), (w + 3, cw + 1, cw + 1)
    p = [None] * 3 if pitches is None else padded if pitches == "padded" else [pitches] * 3
    return planes, tuple(put(ctx, a, p[k], offset) for k, a in enumerate(planes))


@pytest.mark.parametrize("matrix,range_", N.VARIANTS)
@pytest.mark.parametrize("fmt", ["nv12", "i420"])
def test_yuv_formats_equal_the_contract(gpu_ctx, fmt, matrix, range_):
    """every size x pitches (tight, padded, all 256 where a row fits) x base offset (0, 1, 2: the 16-bit chroma loads of i420 are
    aligned at 2) in one list"""
    rng = np.random.default_rng(23)
    wants, frames = [], []
    for h, w in YUV_SIZES:
        y, u, v = yuv_planes(h, w, rng)
        for pitches in (None, "padded", 256):
            if pitches == 256 and w > 256:
                continue
            for offset in (0, 1, 2):
                planes, frame = yuv_frames(gpu_ctx, fmt, y, u, v, pitches, offset)
                wants.append(N.to_bgr(planes, fmt, matrix, range_))
                frames.append(frame)
    outs = S.ingest_all(frames, format=fmt, matrix=matrix, range=range_, ctx=gpu_ctx)
    for want, out in zip(wants, outs):
        assert same(out, want), (fmt, matrix, range_, want.shape)


def test_single_contiguous_nv12_array(gpu_ctx):
    rng = np.random.default_rng(3)
    y, u, v = yuv_planes(6, 8, rng)
    uv = np.stack([u, v], axis=-1)
    whole = np.concatenate([y, uv.reshape(3, 8)], axis=0)  # (H * 3 / 2) x W
    assert same(S.ingest(put(gpu_ctx, whole), format="nv12", ctx=gpu_ctx), N.to_bgr((y, uv), "nv12"))


@pytest.fixture(scope="module")
def every_triple(gpu_ctx):
    """A 4096 x 4096 nv12 frame whose 2 x 2 blocks enumerate all 65 536 (U, V) pairs against all 256 Y values: block k = by * 2048 + bx
    holds the pair (U, V) = (k & 255, (k >> 8) & 255) and the four Y values 4 (k >> 16) .. 4 (k >> 16) + 3.  Uploaded once."""
    k = np.arange(2048 * 2048, dtype=np.int64).reshape(2048, 2048)
    uv = np.stack([k & 255, (k >> 8) & 255], axis=-1).astype(np.uint8)
    y = np.empty((4096, 4096), np.uint8)
    g = ((k >> 16) * 4).astype(np.uint8)
    y[0::2, 0::2], y[0::2, 1::2], y[1::2, 0::2], y[1::2, 1::2] = g, g + 1, g + 2, g + 3
    triples = np.unique((y.astype(np.int64)[::2, ::2] >> 2 << 16 | k & 0xFFFF).reshape(-1))
    assert triples.size == 64 * 65536  # 64 groups of four Y values x every pair: with the four of a block, all 2^24 triples
    return (y, uv), (put(gpu_ctx, y), put(gpu_ctx, uv))


@pytest.mark.parametrize("matrix,range_", N.VARIANTS)
def test_arithmetic_exhaustively(gpu_ctx, every_triple, matrix, range_):
    planes, frame = every_triple
    out = S.ingest(frame, format="nv12", matrix=matrix, range=range_, ctx=gpu_ctx)
    assert same(out, N.to_bgr(planes, "nv12", matrix, range_))


# ---- one launch for a list --------------------------------------------------------------------------------------------------------
def test_one_launch_for_a_list_of_unequal_frames(gpu_ctx):
    rng = np.random.default_rng(7)
    y, u, v = yuv_planes(37, 301, rng)
    nv12, f_nv12 = yuv_frames(gpu_ctx, "nv12", y, u, v, 512, 0)
    bgra = source("bgra", 9, 700, rng)
    i420, f_i420 = yuv_frames(gpu_ctx, "i420", *yuv_planes(5, 3, rng), "padded", 1)
    mask = source("gray", 20, 33, rng)
    frames = [f_nv12, put(gpu_ctx, bgra, offset=1), f_i420, put(gpu_ctx, mask, 40)]
    formats = ["nv12", "bgra", "i420", None]
    gpu_ctx.sync()
    gpu_ctx.prof_enable()
    gpu_ctx.prof_reset()
    try:
        outs = S.ingest_all(frames, format=formats, matrix="bt601", range="full", ctx=gpu_ctx)
        launched = [(r["kernel"], r["calls"]) for r in gpu_ctx.prof_results() if r["calls"]]
    finally:
        gpu_ctx.prof_enable(False)
    assert launched == [("ingest", 1)]
    wants = [N.to_bgr(nv12, "nv12", "bt601", "full"), N.to_bgr(bgra, "bgra"), N.to_bgr(i420, "i420", "bt601", "full"), mask]
    for want, out in zip(wants, outs):
        assert same(out, want)
    flags = C.c_int(-1)
    _lib.check(gpu_ctx._lib.stx_buf_flags(outs[3]._h, C.byref(flags)))
    assert flags.value == 0  # nothing is known about a foreign mask


# ---- ordering arguments -------------------------------------------------------------------------------------------------------------
def test_stream_and_wait_arguments_give_the_same_bytes(gpu_ctx):
    """the legacy default stream as the producer's (argument and the object's own entry), wait=False followed by ctx.sync(); no race is
    staged"""
    rng = np.random.default_rng(9)
    a = source("rgb", 21, 130, rng)
    want = N.to_bgr(a, "rgb")
    assert same(S.ingest(put(gpu_ctx, a), format="rgb", stream=1, ctx=gpu_ctx), want)
    assert same(S.ingest(put(gpu_ctx, a, stream=1), format="rgb", ctx=gpu_ctx), want)
    assert same(S.ingest(put(gpu_ctx, a, stream=None), format="rgb", ctx=gpu_ctx), want)
    assert same(S.ingest(put(gpu_ctx, a, stream=77), format="rgb", stream=1, ctx=gpu_ctx), want)  # stream= overrides the entry
    src = put(gpu_ctx, a)
    out = S.ingest(src, format="rgb", wait=False, ctx=gpu_ctx)
    gpu_ctx.sync()
    assert same(out, want)


# ---- export ---------------------------------------------------------------------------------------------------------------------------
def test_export_of_an_image_and_of_a_crop_view(gpu_ctx):
    rng = np.random.default_rng(13)
    for a in (source("bgr", 19, 37, rng), source("gray", 19, 37, rng), source(None, 6, 9, rng, np.int16, 3), source(None, 6, 9, rng, np.float32, 1)):
        img = S.DeviceImage.from_numpy(a, gpu_ctx)
        d = img.__cuda_array_interface__
        size = a.itemsize
        assert d["version"] == 3 and d["shape"] == a.shape and d["typestr"] == ("|u1" if size == 1 else a.dtype.str)
        assert d["data"] == (img.device_ptr(), False) and d["stream"] is None and "mask" not in d
        assert d["strides"] == ((img.stride_bytes, size) if a.ndim == 2 else (img.stride_bytes, a.shape[2] * size, size))
        assert S.parse_cuda_array_interface(img)[:6] == (img.device_ptr(), a.shape[0], a.shape[1], img.channels, img._elem, img.stride_bytes)
        crop = img[2:5, 3:8]
        dc = crop.__cuda_array_interface__
        assert dc["shape"] == a[2:5, 3:8].shape and dc["strides"] == d["strides"]  # the parent's pitch
        assert dc["data"][0] == crop.device_ptr() == img.device_ptr() + 2 * img.stride_bytes + 3 * size * img.channels
        # the crop, wrapped as a foreign array and ingested, equals the numpy slice
        back = S.ingest(Foreign(crop, dc["data"][0], dc["shape"], dc["strides"], dc["typestr"]), ctx=gpu_ctx)
        assert same(back, a[2:5, 3:8]) and back.device_ptr() != crop.device_ptr()
        assert same(S.as_device(Foreign(img, d["data"][0], d["shape"], d["strides"], d["typestr"]), gpu_ctx), a)


# ---- pipeline -------------------------------------------------------------------------------------------------------------------------
def test_as_device_takes_a_foreign_array(gpu_ctx):
    rng = np.random.default_rng(17)
    a, m = source("bgr", 12, 20, rng), source("gray", 12, 20, rng)
    assert same(S.as_device(put(gpu_ctx, a, 70, 1), gpu_ctx), a) and same(S.as_device(put(gpu_ctx, m), gpu_ctx), m)


def test_stitch_job_on_foreign_frames(gpu_ctx):
    n, w, h = 2, 64, 48
    cams = synthetic.ring_cameras(n, w, h, focal_factor=0.75, span_deg=90.0)
    first, second = synthetic.make_frames(range(0, n), w, h), synthetic.make_frames(range(5, 5 + n), w, h)
    want = S.pipeline.StitchJob(first, cams, ctx=gpu_ctx)
    want1 = [x.numpy() for x in want.run()]
    want2 = [x.numpy() for x in want.run(frames=second)]
    assert not np.array_equal(want1[0], want2[0])
    job = S.pipeline.StitchJob([put(gpu_ctx, f, w * 3 + 13, 1) for f in first], cams, ctx=gpu_ctx)
    got1 = [x.numpy() for x in job.run()]
    got2 = [x.numpy() for x in job.run(frames=[put(gpu_ctx, f) for f in second])]
    assert job.last_reused  # the second run is the known rig's
    for a, b in zip(want1 + want2, got1 + got2):
        assert np.array_equal(a, b)
    want = [x.numpy() for x in S.pipeline.compose(first, cams, ctx=gpu_ctx)]
    got = [x.numpy() for x in S.pipeline.compose([put(gpu_ctx, f) for f in first], cams, ctx=gpu_ctx)]
    assert np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1])


def test_composer_on_foreign_frames(gpu_ctx):
    n, w, h = 2, 64, 48
    kw = dict(finder="voronoi", medium_megapix=0.005, low_megapix=0.002)
    old, new = synthetic.make_frames(range(0, n), w, h), synthetic.make_frames(range(5, 5 + n), w, h)
    images = S.Images.of(old, kw["medium_megapix"], kw["low_megapix"], -1)
    mw, mh = images.get_scaled_img_sizes(S.Images.Resolution.MEDIUM)[0]
    cams = synthetic.ring_cameras(n, mw, mh, focal_factor=0.75, span_deg=90.0)
    comp = S.Composer(ctx=gpu_ctx, **kw)
    plan = comp.prepare(old, cams)
    want = [x.numpy() for x in comp.run(plan, images=new)]
    got = [x.numpy() for x in comp.run(plan, images=[put(gpu_ctx, f, w * 3 + 7, 1) for f in new])]
    assert np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1])
    comp2 = S.Composer(ctx=gpu_ctx, **kw)
    got = [x.numpy() for x in comp2.run(comp2.prepare([put(gpu_ctx, f) for f in old], cams), images=[put(gpu_ctx, f) for f in new])]
    assert np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1])
    with pytest.raises(S.StitchingError, match="same rig, same sizes"):
        comp.run(plan, images=[put(gpu_ctx, f[:, :-1]) for f in new])


# ---- refusals: decided on the host, nothing is launched, the context works afterwards -------------------------------------------------------
def raw_ingest(ctx, ptr, pitch, w, h, channels, elem, fmt):
    """stx_ingest itself, past the checks of the Python layer -> (status, message)"""
    F = (_lib.ForeignFrame * 1)()
    F[0].plane[0], F[0].pitch[0] = ptr, pitch
    F[0].w, F[0].h, F[0].channels, F[0].elem, F[0].format = w, h, channels, elem, fmt
    out = (C.c_void_p * 1)()
    rc = ctx._lib.stx_ingest(ctx.handle, 1, F, 1, 0, None, 0, out)
    assert rc != 0 or out[0]
    if rc == 0:
        ctx._lib.stx_buf_free(C.c_void_p(out[0]))
    return rc, ctx._lib.stx_last_error().decode()


def test_refusals(gpu_ctx):
    rng = np.random.default_rng(19)
    a = source("bgr", 8, 10, rng)
    good = put(gpu_ctx, a)
    ptr = good.__cuda_array_interface__["data"][0]
    host = np.ascontiguousarray(a)
    pinned = S.pinned_empty(a.shape)
    gpu_ctx.sync()
    gpu_ctx.prof_enable()
    gpu_ctx.prof_reset()
    try:
        # host pointers: pageable and page-locked
        with pytest.raises(S.StitchingError, match="from_numpy"):
            S.ingest(Foreign(host, host.ctypes.data, a.shape, None), ctx=gpu_ctx)
        with pytest.raises(S.StitchingError, match="from_numpy"):
            S.ingest(Foreign(pinned, pinned.ctypes.data, a.shape, None), ctx=gpu_ctx)
        # a shape that claims 2^40 bytes: far more than any allocation holds
        with pytest.raises(S.StitchingError, match="its allocation holds"):
            S.ingest(Foreign(good.owner, ptr, (1 << 14, 10, 3), (1 << 26, 3, 1)), ctx=gpu_ctx)
        # a pitch below the row bytes: the Python layer refuses it, and so does the library
        with pytest.raises(S.StitchingError, match="row stride"):
            S.ingest(Foreign(good.owner, ptr, a.shape, (29, 3, 1)), ctx=gpu_ctx)
        rc, msg = raw_ingest(gpu_ctx, ptr, 29, 10, 8, 3, _lib.U8, _lib.INGEST_FORMATS["bgr"])
        assert rc == -1 and "pitch" in msg
        # a format that disagrees with its channel count
        with pytest.raises(S.StitchingError, match="4 channel"):
            S.ingest(good, format="bgra", ctx=gpu_ctx)
        rc, msg = raw_ingest(gpu_ctx, ptr, 30, 10, 8, 3, _lib.U8, _lib.INGEST_FORMATS["bgra"])
        assert rc == -1 and "channel" in msg
        rc, msg = raw_ingest(gpu_ctx, ptr, 30, 10, 8, 1, _lib.U8, _lib.INGEST_FORMATS["nv12"])  # the UV plane is missing
        assert rc == -1 and "null" in msg
        for w, h in ((0, 8), (10, 0), (_lib.INGEST_MAX_SIDE + 1, 8)):
            rc, msg = raw_ingest(gpu_ctx, ptr, 1 << 20, w, h, 3, _lib.U8, 0)
            assert rc == -1 and "on a side" in msg
        launched = [r["kernel"] for r in gpu_ctx.prof_results() if r["calls"]]
    finally:
        gpu_ctx.prof_enable(False)
    assert launched == []
    assert same(S.ingest(good, format="bgr", ctx=gpu_ctx), a)  # the context is usable
