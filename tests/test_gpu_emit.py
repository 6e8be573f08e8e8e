"""Device frame emit on the GPU: every format equals tests/numpy_emit.py byte for byte, into planes of the library's own and in place
into foreign memory on the word, the 16-bit and the byte path of the kernel, from whole images and from crop views, in one launch per
list; not one byte outside the planes' rows changes; the arithmetic over all 2^24 colours; alpha; ordering arguments; the way back
through ingest; a StitchJob's panorama; refusals decided on the host.

Foreign memory is made as tests/test_gpu_ingest.py makes it: an allocation the test owns (a flat u8 DeviceImage) filled with a sentinel
byte, the target planes at offsets and pitches inside it.  No second GPU framework enters the process."""
import ctypes as C

import numpy as np
import pytest

import stitching_amd as S
from stitching_amd import _lib, synthetic
from tests import numpy_emit as E
from tests import numpy_ingest as N

pytestmark = pytest.mark.gpu
FILL = 0xA5  # what lies before, between, beside and after the rows of a target's planes


class Foreign:
    """A pointer, a shape, strides and an owner: all a consumer of `__cuda_array_interface__` sees of another framework's array."""

    def __init__(self, owner, ptr, shape, strides, typestr="|u1", stream="absent"):
        self.owner = owner
        self.__cuda_array_interface__ = {"version": 3, "shape": tuple(shape), "typestr": typestr, "data": (ptr, False), "strides": strides}
        if stream != "absent":
            self.__cuda_array_interface__["stream"] = stream


def planes_of(want):
    return list(want) if isinstance(want, tuple) else [want]


def row_bytes_of(a):
    return a[0].nbytes


def pitch_for(row_bytes, mode):
    """words: a multiple of 4; halves: 2 mod 4; bytes: odd — each with a few bytes of padding behind the row"""
    if mode == "words":
        return (row_bytes + 3) // 4 * 4 + 8
    if mode == "halves":
        return (row_bytes + 3) // 4 * 4 + 6
    return (row_bytes + 5) | 1


def place(cur, mode):
    """the next base at or after `cur`: a multiple of 4, 2 mod 4, or odd"""
    cur = (cur + 3) // 4 * 4
    return cur if mode == "words" else cur + 2 if mode == "halves" else cur + 1


class Arena:
    """An allocation of the test's own that holds the target planes of one emit, `mode` deciding bases and pitches.  `targets` is what
    emit takes; `check(want)` reads the WHOLE allocation back: the planes' rows hold `want`, every other byte is still FILL."""

    def __init__(self, ctx, want, mode, stream="absent"):
        self.spans, cur = [], 16
        for a in planes_of(want):
            off, pitch = place(cur, mode), pitch_for(row_bytes_of(a), mode)
            self.spans.append((off, pitch))
            cur = off + a.shape[0] * pitch + 7
        self.size = cur + 16
        self.dev = S.DeviceImage.from_numpy(np.full((1, self.size), FILL, np.uint8), ctx)
        base = self.dev.device_ptr()
        assert base % 64 == 0
        objs = [Foreign(self.dev, base + off, a.shape, (pitch,) + np.empty(a.shape, a.dtype).strides[1:], a.dtype.str if a.itemsize > 1 else "|u1",
                        stream) for a, (off, pitch) in zip(planes_of(want), self.spans)]  # packed pixels whatever order numpy keeps `a` in
        self.targets = tuple(objs) if isinstance(want, tuple) else objs[0]

    def check(self, want):
        flat = np.full(self.size, FILL, np.uint8)
        for a, (off, pitch) in zip(planes_of(want), self.spans):
            rows, rb = a.shape[0], row_bytes_of(a)
            np.lib.stride_tricks.as_strided(flat[off:], (rows, rb), (pitch, 1))[...] = np.ascontiguousarray(a).view(np.uint8).reshape(rows, rb)
        got = self.dev.numpy().reshape(-1)
        bad = np.flatnonzero(got != flat)
        assert bad.size == 0, f"{bad.size} bytes differ, the first at {int(bad[0])} of {self.size}: {int(got[bad[0]])} for {int(flat[bad[0]])}"


def same(img, want):
    got = img.numpy()
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want)


def same_planes(got, want):
    if isinstance(want, tuple):
        return isinstance(got, tuple) and len(got) == len(want) and all(same(g, w) for g, w in zip(got, want))
    return same(got, want)


def source(rng, h, w, c=3, dtype=np.uint8):
    shape = (h, w) if c == 1 else (h, w, c)
    if dtype == np.float32:
        return rng.standard_normal(shape).astype(np.float32)
    return rng.integers(np.iinfo(dtype).min, int(np.iinfo(dtype).max) + 1, shape, dtype=dtype)


def upload(ctx, a, crop):
    """`a` on the device: an image of its own, or a crop view at x = 3 (an odd byte for u8 with 1 or 3 channels), y = 1 of a larger one"""
    if not crop:
        return S.DeviceImage.from_numpy(a, ctx)
    big = np.full((a.shape[0] + 2, a.shape[1] + 5) + a.shape[2:], 77, a.dtype)
    big[1:-1, 3:-2] = a
    return S.DeviceImage.from_numpy(big, ctx)[1:-1, 3:-2]


# ---- every format, size, source and target ------------------------------------------------------------------------------------------
# 257: one pixel more than a workgroup's 64 lanes x 4 pixels; 5 rows / 9 rows: one row unit more than a workgroup's 4 (4:2:0: row pairs)
SIZES = [(1, 1), (2, 3), (5, 7), (1, 9), (7, 1), (4, 64), (3, 257), (9, 6)]
CASES = [("bgr", 3, np.uint8, None), ("rgb", 3, np.uint8, None), ("bgra", 3, np.uint8, None), ("rgba", 3, np.uint8, None),
         ("gray", 1, np.uint8, None), (None, 2, np.uint8, None), (None, 3, np.int16, None), (None, 4, np.float32, None), (None, 1, np.uint8, None)]
CASES += [(f, 3, np.uint8, v) for f in ("nv12", "i420") for v in E.VARIANTS]


def case_id(case):
    fmt, c, dtype, variant = case
    return f"{fmt}-{np.dtype(dtype).name}x{c}" + (f"-{variant[0]}-{variant[1]}" if variant else "")


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_every_format_equals_the_contract(gpu_ctx, case):
    """every size x source (whole image: words; crop view at an odd x: bytes) x target (out=None; foreign memory with aligned base and
    pitch: words; 2 mod 4: the 16-bit chroma stores of i420; odd base and pitch: bytes) as ONE list, one launch; bgra / rgba with a mask
    as alpha on every second item.  After it every foreign allocation is read back whole: not one byte outside the planes' rows changed."""
    fmt, c, dtype, variant = case
    matrix, range_ = variant or ("bt709", "limited")
    rng = np.random.default_rng(41)
    images, alphas, outs, wants, arenas = [], [], [], [], []
    for h, w in SIZES:
        for crop in (False, True):
            for mode in (None, "words", "halves", "bytes"):
                a = source(rng, h, w, c, dtype)
                m = source(rng, h, w, 1) if fmt in ("bgra", "rgba") and len(images) % 2 else None
                want = E.from_bgr(a, fmt, matrix, range_, alpha=m)
                arena = None if mode is None else Arena(gpu_ctx, want, mode)
                images.append(upload(gpu_ctx, a, crop))
                alphas.append(None if m is None else upload(gpu_ctx, m, crop))
                outs.append(None if arena is None else arena.targets)
                wants.append(want)
                arenas.append(arena)
    got = S.emit_all(images, fmt, out=outs, alpha=alphas, matrix=matrix, range=range_, ctx=gpu_ctx)
    assert len(got) == len(wants)
    for g, want, arena, target in zip(got, wants, arenas, outs):
        if arena is None:
            assert same_planes(g, want), (fmt, planes_of(want)[0].shape)
        else:
            assert g is target  # written in place, the same objects come back
            arena.check(want)
    # one image on its own, both ways
    assert same_planes(S.emit(images[-1], fmt, alpha=alphas[-1], matrix=matrix, range=range_, ctx=gpu_ctx), wants[-1])
    arena = Arena(gpu_ctx, wants[-1], "bytes")
    assert S.emit(images[-1], fmt, out=arena.targets, alpha=alphas[-1], matrix=matrix, range=range_, ctx=gpu_ctx) is arena.targets
    arena.check(wants[-1])


def test_single_contiguous_nv12_target(gpu_ctx):
    rng = np.random.default_rng(3)
    a = source(rng, 6, 8)
    y, uv = E.from_bgr(a, "nv12")
    whole = np.concatenate([y, uv.reshape(3, 8)], axis=0)  # (H * 3 / 2) x W
    dev = S.DeviceImage.from_numpy(np.full((1, 9 * 8 + 32), FILL, np.uint8), gpu_ctx)
    target = Foreign(dev, dev.device_ptr() + 16, (9, 8), None)
    assert S.emit(S.DeviceImage.from_numpy(a, gpu_ctx), "nv12", out=target, ctx=gpu_ctx) is target
    got = dev.numpy().reshape(-1)
    assert np.array_equal(got[16:16 + 72].reshape(9, 8), whole) and np.all(got[:16] == FILL) and np.all(got[16 + 72:] == FILL)


# ---- alpha ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["bgra", "rgba"])
def test_alpha_is_the_mask_or_255(gpu_ctx, fmt):
    rng = np.random.default_rng(43)
    a, m = source(rng, 11, 263), source(rng, 11, 263, 1)
    da, dm = S.DeviceImage.from_numpy(a, gpu_ctx), S.DeviceImage.from_numpy(m, gpu_ctx)
    with_mask, without = S.emit(da, fmt, alpha=dm, ctx=gpu_ctx).numpy(), S.emit(da, fmt, ctx=gpu_ctx).numpy()
    assert np.array_equal(with_mask, E.from_bgr(a, fmt, alpha=m)) and np.array_equal(with_mask[..., 3], m)
    assert np.array_equal(without, E.from_bgr(a, fmt)) and np.all(without[..., 3] == 255)
    assert np.array_equal(with_mask[..., :3], a if fmt == "bgra" else a[..., ::-1])


# ---- the arithmetic, exhaustively -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def every_colour(gpu_ctx):
    """A 4096 x 4096 BGR image that enumerates all 2^24 (B, G, R): pixel p = y * 4096 + x holds (p & 255, (p >> 8) & 255, p >> 16).
    Uploaded once.  Its 2 x 2 blocks pair B with B + 1 and G with G + 16 — the sums the enumeration makes."""
    p = np.arange(1 << 24, dtype=np.uint32).reshape(4096, 4096)
    a = np.stack([p & 255, (p >> 8) & 255, p >> 16], axis=-1).astype(np.uint8)
    return a, S.DeviceImage.from_numpy(a, gpu_ctx)


@pytest.mark.parametrize("matrix,range_", E.VARIANTS)
def test_arithmetic_exhaustively(gpu_ctx, every_colour, matrix, range_):
    """the luma of every colour; the chroma of the blocks the enumeration makes"""
    a, dev = every_colour
    y, uv = S.emit(dev, "nv12", matrix=matrix, range=range_, ctx=gpu_ctx)
    want_y, want_uv = E.from_bgr(a, "nv12", matrix, range_)
    assert same(y, want_y)
    assert same(uv, want_uv)


@pytest.mark.parametrize("fmt", ["nv12", "i420"])
def test_block_sums_at_their_ends(gpu_ctx, fmt):
    """blocks whose sums are 0, 1020 in every channel and 1020 in one channel alone: B alone is the one chroma that clips (U = 256 in
    full range), and an odd width and height put single-channel 1020 sums into replicated edge blocks as well"""
    colours = [(0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255)]
    a = np.zeros((5, 2 * len(colours) + 1, 3), np.uint8)
    for k, colour in enumerate(colours):
        a[:, 2 * k:2 * k + 2] = colour
    a[:, -1] = (255, 0, 0)  # the odd last column: a replicated block of pure blue
    s = E.block_sums(a)
    assert {tuple(v) for v in s.reshape(-1, 3)} >= {(0, 0, 0), (1020, 1020, 1020), (1020, 0, 0), (0, 1020, 0), (0, 0, 1020)}
    dev = S.DeviceImage.from_numpy(a, gpu_ctx)
    for matrix, range_ in E.VARIANTS:
        want = E.from_bgr(a, fmt, matrix, range_)
        if range_ == "full":
            assert want[1][0, 2].reshape(-1)[0] == 255 and int(E.coefficients(matrix, range_)[1][0]) * 1020 + 131072 >> 18 == 128  # 256 clipped
        assert same_planes(S.emit(dev, fmt, matrix=matrix, range=range_, ctx=gpu_ctx), want), (fmt, matrix, range_)


# ---- one launch for a list --------------------------------------------------------------------------------------------------------------
def test_one_launch_for_a_list_of_unequal_items(gpu_ctx):
    rng = np.random.default_rng(7)
    hosts = [source(rng, 37, 301), source(rng, 9, 700), source(rng, 5, 3), source(rng, 20, 33, 1)]
    mask = source(rng, 9, 700, 1)
    formats = ["nv12", "bgra", "i420", None]
    wants = [E.from_bgr(hosts[0], "nv12", "bt601", "full"), E.from_bgr(hosts[1], "bgra", alpha=mask), E.from_bgr(hosts[2], "i420", "bt601", "full"),
             hosts[3]]
    arenas = [Arena(gpu_ctx, wants[0], "words"), None, Arena(gpu_ctx, wants[2], "bytes"), None]
    images = [upload(gpu_ctx, a, crop) for a, crop in zip(hosts, (False, True, False, True))]
    dmask = upload(gpu_ctx, mask, False)
    gpu_ctx.sync()
    gpu_ctx.prof_enable()
    gpu_ctx.prof_reset()
    try:
        outs = S.emit_all(images, formats, out=[None if a is None else a.targets for a in arenas], alpha=[None, dmask, None, None],
                          matrix="bt601", range="full", ctx=gpu_ctx)
        launched = [(r["kernel"], r["calls"]) for r in gpu_ctx.prof_results() if r["calls"]]
    finally:
        gpu_ctx.prof_enable(False)
    assert launched == [("emit", 1)]
    for out, want, arena in zip(outs, wants, arenas):
        if arena is None:
            assert same_planes(out, want)
        else:
            arena.check(want)


# ---- round trips ------------------------------------------------------------------------------------------------------------------------
def test_device_round_trip_through_ingest(gpu_ctx):
    rng = np.random.default_rng(47)
    hosts = [source(rng, 37, 53), source(rng, 8, 260)]
    images = [S.DeviceImage.from_numpy(a, gpu_ctx) for a in hosts]
    for fmt in ("nv12", "i420"):
        back = S.ingest_all(S.emit_all(images, fmt, ctx=gpu_ctx), fmt, ctx=gpu_ctx)
        for a, b in zip(hosts, back):
            assert same(b, N.to_bgr(E.from_bgr(a, fmt), fmt))
    for fmt in ("rgb", "bgra", "rgba", "bgr"):  # the packed formats come back exactly
        back = S.ingest_all(S.emit_all(images, fmt, ctx=gpu_ctx), fmt, ctx=gpu_ctx)
        assert all(same(b, a) for a, b in zip(hosts, back))


def test_panorama_of_a_stitch_job(gpu_ctx):
    n, w, h = 2, 64, 48
    cams = synthetic.ring_cameras(n, w, h, focal_factor=0.75, span_deg=90.0)
    pano, mask = S.pipeline.StitchJob(synthetic.make_frames(range(0, n), w, h), cams, ctx=gpu_ctx).run()
    hp, hm = np.asarray(pano), np.asarray(mask)
    assert hp.ndim == 3 and hp.dtype == np.uint8 and hm.shape == hp.shape[:2] and hp.shape[0] >= 20 and hp.shape[1] >= 40 and np.count_nonzero(hm)
    assert same_planes(S.emit(pano, "nv12", ctx=gpu_ctx), E.from_bgr(hp, "nv12"))
    assert same(S.emit(pano, "bgra", alpha=mask, ctx=gpu_ctx), E.from_bgr(hp, "bgra", alpha=hm))
    want = E.from_bgr(hp, "nv12")
    surface = Arena(gpu_ctx, want, "words")
    S.emit(pano, "nv12", out=surface.targets, ctx=gpu_ctx)
    surface.check(want)
    crop = E.from_bgr(hp[3:20, 5:40], "rgba", alpha=hm[3:20, 5:40])
    assert same(S.emit(pano[3:20, 5:40], "rgba", alpha=mask[3:20, 5:40], ctx=gpu_ctx), crop)


# ---- ordering arguments -----------------------------------------------------------------------------------------------------------------
def test_stream_and_wait_arguments_give_the_same_bytes(gpu_ctx):
    """the legacy default stream as the consumer's (argument and the target's own entry), wait=False followed by ctx.sync(); no race is
    staged"""
    rng = np.random.default_rng(9)
    a = source(rng, 21, 130)
    dev = S.DeviceImage.from_numpy(a, gpu_ctx)
    want = E.from_bgr(a, "nv12", "bt601", "limited")
    kw = dict(matrix="bt601", range="limited", ctx=gpu_ctx)
    for stream_arg, entry in ((1, "absent"), (None, 1), (None, None), (1, 77)):  # stream= overrides the entry
        arena = Arena(gpu_ctx, want, "words", stream=entry)
        S.emit(dev, "nv12", out=arena.targets, stream=stream_arg, **kw)
        arena.check(want)
    assert same_planes(S.emit(dev, "nv12", stream=1, **kw), want)
    arena = Arena(gpu_ctx, want, "bytes")
    S.emit(dev, "nv12", out=arena.targets, wait=False, **kw)
    planes = S.emit(dev, "nv12", wait=False, **kw)
    gpu_ctx.sync()
    arena.check(want)
    assert same_planes(planes, want)


# ---- refusals: decided on the host, nothing is launched, the context works afterwards ---------------------------------------------------
def raw_emit(ctx, src, fmt, planes, alpha=None):
    """stx_emit itself, past the checks of the Python layer; planes: [(pointer, pitch)] -> (status, message)"""
    item = (_lib.EmitItem * 1)()
    item[0].src, item[0].alpha, item[0].format, item[0].has_target = src._h.value, None if alpha is None else alpha._h.value, fmt, 1
    for k, (ptr, pitch) in enumerate(planes):
        item[0].plane[k], item[0].pitch[k] = ptr, pitch
    out = (C.c_void_p * 3)()
    rc = ctx._lib.stx_emit(ctx.handle, 1, item, 1, 0, None, 0, out)
    assert not any(out)
    return rc, ctx._lib.stx_last_error().decode()


def test_refusals(gpu_ctx):
    rng = np.random.default_rng(19)
    a = source(rng, 8, 10)
    src = S.DeviceImage.from_numpy(a, gpu_ctx)
    want = E.from_bgr(a, "nv12")
    arena = Arena(gpu_ctx, want, "words")
    (py, ypitch), (puv, uvpitch) = [(arena.dev.device_ptr() + off, pitch) for off, pitch in arena.spans]
    host = np.zeros((8, 30), np.uint8)
    pinned = S.pinned_empty((8, 30))
    fmt = _lib.INGEST_FORMATS
    gpu_ctx.sync()
    gpu_ctx.prof_enable()
    gpu_ctx.prof_reset()
    try:
        for h in (host, pinned):  # host pointers: pageable and page-locked
            rc, msg = raw_emit(gpu_ctx, src, fmt["bgr"], [(h.ctypes.data, 30)])
            assert rc == -1 and "item 0 plane 0" in msg and "host memory" in msg
            with pytest.raises(S.StitchingError, match="host memory"):
                S.emit(src, "bgr", out=Foreign(h, h.ctypes.data, (8, 10, 3), None), ctx=gpu_ctx)
        # a plane whose last byte lies beyond its allocation: the last row of the UV plane, by its pitch
        rc, msg = raw_emit(gpu_ctx, src, fmt["nv12"], [(py, ypitch), (puv, 1 << 38)])
        assert rc == -1 and "item 0 plane 1" in msg and "its allocation holds" in msg
        # a pitch below the row bytes
        rc, msg = raw_emit(gpu_ctx, src, fmt["nv12"], [(py, 9), (puv, uvpitch)])
        assert rc == -1 and "item 0 plane 0" in msg and "pitch" in msg
        rc, msg = raw_emit(gpu_ctx, src, fmt["nv12"], [(py, ypitch), (puv, 9)])
        assert rc == -1 and "item 0 plane 1" in msg and "pitch" in msg
        # two target planes that overlap: the UV plane inside the Y plane's last row
        rc, msg = raw_emit(gpu_ctx, src, fmt["nv12"], [(py, ypitch), (py + 7 * ypitch + 4, uvpitch)])
        assert rc == -1 and "item 0 plane 0 overlaps item 0 plane 1" in msg
        # a target that overlaps its source, and one that overlaps the alpha image
        rc, msg = raw_emit(gpu_ctx, src, fmt["rgb"], [(src.device_ptr(), src.stride_bytes)])
        assert rc == -1 and "overlaps the source image of item 0" in msg
        with pytest.raises(S.StitchingError, match="overlaps the source"):
            S.emit(src, "rgb", out=Foreign(src, src.device_ptr(), (8, 10, 3), (src.stride_bytes, 3, 1)), ctx=gpu_ctx)
        mask = S.DeviceImage.from_numpy(source(rng, 8, 40, 1), gpu_ctx)
        rc, msg = raw_emit(gpu_ctx, src, fmt["bgra"], [(mask.device_ptr(), mask.stride_bytes)], alpha=mask[:, :10])
        assert rc == -1 and "overlaps the alpha image of item 0" in msg
        # an alpha of the wrong size, an alpha for a format without one, a source the format is not made from
        rc, msg = raw_emit(gpu_ctx, src, fmt["bgra"], [(py, 40)], alpha=mask)
        assert rc == -1 and "alpha image is u8x1 of 10x8" in msg
        rc, msg = raw_emit(gpu_ctx, src, fmt["bgr"], [(py, 30)], alpha=mask[:, :10])
        assert rc == -1 and "has no alpha" in msg
        rc, msg = raw_emit(gpu_ctx, mask, fmt["nv12"], [(py, 40), (puv, 40)])
        assert rc == -1 and "channel" in msg
        rc, msg = raw_emit(gpu_ctx, src, fmt["nv12"], [(py, ypitch)])  # the UV plane is missing
        assert rc == -1 and "item 0 plane 1 is null" in msg
        launched = [r["kernel"] for r in gpu_ctx.prof_results() if r["calls"]]
    finally:
        gpu_ctx.prof_enable(False)
    assert launched == []
    arena.check((np.full_like(want[0], FILL), np.full_like(want[1], FILL)))  # nothing was written
    S.emit(src, "nv12", out=arena.targets, ctx=gpu_ctx)  # the context is usable
    arena.check(want)
