"""stx_resize_linear_exact_batch: n images of unequal sizes in one launch are byte for byte n calls of stx_resize_linear_exact, and the
CPU oracle's cv::resize(INTER_LINEAR_EXACT).  The shapes are small on purpose: what can break is the flat tile list (an image with fewer
destination pixels than one 64 x 4 tile, images whose tiles fill their rectangle exactly, the last tile of one image next to the first of
the next), the per-image channel count, and the pitch of a view."""
import ctypes as C

import numpy as np
import pytest

import stitching_amd as S
from stitching_amd import _lib
from stitching_amd.seam_finder import resize_linear_exact, resize_linear_exact_all

# (source w, h, channels, view (x, y, w, h) or None, destination w, h)
CASES = [
    (37, 29, 1, None, 13, 11),            # non-integer downscale
    (64, 48, 3, None, 17, 9),             # different x and y factors
    (20, 15, 1, None, 33, 27),            # upscale
    (1, 1, 3, None, 5, 3),                # degenerate source, less than one tile
    (300, 7, 1, None, 3, 7),              # wide source
    (50, 40, 3, (7, 5, 31, 23), 16, 12),  # pitched view
    (40, 30, 3, None, 128, 8),            # exactly 2 x 2 tiles
]
BATCHES = {"one": [5], "one_tile": [3], "two": [6, 3], "two_swapped_channels": [2, 1], "seven": [0, 1, 2, 3, 4, 5, 6],
           "exact_tiles": [6, 6]}


@pytest.fixture(scope="module")
def sources():
    rng = np.random.default_rng(20260101)
    out = []
    for w, h, c, view, dw, dh in CASES:
        a = rng.integers(0, 256, (h, w) if c == 1 else (h, w, c), dtype=np.uint8)
        out.append(a)
    return out


def _device_source(k, host, ctx):
    d = S.DeviceImage.from_numpy(host, ctx)
    view = CASES[k][3]
    if view is None:
        return d, host
    x, y, w, h = view
    v = d[y:y + h, x:x + w]
    assert v.stride_bytes == d.stride_bytes and (v.width, v.height) == (w, h)  # a view: the parent's pitch
    return v, host[y:y + h, x:x + w]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(BATCHES))
def test_batch_equals_single_calls_and_the_oracle(oracle, gpu_ctx, sources, name):
    ks = BATCHES[name]
    dev, host = zip(*[_device_source(k, sources[k], gpu_ctx) for k in ks])
    sizes = [CASES[k][4:6] for k in ks]
    got = resize_linear_exact_all(list(dev), sizes, ctx=gpu_ctx, device_resident=True)
    assert len(got) == len(ks) and all(isinstance(g, S.DeviceImage) for g in got)
    for k, d, h, size, g in zip(ks, dev, host, sizes, got):
        g = g.numpy()
        assert g.shape[:2] == (size[1], size[0]) and g.dtype == np.uint8 and g.ndim == h.ndim
        one = resize_linear_exact(d, size, ctx=gpu_ctx, device_resident=False)
        assert np.array_equal(g, one), f"case {k}: the batch differs from stx_resize_linear_exact"
        assert np.array_equal(g, oracle.resize_linear_exact(np.ascontiguousarray(h), size)), f"case {k}: differs from the oracle"


@pytest.mark.gpu
def test_host_arrays_and_numpy_results(oracle, gpu_ctx, sources):
    got = resize_linear_exact_all([sources[0], sources[1]], [(13, 11), (17, 9)], ctx=gpu_ctx, device_resident=False)
    assert all(isinstance(g, np.ndarray) for g in got)
    assert np.array_equal(got[0], oracle.resize_linear_exact(sources[0], (13, 11)))
    assert np.array_equal(got[1], oracle.resize_linear_exact(sources[1], (17, 9)))


@pytest.mark.gpu
def test_images_resize_takes_the_batch_for_a_list(oracle, gpu_ctx):
    """device residency + a list: Images.resize stays a generator and yields what the per-image path yields"""
    rng = np.random.default_rng(7)
    frames = [rng.integers(0, 256, (300, 400, 3), dtype=np.uint8) for _ in range(3)]
    images = S.Images.of(frames, 0.6, 0.01, -1)
    S.set_device_resident(True)
    try:
        medium = list(images.resize(S.Images.Resolution.MEDIUM))
        gen = images.resize(S.Images.Resolution.LOW, medium)
        assert hasattr(gen, "__next__")
        low = list(gen)
    finally:
        S.set_device_resident(False)
    sizes = images.get_scaled_img_sizes(S.Images.Resolution.LOW)
    assert all(isinstance(a, S.DeviceImage) for a in low) and sizes[0] != (400, 300)
    for a, f, size in zip(low, frames, sizes):
        assert np.array_equal(a.numpy(), oracle.resize_linear_exact(f, size))


def _raw(ctx, handles, wh):
    n = len(handles)
    outs = (C.c_void_p * max(n, 1))()
    q = np.ascontiguousarray(np.asarray(wh, np.int32).reshape(-1))
    rc = ctx._lib.stx_resize_linear_exact_batch(ctx.handle, n, (C.c_void_p * max(n, 1))(*handles), q.ctypes.data_as(C.POINTER(C.c_int)), outs)
    return rc, (ctx._lib.stx_last_error() or b"").decode(), outs


@pytest.mark.gpu
def test_argument_checks(gpu_ctx):
    ok = S.DeviceImage.from_numpy(np.zeros((6, 8, 3), np.uint8), gpu_ctx)
    rc, msg, _ = _raw(gpu_ctx, [], [1, 1])
    assert rc == -1 and "0 images" in msg  # STX_ERR_INVALID
    with pytest.raises(S.StitchingError):
        resize_linear_exact_all([], [], ctx=gpu_ctx)
    f32 = S.DeviceImage.from_numpy(np.zeros((6, 8), np.float32), gpu_ctx)
    two = S.DeviceImage.from_numpy(np.zeros((6, 8, 2), np.uint8), gpu_ctx)
    for bad in (f32, two):
        rc, msg, outs = _raw(gpu_ctx, [ok._h, bad._h], [4, 3, 4, 3])
        assert rc == -5 and msg == "resize needs a u8x1 or u8x3 image" and not outs[0] and not outs[1]  # STX_ERR_UNSUPPORTED, nothing handed out
    for wh in ([4, 3, 0, 3], [4, 3, 4, -1]):
        rc, msg, outs = _raw(gpu_ctx, [ok._h, ok._h], wh)
        assert rc == -1 and msg == f"resize to {wh[2]}x{wh[3]}" and not outs[0]
    rc, msg, _ = _raw(gpu_ctx, [ok._h, None], [4, 3, 4, 3])
    assert rc == -1 and msg == "null argument"
    with pytest.raises(S.StitchingError, match="one size per image"):
        resize_linear_exact_all([ok], [(4, 3), (2, 2)], ctx=gpu_ctx)
    # the same codes and messages as the single-image entry point
    out = C.c_void_p()
    assert gpu_ctx._lib.stx_resize_linear_exact(gpu_ctx.handle, f32._h, 4, 3, C.byref(out)) == -5
    assert gpu_ctx._lib.stx_last_error().decode() == "resize needs a u8x1 or u8x3 image"
    assert _lib.STX_OK == 0
