"""The constructed resize families (tests/constructed_resizes.py) on the device: every case of every family gives 0 differing bytes
against the numpy contract (tests/numpy_resize.py) and against the CPU oracle, on the kernel path `expected_path` names for it —
stx_debug_seam_resize_paths (include/stitching_amd_debug.h) counts the images each path launched, and its increase over a call must be
what the construction says, image by image.  Batched calls equal the per-image calls, rectangles (sub) equal the rectangle of the
whole result, and the parent image around a view is unchanged after the call.

What the families separate is shown without a GPU in tests/test_constructed_resizes.py.  Every input here is a valid call: nothing
provokes a fault."""
import ctypes as C

import numpy as np
import pytest

import stitching_amd as S
from stitching_amd.seam_finder import SeamFinder, resize_linear_exact, resize_linear_exact_all
from tests import constructed_resizes as CR
from tests import numpy_resize as NR

pytestmark = pytest.mark.gpu


def _counts(ctx):
    out = (C.c_int * 4)()
    assert ctx._lib.stx_debug_seam_resize_paths(ctx.handle, out) == 0
    return list(out)


def _upload(ctx, f):
    """-> (parent on the device, the view of it): the view's pointer and pitch are what expected_path assumes"""
    parent = S.DeviceImage.from_numpy(f.parent, ctx)
    view = parent if f.whole else parent[f.y:f.y + f.h, f.x:f.x + f.w]
    assert view.shape == (f.h, f.w) and view.stride_bytes == CR.buf_pitch(f.parent.shape[1])
    assert view.device_ptr() % 8 == f.x % 8 and parent.device_ptr() % CR.BUF_PITCH == 0
    return parent, view


def _run(ctx, c):
    """-> (results as numpy, the counter's increase over the call); asserts that no parent image changed"""
    pairs = [_upload(ctx, f) for f in c["finals"]]
    lows = [S.DeviceImage.from_numpy(low, ctx) for low in c["lows"]]
    views = [v for _, v in pairs]
    before = _counts(ctx)
    out = SeamFinder.resize_all(lows, views, sub=c["sub"]) if c["batch"] else [SeamFinder.resize(lows[0], views[0])]
    after = _counts(ctx)
    got = [np.asarray(o) for o in out]
    for (parent, _), f in zip(pairs, c["finals"]):
        assert np.array_equal(parent.numpy(), f.parent), c["name"]
    for low, a in zip(lows, c["lows"]):
        assert np.array_equal(low.numpy(), a), c["name"]
    return got, [b - a for a, b in zip(before, after)]


def _oracle(oracle, c):
    out = []
    for i, (low, f) in enumerate(zip(c["lows"], c["finals"])):
        if c["sub"] is None:
            out.append(oracle.seam_resize(low, f.array))
        else:
            fw, fh, x0, y0 = c["sub"][i]
            full = np.full((fh, fw), 255, np.uint8)
            full[y0:y0 + f.h, x0:x0 + f.w] = f.array
            out.append(oracle.seam_resize(low, full)[y0:y0 + f.h, x0:x0 + f.w])
    return out


def _differing(a, b):
    assert len(a) == len(b) and all(x.shape == y.shape and x.dtype == y.dtype for x, y in zip(a, b))
    return sum(int(np.count_nonzero(x != y)) for x, y in zip(a, b))


@pytest.mark.parametrize("family", sorted(CR.SEAM_FAMILIES))
def test_family_on_its_paths(oracle, gpu_ctx, family):
    for c in CR.SEAM_FAMILIES[family]():
        want = CR.want(c)
        assert _differing(want, _oracle(oracle, c)) == 0, c["name"]
        got, moved = _run(gpu_ctx, c)
        assert _differing(got, want) == 0, (c["name"], CR.expected_path(c))
        assert moved == CR.expected_counts(c), (c["name"], CR.expected_path(c), dict(zip(CR.COUNTERS, moved)))
        if not c["batch"]:
            continue
        if c["sub"] is None:  # the batched call equals the per-image calls, each on its own path
            for i in range(len(c["lows"])):
                one = CR.single(c, i)
                got1, moved1 = _run(gpu_ctx, one)
                assert np.array_equal(got1[0], got[i]), one["name"]
                assert moved1 == CR.expected_counts(one), (one["name"], dict(zip(CR.COUNTERS, moved1)))
        else:  # the rectangle of the whole result: the seam mask enlarged to the full size under a full mask of 255
            for i, (low, f) in enumerate(zip(c["lows"], c["finals"])):
                fw, fh, x0, y0 = c["sub"][i]
                whole = np.asarray(SeamFinder.resize(low, np.full((fh, fw), 255, np.uint8)))
                assert np.array_equal(whole[y0:y0 + f.h, x0:x0 + f.w] & f.array, got[i]), (c["name"], i)


def test_every_path_is_reached_on_the_device(gpu_ctx):
    """one case per answer of expected_path, by the counter alone"""
    first = {}
    for make in CR.SEAM_FAMILIES.values():
        for c in make():
            first.setdefault(CR.expected_path(c), c)
    mixed = next(c for c in CR.view_offsets() if c["name"] == "one odd view among aligned")
    first["per_image_fallback"] = mixed
    assert set(first) == set(CR.PATHS)
    seen = [0, 0, 0, 0]
    for path, c in first.items():
        _, moved = _run(gpu_ctx, c)
        assert moved == CR.expected_counts(c), (path, c["name"], moved)
        seen = [a + b for a, b in zip(seen, moved)]
    assert all(seen), dict(zip(CR.COUNTERS, seen))
    # the fallback sends each image down its own path; the copy of an odd rectangle makes it fit for the LDS kernel
    assert CR.expected_counts(mixed) == [4, 0, 0, 1]
    assert CR.expected_counts(first["aligned_copy_then_lds"]) == [len(first["aligned_copy_then_lds"]["lows"]), 0, 0, 0]


@pytest.mark.parametrize("kind", ("ties", "knife_edges"))
def test_coefficient_images(oracle, gpu_ctx, kind):
    """the same sizes through the image resize, singly (host tables) and batched (coefficients made in the kernel), 1 and 3 channels"""
    imgs, sizes = [], []
    for src_n, dst_n, col, axis in CR.coefficient_cases(kind):
        for ch in (1, 3):
            img, size = CR.coefficient_image(src_n, dst_n, col, axis, ch)
            imgs.append(img)
            sizes.append(size)
    want = [NR.resize_linear_exact(a, s) for a, s in zip(imgs, sizes)]
    assert _differing(want, [oracle.resize_linear_exact(a, s) for a, s in zip(imgs, sizes)]) == 0
    before = _counts(gpu_ctx)
    one = [np.asarray(resize_linear_exact(a, s, gpu_ctx)) for a, s in zip(imgs, sizes)]
    many = [np.asarray(o) for o in resize_linear_exact_all(imgs, sizes, gpu_ctx)]
    assert _counts(gpu_ctx) == before  # image resizes are no seam masks
    for k, (a, b, w) in enumerate(zip(one, many, want)):
        assert np.array_equal(a, w) and np.array_equal(b, w), (kind, k, sizes[k])


def test_image_batches(oracle, gpu_ctx):
    """the batch kernel's flat tile list: tile edges, 1 to 40 images, a 1 x 1 destination between multi-tile ones, 1 and 3 channels
    alternating, pitched views as sources"""
    for name, srcs, sizes, _ in CR.image_batches():
        parents = [S.DeviceImage.from_numpy(a, gpu_ctx) for a, *_ in srcs]
        dev = [p[y:y + h, x:x + w] for p, (_, x, y, w, h) in zip(parents, srcs)]
        arrays = [CR.source_array(s) for s in srcs]
        want = [NR.resize_linear_exact(a, s) for a, s in zip(arrays, sizes)]
        assert _differing(want, [oracle.resize_linear_exact(a, s) for a, s in zip(arrays, sizes)]) == 0
        many = [np.asarray(o) for o in resize_linear_exact_all(dev, sizes, gpu_ctx)]
        one = [np.asarray(resize_linear_exact(d, s, gpu_ctx)) for d, s in zip(dev, sizes)]
        assert _differing(many, want) == 0 and _differing(one, want) == 0, name
        for p, (a, *_) in zip(parents, srcs):
            assert np.array_equal(p.numpy(), a)


def test_a_refused_batch_hands_nothing_out(gpu_ctx):
    """A batch without sub of aligned masks and an odd-offset view (the per-image route) whose third seam mask is a u8x3 image: the call
    returns its error, `outs` stays all null, no kernel is launched, and the context goes on working.  (The entry checks look at every
    image before the first per-image call is made, so this is refused there; the unwinding inside the per-image loop can only be
    entered when an allocation fails half way.)"""
    mixed = next(c for c in CR.view_offsets() if c["name"] == "one odd view among aligned")
    assert CR.expected_path(mixed) == "per_image_fallback"
    pairs = [_upload(gpu_ctx, f) for f in mixed["finals"]]
    lows = [S.DeviceImage.from_numpy(low, gpu_ctx) for low in mixed["lows"]]
    lows[2] = S.DeviceImage.from_numpy(np.zeros(mixed["lows"][2].shape + (3,), np.uint8), gpu_ctx)
    n = len(lows)
    sa, ma, outs = (C.c_void_p * n)(*[a._h for a in lows]), (C.c_void_p * n)(*[v._h for _, v in pairs]), (C.c_void_p * n)()
    before = _counts(gpu_ctx)
    rc = gpu_ctx._lib.stx_seam_mask_resize_batch(gpu_ctx.handle, n, sa, ma, outs)
    assert rc == -1 and b"u8x1" in gpu_ctx._lib.stx_last_error()
    assert [outs[i] for i in range(n)] == [None] * n and _counts(gpu_ctx) == before
    got, moved = _run(gpu_ctx, mixed)
    assert _differing(got, CR.want(mixed)) == 0 and moved == [4, 0, 0, 1]
