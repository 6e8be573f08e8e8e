"""Source validity masks on the device: a frame that carries a mask (S.with_validity, `source_masks=`) gets the nearest-neighbour warp of
that mask instead of a warped rectangle.  Every constructed warp case (tests/constructed_warps.py) and the rounding family
(tests/constructed_source_masks.py) through S.Warper(...).warp_images_and_masks(..., rects=, source_masks=) against
oracle.remap_nearest(mask, *oracle.build_maps(rect)): 0 differing bytes, no tolerance, with the hash and the binary mask, as image + mask
and as mask only, under each case's own remap model.  The image equals the call without a mask byte for byte; source and mask read back
unmodified.  Then mixed batches, a pitched mask view, the per-pixel projectors, the C handles and their refusals, and the shrink."""
import ctypes as C

import numpy as np
import pytest

import stitching_amd as S
from stitching_amd import _lib, synthetic
from tests import constructed_source_masks as CM
from tests import constructed_warps as CW
from tests import numpy_source_masks as NS

pytestmark = pytest.mark.gpu

STX_ERR_INVALID = -1
_maps, _plain, _dev_src, _dev_mask = {}, {}, {}, {}


class _Model:
    """the remap model of a case on both sides, the previous ones back afterwards"""

    def __init__(self, oracle, mode):
        self.oracle, self.mode = oracle, mode

    def __enter__(self):
        self.prev_p, self.prev_o = S.remap_mode(), self.oracle.set_model()
        S.set_remap_mode(self.mode.replace("_", "-"))
        self.oracle.set_model(**{**self.prev_o, "remap": self.mode})

    def __exit__(self, *exc):
        S.set_remap_mode(self.prev_p)
        self.oracle.set_model(**self.prev_o)


def maps(oracle, case):
    if case.name not in _maps:
        _maps[case.name] = oracle.build_maps(case.warper_type, case.scale, case.K, case.R, case.rect)
    return _maps[case.name]


def want_mask(oracle, case, pattern):
    """the reference: the oracle's nearest remap of the mask (None: of a 255 image) over the oracle's maps of the rectangle"""
    m = np.full((case.size[1], case.size[0]), 255, np.uint8) if pattern is None else CM.mask(pattern, case.size)
    return oracle.remap_nearest(m, *maps(oracle, case))


def dev_source(size, ctx):
    if size not in _dev_src:
        _dev_src[size] = S.as_device(np.ascontiguousarray(CW.source(*size)), ctx)
    return _dev_src[size]


def dev_mask(pattern, size, ctx):
    if (pattern, size) not in _dev_mask:
        _dev_mask[(pattern, size)] = S.as_device(np.ascontiguousarray(CM.mask(pattern, size)), ctx)
    return _dev_mask[(pattern, size)]


def device_warp(cases, patterns, ctx, images=True):
    """one call for `cases` (one warper type, scale and remap model), patterns[i]: the mask pattern of image i or None -> (imgs, masks)"""
    c0 = cases[0]
    assert all((c.warper_type, c.scale, c.model) == (c0.warper_type, c0.scale, c0.model) for c in cases)
    g = S.Warper(c0.warper_type, ctx=ctx)
    g.scale = c0.scale
    srcs = [dev_source(c.size, ctx) for c in cases]
    sm = None if all(p is None for p in patterns) else [None if p is None else dev_mask(p, c.size, ctx) for c, p in zip(cases, patterns)]
    Ks, Rs = np.stack([c.K for c in cases]), np.stack([c.R for c in cases])
    imgs, masks, rects = g.warp_images_and_masks(srcs, [None] * len(cases), rects=[c.rect for c in cases], camera_arrays=(Ks, Rs),
                                                 source_masks=sm, images=images)
    assert [tuple(r) for r in rects] == [c.rect for c in cases]
    return (None if imgs is None else [np.asarray(i) for i in imgs]), [np.asarray(m) for m in masks]


def unmodified(cases, patterns, ctx):
    for size in {c.size for c in cases}:
        assert np.array_equal(dev_source(size, ctx).numpy(), CW.source(*size)), f"{size}: the source was modified"
    for key in {(p, c.size) for c, p in zip(cases, patterns) if p is not None}:
        assert np.array_equal(dev_mask(*key, ctx).numpy(), CM.mask(*key)), f"{key}: the mask was modified"


def plain(case, oracle, ctx):
    """the case warped without a mask, once (read only): what the images must equal"""
    if case.name not in _plain:
        with _Model(oracle, case.model):
            imgs, masks = device_warp([case], [None], ctx)
        _plain[case.name] = (imgs[0], masks[0])
    return _plain[case.name]


@pytest.mark.parametrize("name", list(CM.ALL_CASES))
def test_case_equals_the_oracle(oracle, gpu_ctx, name):
    case = CM.ALL_CASES[name]
    p_img, p_mask = plain(case, oracle, gpu_ctx)
    assert np.array_equal(p_mask, want_mask(oracle, case, None))
    bad = []
    for pattern in CM.PATTERNS:
        want = want_mask(oracle, case, pattern)
        with _Model(oracle, case.model):
            imgs, masks = device_warp([case], [pattern], gpu_ctx)
            _, only = device_warp([case], [pattern], gpu_ctx, images=False)
        di, dm, do = (int(np.count_nonzero(a != b)) if a.shape == b.shape else -1
                      for a, b in ((imgs[0], p_img), (masks[0], want), (only[0], want)))
        print(f"{case.family} {case.name} {pattern}: image {di}, mask {dm}, mask-only {do} differing bytes")
        if di or dm or do:
            bad.append((pattern, di, dm, do))
    unmodified([case], list(CM.PATTERNS), gpu_ctx)
    assert not bad, (case.name, bad)


def batch_cases():
    """the batch list of tests/test_gpu_constructed_warps.py (copied, see there): the plane warper's fixed-point cases of scale 1 in one
    call — launches of refused sources (warp_kernel, image by image), of one narrow rectangle among seven wide ones (flat grid), of equal
    ones (z grid)"""
    cases = [c for c in CW.CASES.values() if (c.warper_type, c.model, c.scale) == ("plane", "q15", 1.0)]
    refused = [c for c in cases if not CW.tuned(c)]
    small = [c for c in cases if CW.tuned(c) and c.rect[2] <= CW.LANES]
    big = [c for c in cases if CW.tuned(c) and c.rect[2] > CW.LANES]
    fill = -len(refused) % CW.BATCH
    out, big = refused + big[:fill], big[fill:]
    mixed = min(len(small), (len(big) - 2 * CW.BATCH) // 7)
    for k, s in enumerate(small[:mixed]):
        seven = big[7 * k:7 * k + 7]
        out += seven[:k % CW.BATCH] + [s] + seven[k % CW.BATCH:]
    return out + big[7 * mixed:] + small[mixed:]


@pytest.mark.parametrize("images", [True, False])
@pytest.mark.parametrize("phase", [0, 1])
def test_mixed_batch(oracle, gpu_ctx, phase, images):
    """every other image without a mask (phase: which half), the others alternating between the two patterns; refused sources among
    them: launches where only some images carry a mask, where none does, and warp_kernel launches with a mask beside the source"""
    cases = batch_cases()
    refused = [i for i, c in enumerate(cases) if not CW.tuned(c)]
    names = list(CM.PATTERNS)
    patterns = [None if i % 2 == phase else names[(i // 2) % 2] for i in range(len(cases))]
    assert len(cases) > 4 * CW.BATCH and refused
    assert any(patterns[i] is not None for i in refused) and any(patterns[i] is None for i in refused)
    imgs, masks = device_warp(cases, patterns, gpu_ctx, images=images)
    bad = []
    for i, (c, p) in enumerate(zip(cases, patterns)):
        if not np.array_equal(masks[i], want_mask(oracle, c, p)) or (images and not np.array_equal(imgs[i], plain(c, oracle, gpu_ctx)[0])):
            bad.append((c.name, p))
    unmodified(cases, patterns, gpu_ctx)
    print(f"mixed batch of {len(cases)} images, {sum(p is not None for p in patterns)} with a mask: {len(bad)} differ")
    assert not bad, bad


@pytest.mark.parametrize("name", ["mask_rounding-x-33_64", "mask_rounding-y-31_64", "mask_ties-9x9", "refused-32768-x-up"])
def test_mask_that_is_a_slice_of_a_wider_one(oracle, gpu_ctx, name):
    """pitch != width and an odd base address: the kernels read the mask through its own pitch (tuned kernel and, for the refused source,
    warp_kernel)"""
    case = CM.ALL_CASES[name]
    wide, off = CM.wide_mask(case.size)
    d_wide = S.as_device(np.ascontiguousarray(wide), gpu_ctx)
    view = d_wide[:, off:off + case.size[0]]
    assert view.stride_bytes == d_wide.stride_bytes != case.size[0] and view.device_ptr() % 2 == 1
    m = wide[:, off:off + case.size[0]]
    want = oracle.remap_nearest(np.ascontiguousarray(m), *maps(oracle, case))
    g = S.Warper(case.warper_type, ctx=gpu_ctx)
    g.scale = case.scale
    for images in (True, False):
        imgs, masks, _ = g.warp_images_and_masks([dev_source(case.size, gpu_ctx)], [None], rects=[case.rect], camera_arrays=(case.K[None], case.R[None]),
                                                 source_masks=[view], images=images)
        assert np.array_equal(np.asarray(masks[0]), want), int(np.count_nonzero(np.asarray(masks[0]) != want))
        if images:
            assert np.array_equal(np.asarray(imgs[0]), plain(case, oracle, gpu_ctx)[0])
    assert np.array_equal(d_wide.numpy(), wide)


PW, PH = 97, 61


@pytest.mark.parametrize("wtype", ["fisheye", "compressedPlaneA2B1", "paniniA2B1", "transverseMercator"])
def test_per_pixel_projectors(oracle, gpu_ctx, wtype):
    """one warper of every group of warp_general_kernel: whole ROIs, a frame with a mask beside one without"""
    cams = synthetic.ring_cameras(3, PW, PH, span_deg=70.0)[:2]
    rng = np.random.default_rng(11)
    frames = [rng.integers(0, 256, (PH, PW, 3), dtype=np.uint8) for _ in cams]
    g = S.Warper(wtype, ctx=gpu_ctx)
    g.set_scale(cams)
    for pattern in CM.PATTERNS:
        m = CM.mask(pattern, (PW, PH))
        imgs, masks, rois = g.warp_images_and_masks(frames, cams, source_masks=[m, None])
        p_imgs, p_masks, p_rois = g.warp_images_and_masks(frames, cams)
        assert rois == p_rois
        for k, cam in enumerate(cams):
            K, R = np.float32(g.get_K(cam)), np.float32(cam.R)
            xm, ym = oracle.build_maps(wtype, float(g.scale), K, R, rois[k])
            want = oracle.remap_nearest(m if k == 0 else np.full((PH, PW), 255, np.uint8), xm, ym)
            assert np.array_equal(np.asarray(masks[k]), want), (wtype, pattern, k, int(np.count_nonzero(np.asarray(masks[k]) != want)))
            assert np.array_equal(np.asarray(imgs[k]), np.asarray(p_imgs[k]))
        assert (np.asarray(masks[0]) != np.asarray(p_masks[0])).any()
        _, only, _ = g.warp_images_and_masks(frames, cams, source_masks=[m, None], images=False)
        assert all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(only, masks))


@pytest.mark.parametrize("wtype", ["spherical", "plane", "stereographic"])
def test_warp_image_and_mask_honours_validity(oracle, gpu_ctx, wtype):
    cam = synthetic.ring_cameras(3, PW, PH, span_deg=70.0)[1]
    rng = np.random.default_rng(12)
    frame = rng.integers(0, 256, (PH, PW, 3), dtype=np.uint8)
    m = CM.mask("hash", (PW, PH))
    g = S.Warper(wtype, ctx=gpu_ctx)
    g.set_scale([cam])
    d = S.as_device(frame, gpu_ctx)
    img0, mask0, roi0 = g.warp_image_and_mask(d, cam)
    img1, mask1, roi1 = g.warp_image_and_mask(S.with_validity(d, m), cam)
    assert roi0 == roi1 and np.array_equal(np.asarray(img0), np.asarray(img1))
    xm, ym = oracle.build_maps(wtype, float(g.scale), np.float32(g.get_K(cam)), np.float32(cam.R), roi1)
    assert np.array_equal(np.asarray(mask1), oracle.remap_nearest(m, xm, ym))
    assert np.array_equal(np.asarray(mask0), oracle.remap_nearest(np.full((PH, PW), 255, np.uint8), xm, ym))
    # everything else reads the pixels and ignores the mask
    assert np.array_equal(np.asarray(g.warp_image(S.with_validity(d, m), cam)), np.asarray(img0))


def buf_flags(img):
    f = C.c_int(-1)
    _lib.check(img.ctx._lib.stx_buf_flags(img._h, C.byref(f)))
    return f.value


def test_warped_mask_is_binary_when_the_source_mask_is(gpu_ctx):
    case = CM.ALL_CASES["mask_rounding-x-33_64"]
    g = S.Warper(case.warper_type, ctx=gpu_ctx)
    g.scale = case.scale
    prev = S.device_resident()
    S.set_device_resident(True)
    try:
        flags = {}
        for pattern in (None, "hash", "binary"):
            sm = None if pattern is None else [dev_mask(pattern, case.size, gpu_ctx)]
            _, masks, _ = g.warp_images_and_masks([dev_source(case.size, gpu_ctx)], [None], rects=[case.rect],
                                                  camera_arrays=(case.K[None], case.R[None]), source_masks=sm)
            flags[pattern] = buf_flags(masks[0])
    finally:
        S.set_device_resident(prev)
    assert buf_flags(dev_mask("binary", case.size, gpu_ctx)) == _lib.CONTRIB_U8_BINARY and buf_flags(dev_mask("hash", case.size, gpu_ctx)) == 0
    assert flags == {None: _lib.CONTRIB_U8_BINARY, "hash": 0, "binary": _lib.CONTRIB_U8_BINARY}


def test_handles_round_trip(gpu_ctx):
    rng = np.random.default_rng(13)
    frame, m = rng.integers(0, 256, (PH, PW, 3), dtype=np.uint8), CM.mask("hash", (PW, PH))
    d = S.as_device(frame, gpu_ctx)
    assert d.validity is None
    f = S.with_validity(d, m)
    assert d.validity is None   # the caller's handle is not changed
    assert isinstance(f, S.DeviceImage) and f.shape == d.shape and f.device_ptr() == d.device_ptr() and f.stride_bytes == d.stride_bytes
    v = f.validity
    assert isinstance(v, S.DeviceImage) and v.shape == (PH, PW) and v.dtype == np.uint8 and np.array_equal(v.numpy(), m)
    assert np.array_equal(f.numpy(), frame)
    # a device mask is attached as it is: the same bytes, no copy
    dm = S.as_device(m, gpu_ctx)
    assert S.with_validity(d, dm).validity.device_ptr() == dm.device_ptr()
    # slicing keeps the matching slice of the mask
    s = f[5:40, 7:90]
    assert np.array_equal(s.numpy(), frame[5:40, 7:90]) and np.array_equal(s.validity.numpy(), m[5:40, 7:90])
    assert np.array_equal(s[1:3, 2:9].validity.numpy(), m[6:8, 9:16])
    assert d[5:40, 7:90].validity is None
    # the handle keeps its mask alive
    del dm, v
    g = S.with_validity(d, np.ascontiguousarray(m))
    assert np.array_equal(g.validity.numpy(), m)


def test_refusals_of_with_validity(gpu_ctx):
    L = gpu_ctx._lib
    frame = S.as_device(np.zeros((PH, PW, 3), np.uint8), gpu_ctx)
    mask = S.as_device(np.full((PH, PW), 255, np.uint8), gpu_ctx)
    other = S.Context(gpu_ctx.device)
    try:
        # (the images stay referenced from this dictionary for as long as their handles are used)
        bad = {
            "null frame": (None, mask),
            "null mask": (frame, None),
            "frame not u8x3": (mask, mask),
            "frame not u8": (S.as_device(np.zeros((PH, PW, 3), np.float32), gpu_ctx), mask),
            "mask of 3 channels": (frame, frame),
            "mask not u8": (frame, S.as_device(np.zeros((PH, PW), np.float32), gpu_ctx)),
            "unequal width": (frame, S.as_device(np.zeros((PH, PW + 1), np.uint8), gpu_ctx)),
            "unequal height": (frame, S.as_device(np.zeros((PH - 1, PW), np.uint8), gpu_ctx)),
            "another context": (frame, S.as_device(np.zeros((PH, PW), np.uint8), other)),
            "already carrying a mask": (S.with_validity(frame, mask), mask),
        }
        for what, (a, b) in bad.items():
            out = C.c_void_p()
            rc = L.stx_buf_with_validity(None if a is None else a._h, None if b is None else b._h, C.byref(out))
            assert rc == STX_ERR_INVALID, what
            assert not out.value and L.stx_last_error(), what
        del bad
        assert L.stx_buf_with_validity(frame._h, mask._h, None) == STX_ERR_INVALID
        assert L.stx_buf_validity(None, C.byref(C.c_void_p())) == STX_ERR_INVALID and L.stx_buf_validity(frame._h, None) == STX_ERR_INVALID
        with pytest.raises(S.StitchingError):
            S.with_validity(frame, np.zeros((PH, PW + 1), np.uint8))
    finally:
        other.close()
    # the context is still usable
    assert np.array_equal(S.with_validity(frame, mask).validity.numpy(), np.full((PH, PW), 255, np.uint8))


SHRINKS = [((96, 72), (41, 31)), ((333, 251), (333, 251)), ((67, 5), (1, 1))]


def _shrink_inputs():
    rng = np.random.default_rng(14)
    out = []
    for (sw, sh), _ in SHRINKS:
        m = rng.integers(1, 256, (sh, sw)).astype(np.uint8)
        m[rng.random((sh, sw)) < 0.03] = 0
        m[sh // 3:sh // 3 + max(sh // 4, 1), sw // 5:sw // 5 + max(sw // 3, 1)] = 0
        out.append(m)
    out[2][...] = np.where(out[2] == 0, 7, out[2])   # (67, 5) -> (1, 1): all non-zero, the result is 255 ...
    return out


def test_shrink_masks_all(gpu_ctx):
    ms = _shrink_inputs()
    sizes = [d for _, d in SHRINKS]
    want = [NS.shrink_mask(m, d) for m, d in zip(ms, sizes)]
    assert want[2][0, 0] == 255 and (want[0] == 0).any() and (want[0] == 255).any()
    prev = S.device_resident()
    got = S.shrink_masks_all(ms, sizes, ctx=gpu_ctx)
    for g, w in zip(got, want):
        assert isinstance(g, S.DeviceImage) and buf_flags(g) == _lib.CONTRIB_U8_BINARY
        assert np.array_equal(g.numpy(), w), int(np.count_nonzero(g.numpy() != w))
    assert S.device_resident() == prev
    ms[2][3, 40] = 0   # ... and one zero anywhere in it makes it 0
    assert S.shrink_masks_all(ms[2:], sizes[2:], ctx=gpu_ctx)[0].numpy()[0, 0] == 0
    # a view as the source (its own pitch), device inputs
    d = S.as_device(ms[0], gpu_ctx)
    v = d[3:70, 5:90]
    assert np.array_equal(S.shrink_masks_all([v], [(40, 30)])[0].numpy(), NS.shrink_mask(ms[0][3:70, 5:90], (40, 30)))
    assert S.shrink_masks_all([], []) == []


def test_refusals_of_mask_shrink(gpu_ctx):
    L = gpu_ctx._lib
    m = S.as_device(np.full((72, 96), 255, np.uint8), gpu_ctx)
    other = S.Context(gpu_ctx.device)

    def call(ctx_h, n, images, wh, out=True):
        hs = None if images is None else (C.c_void_p * len(images))(*[None if i is None else i._h for i in images])
        sizes = None if wh is None else (C.c_int * len(wh))(*wh)
        outs = (C.c_void_p * max(n, 1))() if out else None
        rc = L.stx_mask_shrink_batch(ctx_h, n, hs, sizes, outs)
        return rc, outs

    try:
        bad = {
            "null context": (None, 1, [m], [41, 31]),
            "null list": (gpu_ctx.handle, 1, None, [41, 31]),
            "null sizes": (gpu_ctx.handle, 1, [m], None),
            "no masks": (gpu_ctx.handle, 0, [m], [41, 31]),
            "null mask": (gpu_ctx.handle, 1, [None], [41, 31]),
            "wider": (gpu_ctx.handle, 1, [m], [97, 31]),
            "taller": (gpu_ctx.handle, 1, [m], [41, 73]),
            "zero width": (gpu_ctx.handle, 1, [m], [0, 31]),
            "zero height": (gpu_ctx.handle, 1, [m], [41, 0]),
            "negative": (gpu_ctx.handle, 1, [m], [-1, 31]),
            "u8x3": (gpu_ctx.handle, 1, [S.as_device(np.zeros((72, 96, 3), np.uint8), gpu_ctx)], [41, 31]),
            "f32": (gpu_ctx.handle, 1, [S.as_device(np.zeros((72, 96), np.float32), gpu_ctx)], [41, 31]),
            "another context": (gpu_ctx.handle, 1, [S.as_device(np.zeros((72, 96), np.uint8), other)], [41, 31]),
            "second of two": (gpu_ctx.handle, 2, [m, m], [41, 31, 97, 31]),
        }
        for what, args in bad.items():
            rc, outs = call(*args)
            assert rc == STX_ERR_INVALID and L.stx_last_error(), what
            assert not any(outs[i] for i in range(len(outs))), what
        del bad
        assert call(gpu_ctx.handle, 1, [m], [41, 31], out=False)[0] == STX_ERR_INVALID
        with pytest.raises(S.StitchingError):
            S.shrink_masks_all([m], [(97, 31)])
    finally:
        other.close()
    assert np.array_equal(S.shrink_masks_all([m], [(41, 31)])[0].numpy(), np.full((31, 41), 255, np.uint8))
