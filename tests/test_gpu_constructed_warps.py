"""The constructed warp cases (tests/constructed_warps.py) on the device: every case through
S.Warper(...).warp_images_and_masks(imgs, cams, rects=[rect]) against oracle.build_maps on the same rectangle followed by
oracle.remap_linear (image) and oracle.remap_nearest of a 255 image (mask).  0 differing bytes in both, no tolerance; the source reads
back unmodified.  tests/test_constructed_warps.py shows on the CPU which sampling path and which division every case takes
(profiles/constructed_warps.md has the table); a failure here names the family, the path and the count of differing bytes."""
import numpy as np
import pytest

import stitching_amd as S
from tests import constructed_warps as CW

pytestmark = pytest.mark.gpu

_expected, _device_sources, _single = {}, {}, {}


class _Model:
    """the remap model of a case on both sides, the previous ones back afterwards"""

    def __init__(self, oracle, mode):
        self.oracle, self.mode = oracle, mode

    def __enter__(self):
        self.prev_p, self.prev_o = S.remap_mode(), self.oracle.set_model()
        S.set_remap_mode(self.mode.replace("_", "-"))   # the product spells it "float-fma", the oracle "float_fma"
        self.oracle.set_model(**{**self.prev_o, "remap": self.mode})

    def __exit__(self, *exc):
        S.set_remap_mode(self.prev_p)
        self.oracle.set_model(**self.prev_o)


def expected(oracle, case):
    """the oracle's image and mask of a case, made once and shared (read only)"""
    if case.name not in _expected:
        xm, ym = oracle.build_maps(case.warper_type, case.scale, case.K, case.R, case.rect)
        src = case.source
        with _Model(oracle, case.model):
            img = oracle.remap_linear(src, xm, ym)
        mask = oracle.remap_nearest(np.full(src.shape[:2], 255, np.uint8), xm, ym)
        img.setflags(write=False)
        mask.setflags(write=False)
        _expected[case.name] = (img, mask)
    return _expected[case.name]


def path_of(case):
    f = case.facts
    if "waves" not in f:
        return "division " + "/".join(sorted(f["division"]))
    return "/".join(CW.CLASS_NAMES[c] for c in np.unique(f["waves"]))


def device_source(size, gpu_ctx):
    """a size's source on the device, uploaded once for the whole file (a 2 x 32 767 upload takes 0.2 s: 32 767 rows of 6 bytes)"""
    if size not in _device_sources:
        _device_sources[size] = S.as_device(np.ascontiguousarray(CW.source(*size)), gpu_ctx)
    return _device_sources[size]


def device_warp(cases, gpu_ctx):
    """one call for `cases` (one warper type, scale and remap model) -> [(image, mask)]; every source read back and compared"""
    c0 = cases[0]
    assert all((c.warper_type, c.scale, c.model) == (c0.warper_type, c0.scale, c0.model) for c in cases)
    g = S.Warper(c0.warper_type)
    g.scale = c0.scale
    srcs = [device_source(c.size, gpu_ctx) for c in cases]
    Ks, Rs = np.stack([c.K for c in cases]), np.stack([c.R for c in cases])
    imgs, masks, rects = g.warp_images_and_masks(srcs, [None] * len(cases), rects=[c.rect for c in cases], camera_arrays=(Ks, Rs))
    assert [tuple(r) for r in rects] == [c.rect for c in cases]
    for size in {c.size for c in cases}:
        assert np.array_equal(device_source(size, gpu_ctx).numpy(), CW.source(*size)), f"{size}: the source was modified"
    return [(np.asarray(i), np.asarray(m)) for i, m in zip(imgs, masks)]


def single(case, oracle, gpu_ctx):
    """the case warped alone, made once and shared (read only)"""
    if case.name not in _single:
        with _Model(oracle, case.model):
            _single[case.name] = device_warp([case], gpu_ctx)[0]
        for a in _single[case.name]:
            a.setflags(write=False)
    return _single[case.name]


def check(case, got, want):
    di, dm = (int(np.count_nonzero(g != w)) if g.shape == w.shape else -1 for g, w in zip(got, want))
    print(f"{case.family} {case.name}: path {path_of(case)}, image {di} mask {dm} differing bytes")
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape, (case.name, got[0].shape, want[0].shape)
    assert di == 0 and dm == 0, f"family {case.family}, case {case.name}, path {path_of(case)}: {di} differing image bytes, {dm} differing mask bytes"


@pytest.mark.parametrize("name", list(CW.CASES))
def test_case_equals_the_oracle(oracle, gpu_ctx, name):
    case = CW.CASES[name]
    want = expected(oracle, case)
    check(case, single(case, oracle, gpu_ctx), want)


def batch_cases():
    """10. the plane warper's fixed-point cases of scale 1 in one call: more than WARP_BATCH images, rectangles of unequal size (192 x 8,
    160 x 8, 192 x 16, 37 x 7, 3 x 8).  A call is cut into launches of WARP_BATCH consecutive images, and the order decides what each runs:
      - first the sources the tuned kernel refuses, completed to whole launches by wide cases: one refused image sends its launch to
        warp_kernel, image by image;
      - then launches of one narrow rectangle (one wavefront column) among seven wide ones (three), the narrow one at another index from
        launch to launch: the flat grid and its first_wg lookup for images 1 to 7;
      - then the wide ones left over, which have equal workgroup counts: the z grid; and the narrow ones left over"""
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


def launches(cases):
    """what launch_typed makes of a call: [(images, "warp_kernel" | "flat" | "z")].  An image needs 8 x (its bands per XCD, of 4 tile rows
    of 4 rows) x 4 x (its tiles of 64 columns) workgroups; the flat grid is taken where the z grid would launch more than 5 % empty ones"""
    out = []
    for i in range(0, len(cases), CW.BATCH):
        cs = cases[i:i + CW.BATCH]
        own = [8 * ((((c.rect[3] + 3) // 4 + 3) // 4 + 7) // 8) * 4 * ((c.rect[2] + 63) // 64) for c in cs]
        out.append((len(cs), "warp_kernel" if not all(CW.tuned(c) for c in cs) else "flat" if sum(own) < 0.95 * max(own) * len(own) else "z"))
    return out


def test_batch_equals_the_single_calls(oracle, gpu_ctx):
    cases = batch_cases()
    sizes = {c.rect[2:] for c in cases}
    assert len(cases) > 4 * CW.BATCH and len(sizes) >= 5
    ls = launches(cases)
    kinds = [k for _, k in ls]
    # all three occur, the z grid with a full launch of images, and the refused sources sit in the warp_kernel launches alone
    assert kinds.count("flat") >= 8 and (CW.BATCH, "z") in ls and kinds.count("warp_kernel") == -(-sum(not CW.tuned(c) for c in cases) // CW.BATCH)
    narrow_at = {[c.rect[2] <= CW.LANES for c in cases[CW.BATCH * i:CW.BATCH * i + CW.BATCH]].index(True) for i, k in enumerate(kinds) if k == "flat"}
    assert narrow_at == set(range(CW.BATCH))   # the narrow rectangle at every index of a launch
    together = device_warp(cases, gpu_ctx)
    bad = []
    for c, got in zip(cases, together):
        alone, want = single(c, oracle, gpu_ctx), expected(oracle, c)
        if not (np.array_equal(got[0], alone[0]) and np.array_equal(got[1], alone[1]) and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])):
            bad.append(c.name)
    print(f"batch of {len(cases)} images in {len(ls)} launches: {kinds.count('flat')} flat grid, {kinds.count('z')} z grid, "
          f"{kinds.count('warp_kernel')} warp_kernel: {len(bad)} differ")
    assert not bad, bad


def test_batch_of_unequal_sources_in_reverse_order(oracle, gpu_ctx):
    """the same with the order reversed and every third case left out: other images meet in a launch, each at another index"""
    cases = batch_cases()[::-1]
    cases = [c for i, c in enumerate(cases) if i % 3]
    for c, got in zip(cases, device_warp(cases, gpu_ctx)):
        check(c, got, expected(oracle, c))
