"""The constructed exposure families (tests/constructed_exposures.py) on the MI355X: the estimation scenes through
S.ExposureEstimator (`stats` and `feed`) against the restatement tests/numpy_exposure.py — N, skip, c and the integer sums equal, I
bit-equal and gains byte-equal for the three exact kinds, the "gain" kind's two sums bit-equal to constructed_exposures.tree_sum and
its gains at the project's rtol = 1e-9 — and the apply inputs through S.ExposureErrorCompensator (`apply`, `apply_all`) and, for two
cases, the C ABI's stx_block_gain_apply_batch against oracle.gain_apply / oracle.block_gain_apply with 0 differing bytes.  Inputs are
read back unmodified; views are read back with their whole buffers.  What each family reaches, that its facts hold, and that it tells the
contract from a subtly wrong variant is asserted without a GPU in tests/test_constructed_exposures.py; here only the device is asked."""
import ctypes as C
import functools

import numpy as np
import pytest

import stitching_amd as S
from oracle import oracle as O
from stitching_amd import _lib
from tests import constructed_exposures as CE
from tests import numpy_exposure as X

pytestmark = pytest.mark.gpu

EXACT = ("gain_blocks", "channel", "channel_blocks")


@functools.lru_cache(maxsize=None)
def _contract(builder, args, kind, nr_feeds=1):
    """(scene, gains, the first feed's jobs, units) by the restatement: built once per case, never written to"""
    s = getattr(CE, builder)(*args)
    gains, first, units = X.feed(kind, s.corners, s.imgs, s.masks, nr_feeds, s.bl, want_stats=True)
    for g in gains:
        g.setflags(write=False)
    return s, gains, first, units


def _pitched(a, ctx, fill, xoff):
    """`a` as a view, `xoff` columns and 5 rows into a larger device buffer whose surroundings hold `fill` ("random": seeded bytes).
    -> (view, big, dev): the host copy of the whole buffer and its device image, to be read back"""
    shape = (a.shape[0] + 9, a.shape[1] + xoff + 13) + a.shape[2:]
    if isinstance(fill, str):
        big = np.random.default_rng(a.shape[1] + 7 * xoff).integers(0, 256, shape).astype(a.dtype)
    else:
        big = np.full(shape, fill, a.dtype)
    big[5:5 + a.shape[0], xoff:xoff + a.shape[1]] = a
    dev = S.DeviceImage.from_numpy(big, ctx)
    return dev[5:5 + a.shape[0], xoff:xoff + a.shape[1]], big, dev


def _upload(ctx, arrays, fill, views):
    """device images of `arrays` (views: as views at odd column offsets 1, 2, 3, 5, ... amid `fill`) and a check that reads every
    buffer back whole and unchanged"""
    devs, held = [], []
    for k, a in enumerate(arrays):
        if views:
            v, big, dev = _pitched(a, ctx, fill, (1, 2, 3, 5, 7)[k % 5])
        else:
            big = np.array(a)
            v = dev = S.DeviceImage.from_numpy(big, ctx)
        devs.append(v)
        held.append((big, dev))

    def check():
        for big, dev in held:
            assert np.array_equal(dev.numpy(), big)

    return devs, check


def _dense(m, ab, c, sums, plane, channels):
    jobs = {}
    for (a, b), cc, s in zip(ab.tolist(), c.tolist(), sums):
        jobs[(a, b)] = (cc, list(s[:3]) if channels else [s[0]], list(s[3:6]) if channels else [s[1]])
    return X.stats_matrices(m, jobs, plane)


def _estimate(ctx, builder, args, kind, nr_feeds=1, solver="host", views=False, stats=True):
    s, want, first, units = _contract(builder, args, kind, nr_feeds)
    m, channels = len(units), kind.startswith("channel")
    imgs, check_imgs = _upload(ctx, s.imgs, "random", views)
    masks, check_masks = _upload(ctx, s.masks, 255, views)
    est = S.ExposureEstimator(kind, nr_feeds=nr_feeds, block_size=s.bl, solver=solver)
    if stats:
        ab, c, sums = est.stats(s.corners, imgs, masks)
        assert len(ab) == len(first) and {tuple(p) for p in ab.tolist()} == set(first)
        for (a, b), cc, sm in zip(ab.tolist(), c.tolist(), sums):
            rc, ra, rb = first[(a, b)]
            assert cc == rc, (a, b)
            if channels:  # integer sums: equal
                assert [int(v) for v in sm] == list(ra) + list(rb), (a, b)
        for p in range(3 if channels else 1):
            N, I, skip = _dense(m, ab, c, sums, p, channels)
            rN, rI, rskip = X.stats_matrices(m, first, p)
            assert np.array_equal(N, rN) and np.array_equal(skip, rskip)
            if kind == "gain":
                assert np.allclose(I, rI, rtol=1e-12, atol=0)
            else:
                assert np.array_equal(I.view(np.uint64), rI.view(np.uint64))
        if kind == "gain":  # the order the kernel documents, to the bit
            nj = CE.norm_jobs(s)
            for (a, b), cc, sm in zip(ab.tolist(), c.tolist(), sums):
                rc, va, vb = nj[(a, b)]
                want_bits = np.array([CE.tree_sum(va), CE.tree_sum(vb)]).view(np.uint64)
                assert cc == rc and np.array_equal(np.array(sm[:2]).view(np.uint64), want_bits), (a, b, sm[:2])
    est.feed(s.corners, imgs, masks)
    got = est.getMatGains()
    assert est.info["units"] == m and est.info["pair_jobs"] == len(first) and est.info["solver"] == solver
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.shape == w.shape and g.dtype == w.dtype
        if kind == "gain":
            assert np.allclose(g, w, rtol=1e-9, atol=0)
        else:
            assert int(np.count_nonzero(g.view(np.uint8) != w.view(np.uint8))) == 0
    check_imgs()
    check_masks()
    return got


# ---------------------------------------------------------------------------------------------------------------------------------
# estimation
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", CE.LAYOUTS)
@pytest.mark.parametrize("n", CE.JOB_SIZES)
def test_job_sizes(gpu_ctx, n, layout):
    """overlaps of 1 .. 1025 pixels as a row, a column and the squarest rectangle; full masks, the first chunk of 256 off, the last
    partial chunk off; whole images and one block per image"""
    for mode in CE.MASK_MODES:
        for kind in X.KINDS:
            got = _estimate(gpu_ctx, "job_sizes", (n, layout, mode), kind)
            if _contract("job_sizes", (n, layout, mode), kind)[0].facts["c"] == 0:
                assert all((g == 1).all() for g in got)


@pytest.mark.parametrize("kind", X.KINDS)
@pytest.mark.parametrize("which", CE.PLACEMENTS)
def test_placements(gpu_ctx, which, kind):
    got = _estimate(gpu_ctx, "placements", (which,), kind)
    if which.startswith("touch"):
        assert all((g == 1).all() for g in got)


@pytest.mark.parametrize("kind", ("gain_blocks", "channel_blocks"))
@pytest.mark.parametrize("which", CE.BLOCK_GRIDS)
def test_block_grids(gpu_ctx, which, kind):
    _estimate(gpu_ctx, "block_grids", (which,), kind)


@pytest.mark.parametrize("kind", X.KINDS)
@pytest.mark.parametrize("which", CE.VALUES)
def test_values(gpu_ctx, which, kind):
    """an all-white overlap (the last entry of the sqrt table), an all-black one, masks of 0, 1, 127, 254, 255, and a pair that
    overlaps in rectangle but not in mask"""
    _estimate(gpu_ctx, "values", (which,), kind)


@pytest.mark.parametrize("kind", ("gain_blocks", "channel_blocks"))
@pytest.mark.parametrize("case", [("placements", (w,)) for w in CE.PLACEMENTS if not w.startswith("touch")] +
                         [("values", ("mask_levels",)), ("values", ("disjoint_masks",))], ids=lambda c: c[1][0])
def test_device_solver(gpu_ctx, case, kind):
    """the same bits with the gain systems solved by the device LU (4 or more unknowns)"""
    assert len(_contract(*case, kind)[3]) >= 4
    _estimate(gpu_ctx, *case, kind, solver="device", stats=False)


def test_tree_order_at_the_documented_upper_end(gpu_ctx):
    """340 x 300 = 102 000 pixels in one job: the "gain" kind's sums are tree_sum's to the bit"""
    _estimate(gpu_ctx, "tree_large", (), "gain")
    _estimate(gpu_ctx, "tree_large", (), "channel")


@pytest.mark.parametrize("nr_feeds", (2, 3))
@pytest.mark.parametrize("which", CE.BETWEEN_FEEDS)
def test_between_feeds(gpu_ctx, which, nr_feeds):
    """gains far from 1 and saturating products between feeds; 256 pixels beside 16 900 (the grid-stride loop), blocks of 26 under
    bl = 32, BGR triples; widths 20 .. 23 through gain_apply_kernel; the caller's images read back unchanged"""
    for kind in ("gain", "channel") if which == "tails" else X.KINDS:
        _estimate(gpu_ctx, "between_feeds", (which,), kind, nr_feeds, stats=False)


@pytest.mark.parametrize("nr_feeds", (1, 2))
@pytest.mark.parametrize("grid", CE.FILTER_GRIDS, ids=lambda g: "%dx%d" % g)
def test_filter_shapes(gpu_ctx, grid, nr_feeds):
    for kind in ("gain_blocks", "channel_blocks"):
        _estimate(gpu_ctx, "filter_shapes", (grid,), kind, nr_feeds, stats=False)


@pytest.mark.parametrize("nr_feeds", (1, 2))
@pytest.mark.parametrize("case", [("placements", ("inside",)), ("values", ("mask_levels",)), ("between_feeds", ("tails",))], ids=lambda c: c[1][0])
def test_estimation_on_views(gpu_ctx, case, nr_feeds):
    """images and masks as views at odd column offsets: random bytes around the images, 255 around the masks (a read outside a view
    would count); the pitched rows of the statistics, and the scratch copies before the second feed"""
    for kind in X.KINDS:
        _estimate(gpu_ctx, *case, kind, nr_feeds, views=True, stats=nr_feeds == 1)


# ---------------------------------------------------------------------------------------------------------------------------------
# apply
# ---------------------------------------------------------------------------------------------------------------------------------
def _kind(gmap):
    return "channel_blocks" if np.ndim(gmap) == 3 else "gain_blocks"


def _same(got, want, what=None):
    got = np.asarray(got)
    assert got.shape == want.shape and int(np.count_nonzero(got != want)) == 0, what


def _apply_all(imgs, maps, sub=None):
    e = S.ExposureErrorCompensator(_kind(maps[0]))
    e.set_gains(maps)
    return e.apply_all([(0, 0)] * len(imgs), [np.array(im) for im in imgs], sub=sub)


def _apply_view(ctx, img, gains, kind, xoff):
    """one image as a view `xoff` columns into a buffer of random bytes through `apply`: the view is the oracle's, the rest unchanged"""
    view, big, dev = _pitched(img, ctx, "random", xoff)
    e = S.ExposureErrorCompensator(kind)
    e.set_gains([gains])
    e.apply(0, (0, 0), view, None)
    want = big.copy()
    want[5:5 + img.shape[0], xoff:xoff + img.shape[1]] = O.block_gain_apply(img, gains) if kind.endswith("_blocks") else O.gain_apply(img, gains)
    _same(dev.numpy(), want, (kind, xoff))


def _abi_batch(ctx, imgs, maps, flags):
    """stx_block_gain_apply_batch itself: flags None passes a null pointer"""
    d = [S.DeviceImage.from_numpy(np.array(im), ctx) for im in imgs]
    g = [S.DeviceImage.from_numpy(np.ascontiguousarray(m, np.float32), ctx) for m in maps]
    n = len(d)
    ia, ga = (C.c_void_p * n)(*[a._h for a in d]), (C.c_void_p * n)(*[a._h for a in g])
    fl = None if flags is None else (C.c_int * n)(*flags)
    _lib.check(ctx._lib.stx_block_gain_apply_batch(ctx.handle, n, ia, ga, None, fl))
    return [a.numpy() for a in d]


@functools.lru_cache(maxsize=None)
def _ties(channels):
    img, gmap, f = CE.ties(channels)
    CE.assert_tie_facts(f)
    want = O.block_gain_apply(img, gmap)
    for a in (img, gmap, want):
        a.setflags(write=False)
    return img, gmap, want


@pytest.mark.parametrize("channels", (1, 3))
@pytest.mark.parametrize("path", ("fast", "not_fast", "null_flags", "plain"))
def test_ties_blocks(gpu_ctx, path, channels):
    """byte x gain on k + 0.5 for half of the bytes, both parities, 254.5 and 255.5: v_cvt_pk_u8_f32 with and without the range test,
    and stxd::cv_round in the one-pixel-per-lane kernel (a view)"""
    img, gmap, want = _ties(channels)
    if path == "fast":
        _same(_apply_all([img], [gmap])[0], want)
    elif path == "not_fast":  # an unbounded map in the same launch
        other, omap = CE.geometry(9, 5, 2, 2, channels)
        omap = omap.copy()
        omap[0, 0] = np.float32(3e7)
        out = _apply_all([img, other], [gmap, omap])
        _same(out[0], want)
        _same(out[1], O.block_gain_apply(other, omap))
    elif path == "null_flags":  # ABI only: no flags at all is "not bounded"
        _same(_abi_batch(gpu_ctx, [img], [gmap], None)[0], want)
    else:
        _apply_view(gpu_ctx, img, gmap, _kind(gmap), 3)


@pytest.mark.parametrize("w", CE.TIE_WIDTHS)
def test_ties_scalar_ramp(gpu_ctx, w):
    """gains 0.5, 1.5, 2.5 and the triple over all 256 byte values, widths 20 .. 23: the dword groups and the tail of gain_apply_kernel"""
    img, _ = CE.tie_ramp(w)
    for g in CE.TIE_SCALARS + (CE.TIE_SCALARS,):
        e = S.ExposureErrorCompensator("gain" if np.isscalar(g) else "channel")
        e.set_gains([g])
        _same(e.apply(0, (0, 0), img.copy(), None), O.gain_apply(img, g), (w, g))


@functools.lru_cache(maxsize=None)
def _edge(which, channels):
    img, gmap, f = CE.int_edge(which, channels)
    want = O.block_gain_apply(img, gmap)
    for a in (img, gmap, want):
        a.setflags(write=False)
    return img, gmap, want, f


@pytest.mark.parametrize("channels", (1, 3))
def test_int_edge_batched_with_mixed_flags(gpu_ctx, channels):
    """8421504 and its fp32 neighbours, 8.0e6 and the float below it, -0.0, a negative, a subnormal, inf (over a 0 byte too), NaN:
    one launch whose maps are bounded and unbounded, then every map alone (the bounded one through the FAST kernel)"""
    cases = [_edge(w, channels) for w in CE.EDGE_MAPS]
    assert [c[3]["bounded"] for c in cases] == [False, False, True, False, False]
    out = _apply_all([c[0] for c in cases], [c[1] for c in cases])
    for which, o, c in zip(CE.EDGE_MAPS, out, cases):
        _same(o, c[2], which)
    for which, c in zip(CE.EDGE_MAPS, cases):
        _same(_apply_all([c[0]], [c[1]])[0], c[2], which)


@pytest.mark.parametrize("channels", (1, 3))
@pytest.mark.parametrize("which", CE.EDGE_MAPS)
def test_int_edge_plain_kernel(gpu_ctx, which, channels):
    img, gmap, _, _ = _edge(which, channels)
    _apply_view(gpu_ctx, img, gmap, _kind(gmap), 1 + len(which) % 3)


@pytest.mark.parametrize("channels", (1, 3))
def test_geometry(gpu_ctx, channels):
    """5 x 700 and 3 x 300 (the row table needs more workgroups than the columns), widths 1 .. 5 and 255 .. 257, heights 1, 15 .. 17, 33,
    maps 1 x 1, 1 x k, k x 1 and 40 x 3 on 13 x 9: in one apply_all (two launches) and each alone"""
    cases = [CE.geometry(w, h, gw, gh, channels) for w, h, gw, gh in CE.GEOMETRY]
    want = [O.block_gain_apply(img, gmap) for img, gmap in cases]
    assert len(cases) > CE.GAIN_BATCH
    for k, o in enumerate(_apply_all([c[0] for c in cases], [c[1] for c in cases])):
        _same(o, want[k], CE.GEOMETRY[k])
    for k, (img, gmap) in enumerate(cases):
        _same(_apply_all([img], [gmap])[0], want[k], CE.GEOMETRY[k])


@pytest.mark.parametrize("channels", (1, 3))
def test_sub_rectangles(gpu_ctx, channels):
    """rectangles at an odd corner, in the far corner and of one pixel: the whole image compensated and then cut"""
    fw, fh, gw, gh = CE.SUB_FULL
    img, gmap = CE.geometry(fw, fh, gw, gh, channels)
    want = O.block_gain_apply(img, gmap)
    cuts = [img[y:y + h, x:x + w] for x, y, w, h in CE.SUB_RECTS]
    out = _apply_all(cuts, [gmap] * len(cuts), sub=[(fw, fh, x, y) for x, y, w, h in CE.SUB_RECTS])
    for o, (x, y, w, h) in zip(out, CE.SUB_RECTS):
        _same(o, want[y:y + h, x:x + w], (x, y, w, h))


def test_only_the_second_launch_is_unbounded(gpu_ctx):
    imgs, maps, f = CE.unbounded_in_second_launch()
    assert f["bounded"] == [True] * 17 + [False]
    for k, o in enumerate(_apply_all(imgs, maps)):
        _same(o, O.block_gain_apply(imgs[k], maps[k]), k)


def test_one_call_with_maps_of_one_and_three_channels(gpu_ctx):
    """ABI only: the maps after the first whose channel count differs fall to the one-pixel-per-lane kernel"""
    cases = [CE.geometry(21, 18, 3, 2, ch, seed=k) for k, ch in enumerate((1, 3, 1, 3, 3))]
    out = _abi_batch(gpu_ctx, [c[0] for c in cases], [c[1] for c in cases], [_lib.GAIN_MAP_BOUNDED] * len(cases))
    for k, (o, (img, gmap)) in enumerate(zip(out, cases)):
        _same(o, O.block_gain_apply(img, gmap), k)


@pytest.mark.parametrize("xoff", (1, 2, 3, 4))
@pytest.mark.parametrize("kind", ("gain", "channel", "gain_blocks", "channel_blocks"))
def test_apply_on_views(gpu_ctx, kind, xoff):
    """all four compensators on a view that starts 3, 6, 9 bytes past a dword (and 12: aligned again) amid random bytes: the per-byte
    rows of gain_apply_kernel, the one-pixel-per-lane block kernel; the surroundings read back unchanged"""
    rng = np.random.default_rng(xoff)
    img = rng.integers(0, 256, (11, 22 + xoff, 3)).astype(np.uint8)
    gains = {"gain": 1.5, "channel": (0.5, 1.5, 2.5), "gain_blocks": (0.5 + rng.random((2, 3))).astype(np.float32),
             "channel_blocks": (0.5 + rng.random((2, 3, 3))).astype(np.float32)}[kind]
    _apply_view(gpu_ctx, img, gains, kind, xoff)
