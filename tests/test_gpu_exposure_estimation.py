"""Exposure-gain estimation on the MI355X (stitching_amd.ExposureEstimator) against the restatement tests/numpy_exposure.py: the overlap
statistics and the gains of every kind, numpy / device inputs, and the reference's order end to end (low-resolution feed, final-resolution
compose / StitchJob) against the oracle chain."""
import numpy as np
import pytest

import stitching_amd as S
from stitching_amd import config, synthetic
from tests import numpy_exposure as X

pytestmark = pytest.mark.gpu

EXACT = ("gain_blocks", "channel", "channel_blocks")
FACTORS = (1.0, 0.8, 1.25, 0.9, 1.1, 0.7, 1.3, 0.95)


def _frames(oracle, n, w, h):
    return [oracle.gain_apply(synthetic.make_frame(i, w, h), FACTORS[i % len(FACTORS)]) for i in range(n)]


def _cams(wtype, n, w, h):
    if wtype == "affine":
        return synthetic.affine_scan_cameras(n, w, h)
    return synthetic.ring_cameras(n, w, h, focal_factor=0.75, span_deg=min(340.0, 45.0 * n))


def _low_res(oracle, n, wtype, w=192, h=144, aspect=1):
    """Warped low-resolution frames (the product's warper: inputs of both sides), their masks and corners."""
    frames = _frames(oracle, n, w, h)
    cams = _cams(wtype, n, w, h)
    wp = S.Warper(wtype)
    wp.set_scale(cams)
    sizes = [(f.shape[1], f.shape[0]) for f in frames]
    imgs = [np.asarray(x) for x in wp.warp_images(frames, cams, aspect)]
    masks = [np.asarray(x) for x in wp.create_and_warp_masks(sizes, cams, aspect)]
    corners, _ = wp.warp_rois(sizes, cams, aspect)
    return [tuple(int(v) for v in c) for c in corners], imgs, masks


def _case(oracle, name):
    """-> corners, imgs, masks, block_size of a named case."""
    if name == "n1":
        c, i, m = _low_res(oracle, 1, "spherical")
        return c, i, m, 32
    if name == "n2_cyl":
        c, i, m = _low_res(oracle, 2, "cylindrical")
        return c, i, m, 32
    if name == "n3_bl7":
        c, i, m = _low_res(oracle, 3, "spherical")
        return c, i, m, 7
    if name == "n4_affine_bl20":
        c, i, m = _low_res(oracle, 4, "affine", 160, 120)
        return c, i, m, 20
    if name == "n8_negative_bl13":
        c, i, m = _low_res(oracle, 8, "spherical", 128, 96)
        return [(x - 1000, y - 37) for x, y in c], i, m, 13
    if name == "special":  # an image without overlap, an empty mask, masks holding 254
        c, i, m = _low_res(oracle, 4, "cylindrical", 160, 120)
        c[3] = (c[3][0] + 5000, c[3][1])
        m[1] = np.zeros_like(m[1])
        m[2] = m[2].copy()
        m[2][::3] = np.where(m[2][::3] == 255, 254, m[2][::3])
        m[0] = m[0].copy()
        m[0][:, ::5] = np.where(m[0][:, ::5] == 255, 200, m[0][:, ::5])
        return c, i, m, 32
    raise KeyError(name)


CASES = ("n1", "n2_cyl", "n3_bl7", "n4_affine_bl20", "n8_negative_bl13", "special")


def _dense(m, ab, c, sums, plane, channels):
    jobs = {}
    for (a, b), cc, s in zip(ab.tolist(), c.tolist(), sums):
        jobs[(a, b)] = (cc, list(s[:3]) if channels else [s[0]], list(s[3:6]) if channels else [s[1]])
    return X.stats_matrices(m, jobs, plane)


def _check(kind, corners, imgs, masks, bl, nr_feeds=1):
    est = S.ExposureEstimator(kind, nr_feeds=nr_feeds, block_size=bl)
    want, first, units = X.feed(kind, corners, imgs, masks, nr_feeds, bl, want_stats=True)
    m = len(units)
    channels = kind.startswith("channel")
    ab, c, sums = est.stats(corners, imgs, masks)
    assert len(ab) == len(first) and {tuple(p) for p in ab.tolist()} == set(first)
    for p in range(3 if channels else 1):
        N, I, skip = _dense(m, ab, c, sums, p, channels)
        rN, rI, rskip = X.stats_matrices(m, first, p)
        assert np.array_equal(N, rN) and np.array_equal(skip, rskip)
        if kind == "gain":
            assert np.allclose(I, rI, rtol=1e-12, atol=0)
        else:
            assert np.array_equal(I.view(np.uint64), rI.view(np.uint64))
    est.feed(corners, imgs, masks)
    got = est.getMatGains()
    assert est.info["units"] == m and est.info["pair_jobs"] == len(first)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.shape == w.shape and g.dtype == w.dtype
        if kind == "gain":
            assert np.allclose(g, w, rtol=1e-9, atol=0)
        else:
            assert np.array_equal(g.view(np.uint8), w.view(np.uint8))
    if kind == "gain":  # a fixed reduction order: identical run to run
        est2 = S.ExposureEstimator(kind, nr_feeds=nr_feeds, block_size=bl)
        est2.feed(corners, imgs, masks)
        assert all(np.array_equal(a, b) for a, b in zip(got, est2.getMatGains()))
    return got


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("kind", X.KINDS)
def test_stats_and_gains_match_the_restatement(oracle, gpu_ctx, kind, case):
    corners, imgs, masks, bl = _case(oracle, case)
    got = _check(kind, corners, imgs, masks, bl)
    if case == "special":
        assert np.all(got[1] == 1) and np.all(got[3] == 1)


@pytest.mark.parametrize("nr_feeds", [2, 3])
@pytest.mark.parametrize("kind", X.KINDS)
def test_several_feeds(oracle, gpu_ctx, kind, nr_feeds):
    corners, imgs, masks, _ = _case(oracle, "n4_affine_bl20")
    _check(kind, corners, imgs, masks, 24, nr_feeds)


def test_more_than_two_thousand_units(oracle, gpu_ctx):
    corners, imgs, masks = _low_res(oracle, 8, "spherical", 192, 144)
    units = X.make_units(corners, imgs, True, 8)
    assert len(units) > 2000
    _check("gain_blocks", corners, imgs, masks, 8)


@pytest.mark.parametrize("kind", X.KINDS)
def test_numpy_and_device_inputs_agree_and_inputs_stay(oracle, gpu_ctx, kind):
    corners, imgs, masks, bl = _case(oracle, "n3_bl7")
    before = [i.copy() for i in imgs]
    d_imgs = [S.DeviceImage.from_numpy(i, gpu_ctx) for i in imgs]
    d_masks = [S.DeviceImage.from_numpy(m, gpu_ctx) for m in masks]
    a = S.ExposureEstimator(kind, nr_feeds=2, block_size=bl)
    a.feed(corners, imgs, masks)
    b = S.ExposureEstimator(kind, nr_feeds=2, block_size=bl)
    b.feed(corners, d_imgs, d_masks)
    assert all(np.array_equal(x, y) for x, y in zip(a.getMatGains(), b.getMatGains()))
    assert all(np.array_equal(x, y) for x, y in zip(imgs, before))
    assert all(np.array_equal(d.numpy(), y) for d, y in zip(d_imgs, before))
    assert all(np.array_equal(d.numpy(), m) for d, m in zip(d_masks, masks))


def _overlap_ratios(corners, imgs, masks):
    """|log(mean intensity ratio)| over the common pixels of every overlapping pair of images."""
    out = []
    for i in range(len(imgs)):
        for j in range(i + 1, len(imgs)):
            (xi, yi), (xj, yj) = corners[i], corners[j]
            hi, wi = imgs[i].shape[:2]
            hj, wj = imgs[j].shape[:2]
            tx, ty, rx, ry = max(xi, xj), max(yi, yj), min(xi + wi, xj + wj), min(yi + hi, yj + hj)
            if tx >= rx or ty >= ry:
                continue
            si, sj = (slice(ty - yi, ry - yi), slice(tx - xi, rx - xi)), (slice(ty - yj, ry - yj), slice(tx - xj, rx - xj))
            m = (masks[i][si] == 255) & (masks[j][sj] == 255)
            if m.sum() < 100:
                continue
            a, b = imgs[i][si][m].astype(np.float64).mean(), imgs[j][sj][m].astype(np.float64).mean()
            out.append(abs(np.log(a / b)))
    return np.array(out)


@pytest.mark.parametrize("kind", X.KINDS)
def test_end_to_end_in_stitcher_order(oracle, gpu_ctx, monkeypatch, kind):
    """Stitcher.stitch's order with injected cameras: the low-resolution half through the product's classes with the switch on
    "device", then compose / StitchJob at final resolution — against the oracle warper + the restatement's gains + the oracle blender."""
    from stitching_amd.pipeline import StitchJob, compose

    monkeypatch.setattr(config, "_exposure_estimator", "device")
    n, w, h, wtype, strength = 4, 320, 240, "spherical", 5
    frames = _frames(oracle, n, w, h)
    cams = _cams(wtype, n, w, h)
    low = [S.resize_linear_exact(f, (w // 2, h // 2)) for f in frames]
    low = [np.asarray(x) for x in low]
    sizes_low = [(x.shape[1], x.shape[0]) for x in low]
    aspect = 0.5
    wp = S.Warper(wtype)
    wp.set_scale(cams)
    l_imgs = wp.warp_images(low, cams, aspect)
    l_masks = wp.create_and_warp_masks(sizes_low, cams, aspect)
    l_corners, _ = wp.warp_rois(sizes_low, cams, aspect)
    comp = S.ExposureErrorCompensator(kind)
    assert isinstance(comp.compensator, S.ExposureEstimator)
    comp.feed(l_corners, l_imgs, l_masks)

    ow = oracle.Warper(wtype)
    ow.set_scale(cams)
    o_imgs = [np.asarray(x) for x in ow.warp_images(low, cams, aspect)]
    o_masks = [np.asarray(x) for x in ow.create_and_warp_masks(sizes_low, cams, aspect)]
    o_corners, _ = ow.warp_rois(sizes_low, cams, aspect)
    gains = X.feed(kind, o_corners, o_imgs, o_masks)
    for g, r in zip(comp.gains, gains):
        want = np.asarray(r, np.float32 if kind.endswith("_blocks") else np.float64).reshape(np.asarray(g).shape)
        if kind == "gain":
            assert np.allclose(g, want, rtol=1e-9, atol=0)
        else:
            assert np.array_equal(g, want)

    pano, pmask = compose(frames, cams, warper_type=wtype, blend_strength=strength, compensator=comp, ctx=gpu_ctx)
    job_pano, _ = StitchJob(frames, cams, warper_type=wtype, blend_strength=strength, compensator=comp, ctx=gpu_ctx).run()
    pano, pmask, job_pano = np.asarray(pano), np.asarray(pmask), np.asarray(job_pano)

    ow = oracle.Warper(wtype)
    ow.set_scale(cams)
    sizes = [(f.shape[1], f.shape[0]) for f in frames]
    f_imgs = ow.warp_images(frames, cams)
    f_masks = ow.create_and_warp_masks(sizes, cams)
    f_corners, f_sizes = ow.warp_rois(sizes, cams)
    if kind.endswith("_blocks"):
        f_imgs = [oracle.block_gain_apply(np.asarray(im), g) for im, g in zip(f_imgs, gains)]
    else:  # one gain or a BGR triple per image
        f_imgs = [oracle.gain_apply(np.asarray(im), np.ravel(g)) for im, g in zip(f_imgs, gains)]
    ob = oracle.Blender("multiband", strength)
    ob.prepare(f_corners, f_sizes)
    for im, mk, c in zip(f_imgs, f_masks, f_corners):
        ob.feed(im, mk, c)
    o_pano, o_mask = ob.blend()
    o_pano, o_mask = np.asarray(o_pano), np.asarray(o_mask)
    assert np.array_equal(pmask, o_mask)
    if kind in EXACT:
        assert np.array_equal(pano, o_pano) and np.array_equal(job_pano, o_pano)
    else:
        assert np.abs(pano.astype(int) - o_pano).max() <= 1 and np.array_equal(job_pano, pano)

    # the property the gains are for: the overlaps' mean intensities move towards each other
    if kind in ("gain", "channel"):
        comp_low = [oracle.gain_apply(im, np.ravel(g)) for im, g in zip(o_imgs, gains)]
        before, after = _overlap_ratios(o_corners, o_imgs, o_masks), _overlap_ratios(o_corners, comp_low, o_masks)
        assert before.size and after.mean() < before.mean()
