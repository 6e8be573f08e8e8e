"""The affine models of the project's own matcher on the MI355X (stitching_amd.MatchEstimator(model="affine"), csrc/stx_matches.hip)
against their contract tests/numpy_affine.py: every integer array and the float64 bits of H_sample equal, H and confidence within 1e-9
relative.  Inputs are synthetic ImageFeatures (no images); the contract's result of an input is computed once."""
import ctypes as C

import numpy as np
import pytest

import stitching_amd as S
from stitching_amd import _lib
from stitching_amd import match_estimation as ME
from tests import affine_rigs as AR
from tests import numpy_affine as NA
from tests.test_gpu_matches import _same

pytestmark = pytest.mark.gpu

MODELS = ("affine_partial", "affine_full")
PLANTED = {"affine_partial": AR.SIMILARITY, "affine_full": AR.AFFINE}
_REFS = {}


def _estimator(model, **kw):
    est = S.MatchEstimator(model="affine", full_affine=model == "affine_full", **kw)
    assert est.model == model
    return est


def _check(key, feats, model, **kw):
    """the device on `feats` (the contract's dicts) against the contract's result (computed once per key); the inputs stay as they were"""
    F = AR.package_features(feats)
    before = [(f.descriptors.copy(), f.x.copy(), f.y.copy(), f.level.copy()) for f in F]
    est = _estimator(model, **kw)
    got = est.match(F)
    if (key, model) not in _REFS:
        _REFS[(key, model)] = NA.match(feats, model=model, **kw)
    want = _REFS[(key, model)]
    _same(got, want)
    for e, w in zip(got, want):
        if w["H"] is not None:
            assert np.array_equal(e.H[2], [0.0, 0.0, 1.0])
    for f, (d, x, y, l) in zip(F, before):
        assert np.array_equal(f.descriptors, d) and np.array_equal(f.x, x) and np.array_equal(f.y, y) and np.array_equal(f.level, l)
    n = len(F)
    assert est.info["pairs"] == sum(1 for e in got if 0 <= e.src_img_idx < e.dst_img_idx)
    assert est.info["matches"] == sum(len(got[i * n + j].matches) for i in range(n) for j in range(i + 1, n))
    return got, want


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("m", (5, 6, 7, 64, 65, 300))
def test_planted_map(model, m):
    """no RANSAC below 6 matches; 64 and 65: the wavefront's edge; two pyramid levels"""
    A = PLANTED[model]
    got, want = _check(("planted", m), AR.planted_pair(10 + m, m, A), model, ransac_iters=200)
    e = got[1]
    assert len(e.matches) == m
    if m == 5:
        assert e.H is None and e.H_sample is None and e.hypothesis == -1 and e.confidence == 0.0 and e.num_inliers == 0
    else:
        assert e.H_sample[6] == 0 and e.H_sample[7] == 0 and not np.signbit(e.H_sample[6:8]).any() and e.H_sample[8] > 0
    if m >= 64:
        assert e.num_inliers >= int(0.6 * m) and e.confidence > 1
        assert np.abs(e.H[:2, :2] - A[:2, :2]).max() < 0.02 and np.abs(e.H[:2, 2] - A[:2, 2]).max() < 2.0
        back = got[2]
        assert (back.src_img_idx, back.dst_img_idx) == (1, 0) and np.array_equal(back.matches[:, [1, 0, 2]], e.matches)
        assert np.allclose(back.H @ e.H, np.eye(3), atol=1e-9) and back.confidence == e.confidence and back.H_sample is None


def _pool(rs, n):
    return rs.randint(0, 256, (n, 32)).astype(np.uint8)


@pytest.mark.parametrize("model", MODELS)
def test_hypothesis_ties(model):
    """a pure integer translation without outliers: every hypothesis has every match as an inlier, the smallest k wins"""
    rs = np.random.RandomState(20)
    D, xy, order = _pool(rs, 50), rs.randint(40, 440, (50, 2)), rs.permutation(50)
    T = np.array([[1.0, 0.0, 31.0], [0.0, 1.0, -17.0], [0.0, 0.0, 1.0]])
    feats = [AR.features_of(D, xy), AR.features_of(D[order], xy[order] + (31, -17))]
    got, want = _check("translation", feats, model, ransac_iters=64)
    assert got[1].hypothesis == 0 and got[1].num_inliers == 50 and np.abs(got[1].H - T).max() < 1e-9


@pytest.mark.parametrize("model", MODELS)
def test_all_matches_on_one_point(model):
    """coincident sample points: W = 0 (partial) and det M = 0 (full) in every hypothesis, none has an inlier"""
    D = _pool(np.random.RandomState(30), 40)
    xy = np.full((40, 2), 77)
    got, want = _check("one point", [AR.features_of(D, xy), AR.features_of(D[::-1], xy + (3, 4))], model, ransac_iters=64)
    e = got[1]
    assert len(e.matches) == 40 and e.num_inliers == 0 and e.hypothesis == 0 and e.H is None and e.confidence == 0.0
    assert e.H_sample[8] == 0 and not e.inliers_mask.any()


def test_all_matches_on_one_line():
    """collinear sample points: det M = 0 exactly (integer coordinates), the full model has no inliers; two points of a line fix a similarity"""
    D = _pool(np.random.RandomState(31), 40)
    t = np.arange(40)
    xy = np.stack([100 + 10 * t, 50 + 5 * t], axis=1)
    feats = [AR.features_of(D, xy), AR.features_of(D[::-1], xy[::-1] + (3, 4))]
    got, want = _check("one line", feats, "affine_full", ransac_iters=64)
    assert len(got[1].matches) == 40 and got[1].num_inliers == 0 and got[1].hypothesis == 0 and got[1].H_sample[8] == 0 and got[1].H is None
    got, want = _check("one line", feats, "affine_partial", ransac_iters=64)
    assert got[1].num_inliers == 40 and got[1].hypothesis == 0 and np.abs(got[1].H - [[1, 0, 3], [0, 1, 4], [0, 0, 1]]).max() < 1e-9


def test_clockwise_winner():
    """the winning sample of the full model is clockwise: det M < 0 before the sign rule, h8 > 0 after it, inliers as the contract's"""
    feats = AR.planted_pair(65, 80, AR.AFFINE)
    got, want = _check("clockwise", feats, "affine_full", ransac_iters=64)
    e = got[1]
    pts = [NA.uncentred(f) for f in feats]
    xyuv = np.concatenate([pts[0][e.matches[:, 0]], pts[1][e.matches[:, 1]]], axis=1)
    idx = NA.sample(0x5EED, 1, e.hypothesis, len(e.matches), 3)
    raw = NA.closed_form_full(xyuv[idx, 0:2], xyuv[idx, 2:4])
    assert raw[8] < 0 and e.H_sample[8] == -raw[8] and np.array_equal(e.H_sample[:6], -raw[:6]) and e.num_inliers >= 40


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("iters", (1, 64, 4096))
def test_ransac_iters(model, iters):
    got, want = _check(("iters", iters), AR.planted_pair(50, 40, PLANTED[model]), model, ransac_iters=iters)
    assert 0 <= got[1].hypothesis < iters


@pytest.mark.parametrize("model", MODELS)
def test_seed(model):
    feats = AR.planted_pair(60, 80, PLANTED[model])
    a, wa = _check("seed default", feats, model, ransac_iters=64)
    b, wb = _check("seed other", feats, model, ransac_iters=64, seed=12345)
    assert np.array_equal(a[1].matches, b[1].matches) and not np.array_equal(a[1].H_sample, b[1].H_sample)


@pytest.mark.parametrize("model", MODELS)
def test_repeatability(model):
    F = AR.package_features(AR.planted_pair(70, 300, PLANTED[model]))
    a = _estimator(model, ransac_iters=100).match(F)
    b = _estimator(model, ransac_iters=100).match(F)
    for x, y in zip(a, b):
        assert np.array_equal(x.matches, y.matches) and np.array_equal(x.inliers_mask, y.inliers_mask) and x.hypothesis == y.hypothesis
        assert (x.H_sample is None and y.H_sample is None) or np.array_equal(x.H_sample.view(np.uint64), y.H_sample.view(np.uint64))
        assert (x.H is None and y.H is None) or np.array_equal(x.H, y.H)
        assert x.confidence == y.confidence


# ---- the entry point -----------------------------------------------------------------------------------------------------------------------
def _call(ctx, F, model, iters=64, seed=0x5EED):
    """stx_match_features (model None) or stx_match_features_model on centred points -> rc, every output array"""
    n = len(F)
    desc = [np.ascontiguousarray(f.descriptors) for f in F]
    pts = [np.ascontiguousarray(ME.centred_points(f)) for f in F]
    shape = np.array([(d.shape[0], d.shape[1], d.dtype.itemsize) for d in desc], np.int32)
    rows = np.array([len(p) for p in pts], np.int32)
    pairs = n * (n - 1) // 2
    cap = sum(int(rows[i]) + int(rows[j]) for i in range(n) for j in range(i + 1, n))
    out = {"counts": np.full(pairs, -7, np.int32), "matches": np.full((cap, 3), -7, np.int32), "mask": np.full(cap, 9, np.uint8),
           "pick": np.full((pairs, 2), -7, np.int32), "H": np.full((pairs, 9), 7.0), "info": np.full(4, 7.0)}
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    da, pa = (C.c_void_p * n)(*[d.ctypes.data for d in desc]), (C.c_void_p * n)(*[p.ctypes.data for p in pts])
    front = (ctx.handle, n, da, shape.ctypes.data_as(ip), pa, rows.ctypes.data_as(ip), ME.ratio_threshold(0.3), -1, iters, 9.0, seed)
    back = (out["counts"].ctypes.data_as(ip), out["matches"].ctypes.data_as(ip), out["mask"].ctypes.data_as(C.POINTER(C.c_ubyte)),
            out["pick"].ctypes.data_as(ip), out["H"].ctypes.data_as(dp), out["info"].ctypes.data_as(dp))
    if model is None:
        return ctx._lib.stx_match_features(*front, *back), out
    return ctx._lib.stx_match_features_model(*front, int(model), *back), out


def _match_launches(ctx):
    return sorted(r["kernel"] for r in ctx.prof_results() if r["kernel"].startswith("match_") for _ in range(r["calls"]))


def test_entry_point(gpu_ctx):
    """model 0 through stx_match_features_model is stx_match_features bit for bit (a perspective scene, where the models differ); an unknown
    model is refused before anything is launched or written"""
    from tests.test_gpu_matches import _planted

    F = _planted(310, 300)
    rc_a, a = _call(gpu_ctx, F, None)
    rc_b, b = _call(gpu_ctx, F, _lib.MATCH_MODELS["homography"])
    assert rc_a == 0 and rc_b == 0
    for name in ("counts", "matches", "mask", "pick"):
        assert np.array_equal(a[name], b[name]), name
    assert np.array_equal(a["H"].view(np.uint64), b["H"].view(np.uint64)) and a["pick"][0, 0] >= 180 and a["H"][0, 6] != 0
    assert np.array_equal(a["info"][:2], b["info"][:2])
    rc_c, c = _call(gpu_ctx, F, _lib.MATCH_MODELS["affine_full"])
    assert rc_c == 0 and np.array_equal(c["matches"], a["matches"]) and not np.array_equal(c["H"], a["H"]) and c["H"][0, 6] == 0
    gpu_ctx.prof_enable(True)
    gpu_ctx.prof_reset()
    try:
        for model in (-1, 3, 7, 1 << 20):
            rc, out = _call(gpu_ctx, F, model)
            assert rc == -1  # STX_ERR_INVALID
            with pytest.raises(S.StitchingError, match="model"):
                _lib.check(rc)
            assert (out["counts"] == -7).all() and (out["H"] == 7.0).all() and (out["mask"] == 9).all() and (out["info"] == 7.0).all()
        assert _match_launches(gpu_ctx) == []
        assert _call(gpu_ctx, F, _lib.MATCH_MODELS["affine_partial"])[0] == 0
        assert _match_launches(gpu_ctx) == ["match_2nn", "match_pick", "match_ransac", "match_union"]
    finally:
        gpu_ctx.prof_enable(False)


def test_wrapper():
    feats = AR.planted_pair(90, 120, AR.SIMILARITY)
    want = NA.match(feats, ransac_iters=64)
    fm = S.FeatureMatcher("affine", estimator=S.MatchEstimator(model="affine", ransac_iters=64))
    got = fm.match_features(AR.package_features(feats))
    _same(got, want)
    assert got[1].confidence > 1 and np.allclose(got[2].H, np.linalg.inv(got[1].H), rtol=1e-9, atol=0.0)
