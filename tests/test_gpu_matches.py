"""The project's own descriptor matcher and homography RANSAC on the MI355X (stitching_amd.MatchEstimator, csrc/stx_matches.hip) against
its contract tests/numpy_matches.py: every integer array and the float64 bits of H_sample equal, H and confidence within 1e-9 relative.
Inputs are synthetic ImageFeatures (no images) except for one end-to-end case; the contract's result of an input is computed once."""
import numpy as np
import pytest

import stitching_amd as S
from tests import numpy_features as NF
from tests import numpy_matches as N

pytestmark = pytest.mark.gpu

FIELDS = ("src_img_idx", "dst_img_idx", "num_inliers", "hypothesis")


def _feat(idx, desc, xy, size=(640, 480), levels=None, level=None):
    """ImageFeatures of descriptors (n, 32) u8 at integer level pixels xy (n, 2); one level of the image's size unless told otherwise"""
    xy = np.asarray(xy, np.int32).reshape(-1, 2)
    n = len(xy)
    level = np.zeros(n, np.int32) if level is None else np.asarray(level, np.int32)
    return S.ImageFeatures(idx, size, [size] if levels is None else levels, level, xy[:, 0].copy(), xy[:, 1].copy(), np.zeros(n, np.int32),
                           np.zeros(n, np.int64), np.ascontiguousarray(np.asarray(desc, np.uint8).reshape(n, 32)))


def _pool(rs, n):
    """n random 256-bit descriptors: mutual distances near 128"""
    return rs.randint(0, 256, (n, 32)).astype(np.uint8)


def _flip(rs, d, bits):
    """a copy of descriptor d with `bits` distinct bits flipped"""
    out = d.copy()
    for b in rs.choice(256, bits, replace=False):
        out[b // 8] ^= 1 << (b % 8)
    return out


def _same(got, want):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        for name in FIELDS:
            assert getattr(g, name) == w[name], (k, name, getattr(g, name), w[name])
        for name, dtype, shape in (("matches", np.int32, w["matches"].shape), ("inliers_mask", np.uint8, w["inliers_mask"].shape)):
            a = getattr(g, name)
            assert isinstance(a, np.ndarray) and a.dtype == dtype and a.shape == shape, (k, name, a.dtype, a.shape, shape)
            assert np.array_equal(a, w[name]), (k, name, int(np.count_nonzero(a != w[name])))
        assert np.array_equal(g.getInliers(), w["inliers_mask"]) and len(g.getMatches()) == len(w["matches"])
        assert (g.H_sample is None) == (w["H_sample"] is None), (k, "H_sample")
        if w["H_sample"] is not None:
            assert g.H_sample.dtype == np.float64 and g.H_sample.shape == (9,)
            assert np.array_equal(g.H_sample.view(np.uint64), w["H_sample"].view(np.uint64)), (k, g.H_sample, w["H_sample"])
        assert (g.H is None) == (w["H"] is None), (k, "H")
        if w["H"] is not None:
            assert np.allclose(g.H, w["H"], rtol=1e-9, atol=0.0), (k, g.H, w["H"])
        assert g.confidence == pytest.approx(w["confidence"], rel=1e-9, abs=0.0), (k, "confidence")


_REFS = {}


def _check(key, feats, **kw):
    """the device on `feats` against the contract's result (computed once per key); the inputs stay as they were"""
    before = [(f.descriptors.copy(), f.x.copy(), f.y.copy(), f.level.copy()) for f in feats]
    est = S.MatchEstimator(**kw)
    got = est.match(feats)
    if key not in _REFS:
        _REFS[key] = N.match(feats, **kw)
    _same(got, _REFS[key])
    for f, (d, x, y, l) in zip(feats, before):
        assert np.array_equal(f.descriptors, d) and np.array_equal(f.x, x) and np.array_equal(f.y, y) and np.array_equal(f.level, l)
    n = len(feats)
    assert est.info["pairs"] == sum(1 for e in got if 0 <= e.src_img_idx < e.dst_img_idx)
    assert est.info["matches"] == sum(len(got[i * n + j].matches) for i in range(n) for j in range(i + 1, n))
    return got, _REFS[key]


def _scene(seed, counts, noise_bits=12, pool=700):
    """images that show random subsets of one pool of landmarks, each through its own integer translation with a pixel of noise"""
    rs = np.random.RandomState(seed)
    D, P = _pool(rs, pool), rs.randint(100, 540, (pool, 2))
    feats = []
    for i, c in enumerate(counts):
        pick = rs.permutation(pool)[:c]
        d = np.array([_flip(rs, D[k], rs.randint(0, noise_bits + 1)) for k in pick], np.uint8).reshape(c, 32)
        xy = P[pick] + rs.randint(-40, 41, 2)[None, :] + rs.randint(-1, 2, (c, 2))
        feats.append(_feat(i, d, xy))
    return feats


def test_feature_counts():
    """0, 1, 2 features and the counts around the wavefront (64) and the workgroup / LDS tile (256), unequal within the list"""
    counts = (0, 1, 2, 63, 64, 65, 255, 256, 257, 600)
    got, want = _check("counts", _scene(1, counts), ransac_iters=32)
    n = len(counts)
    assert all(len(got[j].matches) == 0 and got[j].src_img_idx == 0 for j in range(1, n))  # an image without features: processed, empty
    assert got[0].src_img_idx == -1 and got[0].dst_img_idx == -1  # the diagonal
    assert sum(1 for e in want if e["num_inliers"] >= 6) >= 20 and max(len(e["matches"]) for e in want) > 200


def _ties():
    rs = np.random.RandomState(2)
    base = _pool(rs, 1)[0]
    alphabet = np.array([base, _flip(rs, base, 1), _flip(rs, base, 3), _flip(rs, base, 40)], np.uint8)
    draw = lambda n: alphabet[rs.randint(0, 4, n)]  # noqa: E731
    xy = lambda n: rs.randint(20, 600, (n, 2))  # noqa: E731
    return [_feat(0, draw(70), xy(70)), _feat(1, alphabet, xy(4)), _feat(2, draw(130), xy(130)), _feat(3, alphabet[[3, 0, 0, 1]], xy(4)),
             _feat(4, draw(5), xy(5))]


def test_ties_and_duplicates():
    """4 descriptor values: ties at every distance, duplicates that give d1 == d2 == 0; an image with each value once is matched into"""
    feats = _ties()
    for conf in (0.3, 0.0):  # T = 717, and T = 1024: equality of d1 and d2 still rejected
        got, want = _check(("ties", conf), feats, match_conf=conf, ransac_iters=16)
        assert len(want[0 * 5 + 1]["matches"]) == 70 and len(want[1 * 5 + 2]["matches"]) == 130  # many to one, from either side
        assert len(want[0 * 5 + 2]["matches"]) == 0  # duplicates on both sides: d1 == d2 == 0 everywhere


def test_ratio_test_rejects_equality():
    """match_conf = 0.5 (T = 512): d1 = 1, d2 = 2 is rejected, d1 = 1, d2 = 3 accepted"""
    one, two, three = (np.zeros(32, np.uint8) for _ in range(3))
    one[0], two[5], three[9] = 0x01, 0x03, 0x07
    far, q, xy = np.full(32, 0xFF, np.uint8), np.zeros((1, 32), np.uint8), np.arange(6).reshape(3, 2) + 50
    got, want = _check("ratio", [_feat(0, q, xy[:1]), _feat(1, np.array([far, one, two]), xy), _feat(2, np.array([far, three, one]), xy)],
                       match_conf=0.5, ransac_iters=4)
    assert len(got[1].matches) == 0 and got[2].matches.tolist() == [[0, 2, 1]]


def test_uniform_train_loads(monkeypatch):
    """STX_MATCH_TRAIN=uniform (the other way match_2nn can take the train descriptors) gives the same results"""
    monkeypatch.setenv("STX_MATCH_TRAIN", "uniform")
    _check("extras", _extras(True), ransac_iters=64)
    _check(("planted", 300), _planted(310, 300), ransac_iters=200)
    _check(("ties", 0.3), _ties(), match_conf=0.3, ransac_iters=16)


def _extras(with_extras):
    rs = np.random.RandomState(3)
    D = _pool(rs, 40)
    P = rs.randint(50, 590, (40, 2))
    b_desc, b_xy = [d for d in D[:30]], [p for p in P[:30] + (7, -5)]
    if with_extras:  # two noisy copies of landmarks 30 .. 34 and no exact one: forward d1 == d2, backward a clear winner each
        for k in range(30, 35):
            for _ in range(2):
                b_desc.append(_flip(rs, D[k], 10))
                b_xy.append(P[k] + (7, -5))
    return [_feat(0, D[:35], P[:35]), _feat(1, np.array(b_desc), np.array(b_xy))]


def test_backward_extras():
    got, want = _check("extras", _extras(True), ransac_iters=64)
    m = want[1]["matches"]
    assert len(m) == 40 and np.array_equal(m[:30, 0], np.arange(30)) and np.array_equal(m[30:, 1], np.arange(30, 40))
    assert np.array_equal(m[30:, 0], np.repeat(np.arange(30, 35), 2)) and (m[30:, 2] == 10).all()
    got, want = _check("no extras", _extras(False), ransac_iters=64)
    assert len(want[1]["matches"]) == 30  # the backward pass finds the forward pairs again and adds none


@pytest.mark.parametrize("width", (1, 2))
def test_range_width(width):
    got, want = _check(("range", width), _scene(4, (40, 45, 50, 55, 60), pool=80), range_width=width, ransac_iters=32)
    for i in range(5):
        for j in range(5):
            e = got[i * 5 + j]
            if i != j and abs(i - j) <= width:
                assert (e.src_img_idx, e.dst_img_idx) == (i, j) and len(e.matches) > 6
            else:
                assert (e.src_img_idx, e.dst_img_idx) == (-1, -1) and len(e.matches) == 0 and e.H is None and e.confidence == 0.0


PERSPECTIVE = np.array([[0.9, -0.12, 14.0], [0.1, 1.05, -9.0], [2.0e-4, -1.0e-4, 1.0]])


def _planted(seed, m, H=PERSPECTIVE, outliers=0.3, size=(640, 480), size_b=(640, 480), extra=9):
    """m landmarks seen in two images, the second through H (in centred level-0 pixels, rounded to the pixel grid of one of two levels);
    a share of them land at random places instead; `extra` unrelated descriptors per image"""
    rs = np.random.RandomState(seed)
    D = _pool(rs, m + 2 * extra)
    c = np.stack([rs.randint(-size[0] // 2 + 20, size[0] // 2 - 20, m), rs.randint(-size[1] // 2 + 20, size[1] // 2 - 20, m)], axis=1)
    q = np.concatenate([c, np.ones((m, 1))], axis=1) @ H.T
    d = q[:, :2] / q[:, 2:3]
    bad = rs.permutation(m)[:int(round(outliers * m))]
    d[bad] = np.stack([rs.randint(-size_b[0] // 2, size_b[0] // 2, len(bad)), rs.randint(-size_b[1] // 2, size_b[1] // 2, len(bad))], axis=1)
    lv_a = [size, (size[0] // 2, size[1] // 2)]
    lv_b = [size_b, (size_b[0] // 2, size_b[1] // 2)]
    la, lb = rs.randint(0, 2, m + extra), rs.randint(0, 2, m + extra)
    pa = np.concatenate([c, rs.randint(-200, 200, (extra, 2))]) + (size[0] // 2, size[1] // 2)
    pb = np.concatenate([np.rint(d), rs.randint(-200, 200, (extra, 2))]) + (size_b[0] // 2, size_b[1] // 2)
    pa, pb = pa // (1 + la[:, None]), pb.astype(np.int64) // (1 + lb[:, None])  # the pixel of the level: half resolution at level 1
    order = rs.permutation(m + extra)
    da = np.concatenate([D[:m], D[m:m + extra]])
    db = np.concatenate([D[:m], D[m + extra:]])[order]
    return [_feat(0, da, pa, size, lv_a, la), _feat(1, db, pb[order], size_b, lv_b, lb[order])]


@pytest.mark.parametrize("m", (5, 6, 7, 64, 65, 300))
def test_planted_homography(m):
    got, want = _check(("planted", m), _planted(10 + m, m), ransac_iters=200)
    e = got[1]
    assert len(e.matches) == m
    if m == 5:
        assert e.H is None and e.H_sample is None and e.hypothesis == -1 and e.confidence == 0.0 and e.num_inliers == 0
    if m >= 64:
        assert e.num_inliers >= int(0.6 * m) and e.confidence > 1 and np.abs(e.H / PERSPECTIVE[2, 2] - PERSPECTIVE)[:2, :2].max() < 0.05
        back = got[2]
        assert (back.src_img_idx, back.dst_img_idx) == (1, 0) and np.array_equal(back.matches[:, [1, 0, 2]], e.matches)
        assert np.allclose(back.H @ e.H, np.eye(3), atol=1e-9) and back.confidence == e.confidence and back.H_sample is None


def test_hypothesis_ties():
    """a pure integer translation without outliers: every hypothesis has every match as an inlier, the smallest k wins"""
    rs = np.random.RandomState(20)
    D, xy, order = _pool(rs, 50), rs.randint(40, 440, (50, 2)), rs.permutation(50)
    T = np.array([[1.0, 0.0, 31.0], [0.0, 1.0, -17.0], [0.0, 0.0, 1.0]])
    feats = [_feat(0, D, xy), _feat(1, D[order], xy[order] + (31, -17))]
    got, want = _check("translation", feats, ransac_iters=64)
    assert got[1].hypothesis == 0 and got[1].num_inliers == 50 and np.abs(got[1].H - T).max() < 1e-9


@pytest.mark.parametrize("kind", ("collinear", "equal"))
def test_degenerate_geometry(kind):
    rs = np.random.RandomState(30)
    D = _pool(rs, 40)
    t = np.arange(40)
    xy = np.stack([100 + 10 * t, 50 + 5 * t], axis=1) if kind == "collinear" else np.full((40, 2), 77)
    got, want = _check(("degenerate", kind), [_feat(0, D, xy), _feat(1, D[::-1], xy[::-1] + (3, 4))], ransac_iters=64)
    assert len(got[1].matches) == 40
    if kind == "equal":  # M is singular: H is all zeros, W at sample point 0 is 0, no hypothesis has inliers
        assert got[1].num_inliers == 0 and got[1].hypothesis == 0 and not got[1].H_sample.any() and got[1].H is None


def test_negative_w():
    """a horizon through the first image: the landmarks behind it land where W < 0 and are no inliers, however well they fit"""
    H = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [1.0 / 100.0, 0.0, 1.0]])
    rs = np.random.RandomState(40)
    m = 120
    D = _pool(rs, m)
    c = np.stack([np.where(np.arange(m) % 3 == 0, rs.randint(-300, -130, m), rs.randint(-60, 300, m)), rs.randint(-200, 200, m)], axis=1)
    w = c[:, 0] / 100.0 + 1.0
    d = np.rint(c / w[:, None]).astype(np.int64)
    feats = [_feat(0, D, c + (320, 240)), _feat(1, D, d + (2000, 2000), size=(4000, 4000))]
    got, want = _check("negative w", feats, ransac_iters=200)
    e = got[1]
    behind = w[e.matches[:, 0]] < 0
    assert len(e.matches) == m and behind.sum() == 40 and e.num_inliers >= 60 and not e.inliers_mask[behind].any()


@pytest.mark.parametrize("iters", (1, 64, 4096))
def test_ransac_iters(iters):
    got, want = _check(("iters", iters), _planted(50, 40), ransac_iters=iters)
    assert 0 <= got[1].hypothesis < iters


def test_seed():
    feats = _planted(60, 80)
    a, wa = _check("seed default", feats, ransac_iters=64)
    b, wb = _check("seed other", feats, ransac_iters=64, seed=12345)
    assert wa[1]["hypothesis"] != wb[1]["hypothesis"] and np.array_equal(a[1].matches, b[1].matches)
    assert not np.array_equal(a[1].H_sample, b[1].H_sample)


def test_repeatability():
    feats = _scene(70, (150, 300, 90))
    a = S.MatchEstimator(ransac_iters=100).match(feats)
    b = S.MatchEstimator(ransac_iters=100).match(feats)
    for x, y in zip(a, b):
        assert np.array_equal(x.matches, y.matches) and np.array_equal(x.inliers_mask, y.inliers_mask) and x.hypothesis == y.hypothesis
        assert (x.H_sample is None and y.H_sample is None) or np.array_equal(x.H_sample.view(np.uint64), y.H_sample.view(np.uint64))
        assert (x.H is None and y.H is None) or np.array_equal(x.H, y.H)
        assert x.confidence == y.confidence


def test_limits_are_refused_before_any_launch(gpu_ctx):
    rs = np.random.RandomState(80)
    good = _feat(0, _pool(rs, 10), rs.randint(0, 400, (10, 2)))
    gpu_ctx.prof_enable(True)
    gpu_ctx.prof_reset()
    try:
        many = S.MatchEstimator.MAX_FEATURES + 1
        with pytest.raises(S.StitchingError, match="65536"):
            S.MatchEstimator().match([good, _feat(1, np.zeros((many, 32), np.uint8), np.zeros((many, 2), np.int32))], ctx=gpu_ctx)
        for iters in (0, -3, 4097):
            with pytest.raises(S.StitchingError, match="4096"):
                S.MatchEstimator(ransac_iters=iters).match([good, good], ctx=gpu_ctx)
        for desc in (np.zeros((10, 16), np.uint8), np.zeros((10, 64), np.uint8), np.zeros((10, 32), np.int32), np.zeros((10, 32), np.float32)):
            bad = _feat(1, _pool(rs, 10), rs.randint(0, 400, (10, 2)))
            bad.descriptors = desc
            with pytest.raises(S.StitchingError, match="n x 32 u8"):
                S.MatchEstimator().match([good, bad], ctx=gpu_ctx)
        bad = _feat(1, _pool(rs, 10), rs.randint(0, 400, (10, 2)))
        bad.descriptors = bad.descriptors[:9]
        with pytest.raises(S.StitchingError, match="9 descriptors and 10 keypoints"):
            S.MatchEstimator().match([good, bad], ctx=gpu_ctx)
        assert not [r["kernel"] for r in gpu_ctx.prof_results() if r["kernel"].startswith("match_")]
        S.MatchEstimator(ransac_iters=8).match([good, good], ctx=gpu_ctx)
        launched = sorted(r["kernel"] for r in gpu_ctx.prof_results() if r["kernel"].startswith("match_"))
        assert launched == ["match_2nn", "match_pick", "match_ransac", "match_union"]
    finally:
        gpu_ctx.prof_enable(False)


def test_wrapper():
    feats = _scene(90, (120, 140, 100), pool=200)
    want = N.match(feats, ransac_iters=64)
    fm = S.FeatureMatcher(estimator=S.MatchEstimator(ransac_iters=64))
    got = fm.match_features(feats)
    _same(got, want)
    conf = S.FeatureMatcher.get_confidence_matrix(got)
    assert conf.shape == (3, 3) and np.allclose(conf, np.array([e["confidence"] for e in want]).reshape(3, 3), rtol=1e-9, atol=0.0)
    assert (np.diag(conf) == 0).all() and np.array_equal(conf, conf.T) and conf[0, 1] > 1
    mm = S.FeatureMatcher.get_matches_matrix(got)
    for i, j in S.FeatureMatcher.get_all_img_combinations(3):
        a, b = mm[i, j], mm[j, i]
        assert (b.src_img_idx, b.dst_img_idx) == (j, i) and np.array_equal(b.matches, a.matches[:, [1, 0, 2]])
        assert np.array_equal(b.inliers_mask, a.inliers_mask) and b.num_inliers == a.num_inliers
        assert np.allclose(b.H, np.linalg.inv(a.H), rtol=1e-9, atol=0.0)
    with pytest.raises(S.StitchingError, match="affine"):
        S.FeatureMatcher("affine", estimator=S.MatchEstimator())


def test_end_to_end_shifted_crops():
    """FeatureEstimator.detect on two crops of one texture shifted by (150, 15), then MatchEstimator: the contract on the contract"""
    from tests.test_features_contract import _texture

    big = _texture(300, 520, 11)
    imgs = [np.ascontiguousarray(big[20:260, 20:340]), np.ascontiguousarray(big[35:275, 170:490])]
    feats = S.FeatureEstimator().detect(imgs)
    want = N.match([NF.detect(a) for a in imgs])
    got = S.MatchEstimator().match(feats)
    _same(got, want)
    assert got[1].confidence > 1 and abs(got[1].H[0, 2] + 150) < 1 and abs(got[1].H[1, 2] + 15) < 1
