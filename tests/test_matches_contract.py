"""tests/numpy_matches.py is a matcher and not just a definition: on a rotated and shrunk copy and on two shifted crops of a textured image
it finds the transform, on unrelated textures it finds none; its closed-form homography equals the solution of the 8 x 8 system, its
sampler draws 4 distinct indices evenly, its ratio test rejects equality.  Also the host-side pieces of the package that need no GPU:
the threshold, the coordinates, the refit, the mirrored entries and the FeatureMatcher wrapper's numpy helpers.  The device is compared
with the contract in tests/test_gpu_matches.py."""
import json
import os

import numpy as np
import pytest

import stitching_amd as S
from stitching_amd import match_estimation as M
from tests import numpy_features as NF
from tests import numpy_matches as N
from tests.test_features_contract import _texture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "matches.json")
H_IMG, W_IMG = 240, 320
CORNERS = np.array([[0.0, 0.0], [W_IMG - 1.0, 0.0], [W_IMG - 1.0, H_IMG - 1.0], [0.0, H_IMG - 1.0]])  # x, y


def rotated_case():
    """a texture and its copy rotated by 30 degrees and shrunk by 1 / 1.2 about the centre -> images, the true map of pixels (x, y)"""
    from scipy.ndimage import affine_transform

    a = _texture(H_IMG, W_IMG, 7)
    th, s = np.deg2rad(30.0), 1.0 / 1.2
    rot = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])  # on (row, col)
    centre = np.array([(H_IMG - 1) / 2.0, (W_IMG - 1) / 2.0])
    inv = rot.T / s  # copy(o) = a(centre + inv (o - centre))
    b = np.stack([affine_transform(a[:, :, k], inv, offset=centre - inv @ centre, order=1, mode="reflect") for k in range(3)], axis=2)
    fwd = np.linalg.inv(inv)
    return [a, b], lambda p: (centre + (fwd @ (p[:, ::-1] - centre).T).T)[:, ::-1]


def shifted_case():
    """two crops of one texture whose content moves by (-150, -15) from the first to the second"""
    big = _texture(300, 520, 11)
    return [np.ascontiguousarray(big[20:20 + H_IMG, 20:20 + W_IMG]), np.ascontiguousarray(big[35:35 + H_IMG, 170:170 + W_IMG])], \
        lambda p: p - np.array([150.0, 15.0])


CASES = {"rotated_copy": rotated_case, "shifted_crops": shifted_case}
_MEASURED = {}


def measure(name):
    """the contract on the contract's features of a case -> entry (0, 1), and what profiles/matches.json records of it"""
    if name not in _MEASURED:
        imgs, true = CASES[name]()
        e = N.match([NF.detect(a) for a in imgs])[1]
        err = None
        if e["H"] is not None:
            half = np.array([W_IMG * 0.5, H_IMG * 0.5])  # level-0 pixel = centred coordinate + half the size
            q = np.concatenate([CORNERS - half, np.ones((4, 1))], axis=1) @ e["H"].T
            err = float(np.hypot(*(q[:, :2] / q[:, 2:3] + half - true(CORNERS)).T).max())
        _MEASURED[name] = (e, {"matches": int(len(e["matches"])), "inliers": int(e["num_inliers"]), "confidence": float(e["confidence"]),
                               "corner_error_px": err})
    return _MEASURED[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_contract_finds_the_transform(name):
    """confidence above 1; the refitted H takes the four image corners within 3 px (the inlier threshold) of the true transform"""
    e, rec = measure(name)
    print(f"{name}: {rec} (recorded: {json.load(open(PROFILE))['contract'][name]})")
    assert e["src_img_idx"] == 0 and e["dst_img_idx"] == 1
    assert e["confidence"] > 1
    assert rec["corner_error_px"] < 3.0
    assert e["num_inliers"] == int(e["inliers_mask"].sum()) >= 6 and 0 <= e["hypothesis"] < 500


def test_unrelated_textures_do_not_match():
    for sa, sb in ((7, 5), (11, 3), (2, 9)):
        e = N.match([NF.detect(_texture(H_IMG, W_IMG, sa)), NF.detect(_texture(H_IMG, W_IMG, sb))])
        assert len(e[1]["matches"]) < 6, (sa, sb, len(e[1]["matches"]))
        for k in (1, 2):
            assert e[k]["confidence"] == 0 and e[k]["H"] is None and e[k]["num_inliers"] == 0 and not e[k]["inliers_mask"].any()
        assert e[1]["H_sample"] is None and e[1]["hypothesis"] == -1


def _dlt(src, dst):
    """h22 = 1: the 8 x 8 system of 4 correspondences"""
    a, b = np.zeros((8, 8)), np.zeros(8)
    for k, ((x, y), (u, v)) in enumerate(zip(src, dst)):
        a[2 * k] = (x, y, 1, 0, 0, 0, -u * x, -u * y)
        a[2 * k + 1] = (0, 0, 0, x, y, 1, -v * x, -v * y)
        b[2 * k], b[2 * k + 1] = u, v
    return np.append(np.linalg.solve(a, b), 1.0)


def test_closed_form_is_the_homography_of_4_points():
    rs = np.random.RandomState(1)
    base = np.array([[-200.0, -150.0], [200.0, -150.0], [200.0, 150.0], [-200.0, 150.0]])
    worst = 0.0
    for _ in range(200):
        src = (base + rs.uniform(-60, 60, (4, 2)))[rs.permutation(4)]
        dst = src * rs.uniform(0.7, 1.4) + rs.uniform(-60, 60, (4, 2)) + rs.uniform(-300, 300, 2)
        h = N.closed_form(src, dst)
        want = _dlt(src, dst)
        worst = max(worst, float(np.abs(h / h[8] - want).max() / np.abs(want).max()))
    print(f"closed form against the 8 x 8 solve: {worst:.3g} relative")
    assert worst < 1e-8


def test_closed_form_sign_rule():
    """as it comes out of the closed form, H has W > 0 at its sample points only sometimes: the sign rule makes it always"""
    rs = np.random.RandomState(2)
    xyuv = np.concatenate([rs.uniform(-150, 150, (40, 2)), np.zeros((40, 2))], axis=1)
    xyuv[:, 2:] = xyuv[:, :2] * 1.1 + (20.0, -30.0)
    raw = fixed = 0
    for k in range(200):
        idx = N.sample(0x5EED, 1, k, 40)
        h = N.closed_form(xyuv[idx, 0:2], xyuv[idx, 2:4])
        raw += bool((h[6] * xyuv[idx[0], 0] + h[7] * xyuv[idx[0], 1]) + h[8] > 0)
        h, ok = N.hypothesis(xyuv, idx)
        fixed += bool(ok and N.inliers(h, xyuv, 9.0).all())
    assert raw < 150 and fixed == 200, (raw, fixed)


def test_sampler():
    """4 distinct indices in 0 .. m - 1 for m = 4 .. 70.  Evenness over 500 draws (2000 picks): an index is expected E = 2000 / m times
    with a standard deviation below sqrt(E); the +-40 % band is at least 4 of them wide while E >= 100, that is for m <= 20 — larger m
    would fail by chance, so the band is checked for m = 4 .. 20 (m = 4: every index in every draw)."""
    for m in range(4, 71):
        count = np.zeros(m, np.int64)
        for k in range(500):
            idx = N.sample(0x5EED, 3 * m + 1, k, m)
            assert len(idx) == 4 and len(set(idx)) == 4 and min(idx) >= 0 and max(idx) < m, (m, k, idx)
            count[idx] += 1
        if m <= 20:
            assert (np.abs(count - 2000.0 / m) <= 0.4 * 2000.0 / m).all(), (m, count)
    assert N.sample(0x5EED, 1, 0, 40) != N.sample(0x5EED, 2, 0, 40) and N.sample(0x5EED, 1, 0, 40) != N.sample(1, 1, 0, 40)
    assert N.mix32(0) == 0 and N.mix32(1) == 0x688990C0 and N.mix32(1 << 32) == 0  # uint32 throughout


def test_ratio_test_rejects_equality():
    T = N.ratio_threshold(0.5)
    assert T == 512 and N.ratio_threshold(0.3) == 717 and N.ratio_threshold(0.65) == 358 and N.ratio_threshold(0.0) == 1024
    assert not N.ratio_test(1, 2, T) and N.ratio_test(1, 3, T) and not N.ratio_test(0, 0, T) and N.ratio_test(0, 1, T)
    q = np.zeros((1, 32), np.uint8)
    one, two, three = (np.zeros(32, np.uint8) for _ in range(3))
    one[0], two[5], three[9] = 0x01, 0x03, 0x07
    far = np.full(32, 0xFF, np.uint8)
    assert len(N.union(q, np.array([far, one, two]), T)) == 0  # d1 = 1, d2 = 2: 1024 < 1024 is false; the backward pass finds duplicates
    m = N.union(q, np.array([far, three, one]), T)  # d1 = 1, d2 = 3
    assert m.tolist() == [[0, 2, 1]]
    assert M.ratio_threshold(0.5) == 512 and all(M.ratio_threshold(c) == N.ratio_threshold(c) for c in np.linspace(0, 1, 1001))


def _random_features(rs, idx, n):
    w0, h0 = int(rs.randint(100, 2000)), int(rs.randint(100, 2000))
    sizes = [(int(np.floor(w0 / 1.2 ** l + 0.5)), int(np.floor(h0 / 1.2 ** l + 0.5))) for l in range(5)]
    level = rs.randint(0, 5, n).astype(np.int32)
    x = np.array([rs.randint(0, sizes[l][0]) for l in level], np.int32)
    y = np.array([rs.randint(0, sizes[l][1]) for l in level], np.int32)
    return S.ImageFeatures(idx, (w0, h0), sizes, level, x, y, np.zeros(n, np.int32), np.zeros(n, np.int64), rs.randint(0, 256, (n, 32)).astype(np.uint8))


def test_host_helpers_equal_the_contract():
    rs = np.random.RandomState(3)
    for k in range(20):
        f = _random_features(rs, k, 50)
        got, want = M.centred_points(f), N.centred(f)
        assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert M.centred_points(_random_features(rs, 0, 0)).shape == (0, 2)
    f = S.ImageFeatures(0, (640, 480), [(640, 480), (533, 400)], np.array([0, 1], np.int32), np.array([0, 10], np.int32),
                        np.array([479, 7], np.int32), np.zeros(2, np.int32), np.zeros(2, np.int64), np.zeros((2, 32), np.uint8))
    assert M.centred_points(f)[0].tolist() == [-320.0, 239.0]
    assert M.centred_points(f)[1].tolist() == [(10 + 0.5) * 640 / 533 - 0.5 - 640 * 0.5, (7 + 0.5) * 480 / 400 - 0.5 - 480 * 0.5]
    H = np.array([[1.1, 0.05, 12.0], [-0.04, 0.95, -7.0], [1e-4, -2e-4, 1.0]])
    for n in (6, 7, 50):
        src = rs.uniform(-300, 300, (n, 2))
        q = np.concatenate([src, np.ones((n, 1))], axis=1) @ H.T
        dst = q[:, :2] / q[:, 2:3] + rs.uniform(-0.5, 0.5, (n, 2))
        got, want = M.refit_homography(src, dst), N.refit(src, dst)
        assert got[2, 2] == 1.0 and np.allclose(got, want, rtol=1e-9, atol=0.0) and np.abs(got - H)[:2, :2].max() < 0.02
        assert np.allclose(M.finite_inverse(got), N.inverse(want), rtol=1e-9, atol=0.0)
    for bad in (np.zeros((3, 3)), np.full((3, 3), np.nan), np.array([[1.0, 2, 3], [2, 4, 6], [0, 0, 1]])):
        assert M.finite_inverse(bad) is None and N.inverse(bad) is None
    for inl, m in ((6, 6), (165, 168), (30, 8), (31, 8), (100, 10), (0, 50)):
        assert M.match_confidence(inl, m) == N.confidence(inl, m)
    assert M.match_confidence(100, 10) == 0.0 and M.match_confidence(165, 168) == 165 / (8 + 0.3 * 168)


def test_mirrored_entries():
    mt = np.array([[0, 5, 10], [3, 1, 20], [4, 4, 0]], np.int32)
    H = np.array([[1.0, 0.1, 5.0], [0.0, 0.9, -3.0], [1e-4, 0.0, 1.0]])
    e = S.MatchesInfo(1, 3, mt, np.array([1, 0, 1], np.uint8), 2, H, 0.7, np.arange(9.0), 12)
    got = e.mirrored()
    want = N.mirrored({"matches": mt, "inliers_mask": e.inliers_mask, "num_inliers": 2, "H": H, "confidence": 0.7}, 1, 3)
    assert (got.src_img_idx, got.dst_img_idx) == (3, 1) == (want["src_img_idx"], want["dst_img_idx"])
    assert np.array_equal(got.matches, want["matches"]) and got.matches.tolist() == [[5, 0, 10], [1, 3, 20], [4, 4, 0]]
    assert np.array_equal(got.inliers_mask, want["inliers_mask"]) and got.num_inliers == 2 and got.confidence == 0.7
    assert np.array_equal(got.H, want["H"]) and np.allclose(got.H @ H, np.eye(3), atol=1e-12)
    assert got.H_sample is None and got.hypothesis == -1 and want["H_sample"] is None and want["hypothesis"] == -1
    m = got.getMatches()
    assert [(d.queryIdx, d.trainIdx, d.distance) for d in m] == [(5, 0, 10.0), (1, 3, 20.0), (4, 4, 0.0)]
    empty = S.MatchesInfo()
    assert (empty.src_img_idx, empty.dst_img_idx, empty.num_inliers, empty.confidence) == (-1, -1, 0, 0.0) and empty.H is None
    assert empty.matches.shape == (0, 3) and empty.matches.dtype == np.int32 and empty.getInliers().shape == (0,) and empty.getMatches() == []
    assert S.MatchEstimator().match([]) == []  # needs no device


def test_estimator_arguments():
    for kw in ({"match_conf": -0.1}, {"match_conf": 1.5}, {"ransac_threshold": -1.0}):
        with pytest.raises(S.StitchingError):
            S.MatchEstimator(**kw)
    e = S.MatchEstimator()
    assert (e.match_conf, e.range_width, e.ransac_iters, e.ransac_threshold, e.seed) == (0.3, -1, 500, 3.0, 0x5EED)
    assert (S.MatchEstimator.MAX_FEATURES, S.MatchEstimator.MAX_ITERS) == (65536, 4096)
    assert {"MatchEstimator", "MatchesInfo", "FeatureMatcher"} <= set(S.__all__)


def test_wrapper_helpers_without_cv2():
    """the values of the reference's helpers (stitching/feature_matcher.py:56-90)"""
    FM = S.FeatureMatcher
    assert FM.MATCHER_CHOICES == ("homography", "affine") and FM.DEFAULT_MATCHER == "homography" and FM.DEFAULT_RANGE_WIDTH == -1
    assert FM.get_default_match_conf("orb") == 0.3 and FM.get_default_match_conf("sift") == 0.65 and FM.get_default_match_conf("x") == 0.65
    assert FM.get_match_conf(None, "orb") == 0.3 and FM.get_match_conf(None, "sift") == 0.65 and FM.get_match_conf(0.4, "orb") == 0.4
    assert np.array_equal(FM.array_in_square_matrix(list(range(9))), np.arange(9).reshape(3, 3))
    assert [(int(i), int(j)) for i, j in FM.get_all_img_combinations(4)] == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    infos = [S.MatchesInfo(confidence=c) for c in (0.0, 1.5, 0.2, 1.5, 0.0, 2.5, 0.2, 2.5, 0.0)]
    mm = FM.get_matches_matrix(infos)
    assert mm.shape == (3, 3) and mm[1, 2] is infos[5] and mm[2, 0] is infos[6]
    assert np.array_equal(FM.get_confidence_matrix(infos), np.array([[0.0, 1.5, 0.2], [1.5, 0.0, 2.5], [0.2, 2.5, 0.0]]))

    class Canned:
        def match(self, features):
            return ["canned", features]

    fm = FM(estimator=Canned(), range_width=3)
    assert fm.matcher is None and fm.match_features([1, 2]) == ["canned", [1, 2]]
    with pytest.raises(S.StitchingError, match="affine"):
        FM("affine", estimator=Canned())
    with pytest.raises(S.StitchingError):
        FM(estimator=Canned(), match_conf=0.3)
    with pytest.raises(S.StitchingError):
        fm.match_features([1, 2], None)
    try:
        import cv2  # noqa: F401
    except ImportError:
        for name in FM.MATCHER_CHOICES:  # the names stay cv2's: without it they raise, they do not fall to the device
            with pytest.raises(S.StitchingError, match="OpenCV"):
                FM(name)
        with pytest.raises(S.StitchingError, match="OpenCV"):
            FM.draw_matches(None, None, None, None, None)
