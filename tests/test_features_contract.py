"""tests/numpy_features.py is a detector and not just a definition: its score and response equal independent statements of them, its
keypoints move with the image content, and on a rotated and shrunk copy of a textured image its descriptors find their counterparts —
better with the orientation than without.  Also the host-side pieces of the package that need no GPU: quotas, level sizes, the pattern,
the tables, ImageFeatures and the FeatureDetector wrapper.  The device is compared with the contract in tests/test_gpu_features.py."""
import json
import os
import sys

import numpy as np
import pytest

import stitching_amd as S
from stitching_amd import feature_estimation as F
from tests import numpy_features as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "features.json")


def _noise(h, w, seed):
    a = np.random.RandomState(seed).randint(0, 256, (h, w)).astype(np.uint16)
    return ((a + np.roll(a, 1, 0) + np.roll(a, 1, 1) + np.roll(a, (1, 1), (0, 1)) + 2) // 4).astype(np.uint8)


def _three(h, w, seed):
    cells = np.random.RandomState(seed).randint(0, 3, ((h + 2) // 3, (w + 2) // 3))
    return np.array([40, 120, 220], np.uint8)[np.kron(cells, np.ones((3, 3), np.int64))[:h, :w]]


def _texture(h, w, seed):
    """blobs of several sizes: corners at every level of the pyramid"""
    from scipy.ndimage import gaussian_filter

    rs = np.random.RandomState(seed)
    t = sum(gaussian_filter(rs.standard_normal((h, w)), s) * s for s in (1.5, 3.0, 6.0))
    t = (t - t.min()) / (t.max() - t.min())
    g = (255 * (0.5 + 0.5 * np.sign(t - 0.5) * np.abs(2 * t - 1) ** 0.5)).astype(np.uint8)  # steepened: edges and corners, not slopes
    return np.repeat(g[:, :, None], 3, axis=2)


def _segment_test_count(g):
    """the independent statement: the number of t in 0 .. 254 at which 9 contiguous ring pixels are all > c + t or all < c - t"""
    g = g.astype(np.int32)
    h, w = g.shape
    c = g[3:h - 3, 3:w - 3]
    ring = np.stack([g[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] for dx, dy in N.RING])
    count = np.zeros(c.shape, np.int32)
    for t in range(255):
        passed = np.zeros(c.shape, bool)
        for side in (ring > c + t, ring < c - t):
            if not side.any():
                continue
            twice = np.concatenate([side, side[:8]])
            run = np.ones_like(side)
            for k in range(9):
                run &= twice[k:k + 16]
            passed |= run.any(axis=0)
        count += passed
    return count


@pytest.mark.parametrize("make", (_noise, _three))
def test_score_counts_the_thresholds_the_segment_test_passes(make):
    g = make(41, 47, 3)
    s = N.score_map(g)
    assert (s[:3] == N.NO_SCORE).all() and (s[:, -3:] == N.NO_SCORE).all()
    inner = s[3:-3, 3:-3].astype(np.int32)
    assert inner.min() >= -255 and inner.max() <= 255 and inner.max() > 20
    assert np.array_equal(np.maximum(inner, 0), _segment_test_count(g))


def test_response_is_the_floor_of_the_float_formula():
    for g in (_noise(60, 70, 1), _three(60, 70, 2), np.full((40, 40), 9, np.uint8)):
        ys, xs = np.mgrid[4:g.shape[0] - 4, 4:g.shape[1] - 4]
        ys, xs = ys.ravel(), xs.ravel()
        f = g.astype(np.float64)
        ix, iy = np.zeros_like(f), np.zeros_like(f)
        ix[:, 1:-1], iy[1:-1, :] = f[:, 2:] - f[:, :-2], f[2:, :] - f[:-2, :]
        box = lambda m: np.array([m[y - 3:y + 4, x - 3:x + 4].sum() for y, x in zip(ys, xs)])  # noqa: E731
        a, b, c = box(ix * ix), box(ix * iy), box(iy * iy)
        want = np.floor((25.0 * (a * c - b * b) - (a + c) ** 2) / 65536.0)  # every term an integer below 2^53: exact
        got = N.response(g, ys, xs)
        assert got.dtype == np.int64 and np.array_equal(got, want.astype(np.int64))
        assert np.abs(got).max() < 2 ** 33
    assert (N.response(np.full((40, 40), 9, np.uint8), [20], [20]) == 0).all()


@pytest.mark.parametrize("shift", ((5, 0), (0, 7), (-3, 4), (11, -9)))
def test_keypoints_move_with_the_content(shift):
    """nlevels = 1, every candidate kept: a keypoint whose 31 x 31 patch lies inside both crops is found in both, same bin, same bytes"""
    dx, dy = shift
    big = _texture(200, 220, 11)
    h, w, oy, ox = 120, 140, 30, 30
    a = N.detect(big[oy:oy + h, ox:ox + w], nlevels=1, nfeatures=60000)
    b = N.detect(big[oy - dy:oy - dy + h, ox - dx:ox - dx + w], nlevels=1, nfeatures=60000)  # the content moves by (+dx, +dy)
    inside = lambda x, y: (x >= 16) & (x <= w - 17) & (y >= 16) & (y <= h - 17)  # noqa: E731
    ka = inside(a["x"] + dx, a["y"] + dy)
    kb = inside(b["x"] - dx, b["y"] - dy)
    assert ka.sum() > 20 and ka.sum() == kb.sum()
    pa = {(int(x) + dx, int(y) + dy): (int(bn), int(r), d.tobytes()) for x, y, bn, r, d in
          zip(a["x"][ka], a["y"][ka], a["bin"][ka], a["R"][ka], a["descriptors"][ka])}
    pb = {(int(x), int(y)): (int(bn), int(r), d.tobytes()) for x, y, bn, r, d in
          zip(b["x"][kb], b["y"][kb], b["bin"][kb], b["R"][kb], b["descriptors"][kb])}
    assert pa == pb


def _points(r):
    """level-0 positions of a result's keypoints, (n, 2) as x, y"""
    w0, h0 = r["level_sizes"][0]
    wl = np.array([s[0] for s in r["level_sizes"]], np.float64)[r["level"]]
    hl = np.array([s[1] for s in r["level_sizes"]], np.float64)[r["level"]]
    return np.stack([(r["x"] + 0.5) * w0 / wl - 0.5, (r["y"] + 0.5) * h0 / hl - 0.5], axis=1)


def matching_share(seed, upright):
    """A textured image and its copy rotated by 30 degrees and shrunk by 1 / 1.2 about the centre: the share of the first image's
    keypoints (among those whose true counterpart lies inside the copy's border) whose Hamming-nearest descriptor in the copy lies
    within 3 pixels of that counterpart."""
    from scipy.ndimage import affine_transform

    h, w = 240, 320
    a = _texture(h, w, seed)
    th, s = np.deg2rad(30.0), 1.0 / 1.2
    rot = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])  # on (row, col)
    centre = np.array([(h - 1) / 2.0, (w - 1) / 2.0])
    inv = rot.T / s  # copy(o) = a(centre + inv (o - centre))
    b = np.stack([affine_transform(a[:, :, k], inv, offset=centre - inv @ centre, order=1, mode="reflect") for k in range(3)], axis=2)
    ra, rb = N.detect(a, upright=upright), N.detect(b, upright=upright)
    pa, pb = _points(ra), _points(rb)
    true = (centre + (np.linalg.inv(inv) @ (pa[:, ::-1] - centre).T).T)[:, ::-1]  # counterparts in the copy, as x, y
    ok = (true[:, 0] >= 16) & (true[:, 0] <= w - 17) & (true[:, 1] >= 16) & (true[:, 1] <= h - 17)
    bits_a, bits_b = np.unpackbits(ra["descriptors"], axis=1), np.unpackbits(rb["descriptors"], axis=1)
    dist = (bits_a[:, None, :] != bits_b[None, :, :]).sum(axis=2)
    nearest = pb[np.argmin(dist, axis=1)]
    hit = np.hypot(nearest[:, 0] - true[:, 0], nearest[:, 1] - true[:, 1]) <= 3.0
    return float(hit[ok].sum()) / float(ok.sum()), int(ok.sum())


def test_descriptors_find_their_counterparts_on_a_rotated_shrunk_copy():
    rec = json.load(open(PROFILE))["matching"]
    share, n = matching_share(rec["seed"], upright=False)
    wrong, _ = matching_share(rec["seed"], upright=True)
    print(f"share {share:.4f} of {n} keypoints (recorded {rec['share']:.4f}); with every bin forced to 0: {wrong:.4f}")
    assert n >= 100
    assert share >= 0.9 * rec["share"], (share, rec["share"])
    assert share > wrong, (share, wrong)


def test_quotas():
    assert N.quotas(500, 1.2, 8) == [109, 90, 75, 63, 52, 44, 36, 31]  # the plain series where its rounding fits
    assert N.quotas(500, 1.2, 1) == [500] and N.quotas(1, 1.2, 8) == [0] * 7 + [1] and N.quotas(500, 1.2, 0) == []
    for scale in (1.05, 1.2, 1.5, 2.0, 3.0):
        for levels in range(1, 17):
            for nfeatures in list(range(1, 130)) + [500, 4999, 65536]:
                q = N.quotas(nfeatures, scale, levels)
                assert len(q) == levels and min(q) >= 0 and sum(q) <= nfeatures, (nfeatures, scale, levels, q)
                assert q == F.level_quotas(nfeatures, scale, levels)
    assert sum(N.quotas(7, 1.2, 8)) == 7  # its rounded terms alone add up to 8
    # against the issue's series written out here, without the cap: equal wherever that series fits, term by term
    fits = 0
    for nfeatures in range(1, 700):
        for levels in range(1, 10):
            d, plain = nfeatures * (1 - 1 / 1.2) / (1 - (1 / 1.2) ** levels), []
            for _ in range(levels - 1):
                plain.append(int(np.floor(d + 0.5)))
                d *= 1 / 1.2
            if sum(plain) <= nfeatures:
                fits += 1
                assert N.quotas(nfeatures, 1.2, levels) == plain + [nfeatures - sum(plain)]
    assert fits > 6000


def test_dropped_levels():
    assert N.level_sizes(200, 150, 8, 1.2)[-1] == (56, 42) and len(N.level_sizes(200, 150, 12, 1.2)) == 9  # 150 / 1.2**9 = 29.07
    assert N.level_sizes(33, 33, 8, 1.2) == [(33, 33)] and N.level_sizes(32, 400, 8, 1.2) == [] and N.level_sizes(400, 32, 8, 1.2) == []
    for w0, h0 in ((200, 150), (641, 937), (33, 50)):
        ls = N.level_sizes(w0, h0, 16, 1.2)
        assert ls == F.level_sizes(w0, h0, 16, 1.2)
        assert all(s == (int(np.floor(w0 / 1.2 ** l + 0.5)), int(np.floor(h0 / 1.2 ** l + 0.5))) for l, s in enumerate(ls))
        nxt = (np.floor(w0 / 1.2 ** len(ls) + 0.5), np.floor(h0 / 1.2 ** len(ls) + 0.5))
        assert len(ls) == 16 or min(nxt) < 33
    img = np.repeat(_noise(150, 200, 4)[:, :, None], 3, axis=2)
    r = N.detect(img, nlevels=12, fast_threshold=5)
    assert len(r["level_sizes"]) == 9 and r["level"].max() <= 8
    pyr = N.pyramid(N.grey(img), 12, 1.2)
    assert [p.shape for p in pyr] == [(h, w) for w, h in r["level_sizes"]]
    none = N.detect(img[:32], nlevels=8)
    assert len(none["x"]) == 0 and none["descriptors"].shape == (0, 32) and none["level_sizes"] == []


def test_pattern_and_tables():
    p = F.pattern()
    assert p.shape == (256, 4) and p.dtype == np.int8 and not p.flags.writeable
    q = p.astype(np.int64)
    assert (q[:, 0] ** 2 + q[:, 1] ** 2 <= 169).all() and (q[:, 2] ** 2 + q[:, 3] ** 2 <= 169).all()
    assert ((q[:, 0] != q[:, 2]) | (q[:, 1] != q[:, 3])).all()
    assert len({tuple(r) for r in q.tolist()}) > 250  # pairs, not one pair 256 times
    rot = N.rotated_patterns()
    assert np.array_equal(rot, F.rotated_patterns().astype(np.int64)) and np.abs(rot).max() <= 13
    assert np.array_equal(rot[0], q) and np.array_equal(rot[9, :, 0], -q[:, 1]) and np.array_equal(rot[9, :, 1], q[:, 0])  # 90 degrees
    assert np.array_equal(np.concatenate([N.CX, N.CY]), F.direction_tables())
    assert N.CX[0] == 16384 and N.CY[9] == 16384 and N.CX[18] == -16384 and N.CY[27] == -16384


def test_contract_is_the_grey_blur_and_resize_it_states():
    from oracle import oracle as O

    rs = np.random.RandomState(8)
    img = rs.randint(0, 256, (37, 45, 3)).astype(np.uint8)
    g = N.grey(img)
    assert g.dtype == np.uint8 and N.grey(np.full((2, 2, 3), 255, np.uint8)).max() == 255 and 1868 + 9617 + 4899 == 1 << 14
    assert np.array_equal(N.resize_linear_exact(g, (38, 31)), O.resize_linear_exact(g, (38, 31)))
    k = np.outer([1, 4, 6, 4, 1], [1, 4, 6, 4, 1])
    p = np.pad(g.astype(np.int64), 2, mode="reflect")
    want = np.array([[((p[y:y + 5, x:x + 5] * k).sum() + 128) >> 8 for x in range(45)] for y in range(37)])
    assert np.array_equal(N.blur(g), want)
    assert p[0, 5] == g[2, 3] and p[-1, 5] == g[-3, 3]  # REFLECT_101: the edge pixel is not repeated


class _Stub:
    def __init__(self):
        self.calls = []

    def detect(self, imgs, masks=None):
        self.calls.append((imgs, masks))
        return [("features", i) for i in range(len(imgs))]


def test_feature_detector_surface_without_a_gpu(monkeypatch):
    assert list(S.FeatureDetector.DETECTOR_CHOICES) == ["orb", "sift"] and S.FeatureDetector.DEFAULT_DETECTOR == "orb"
    stub = _Stub()
    det = S.FeatureDetector("no such name", estimator=stub)  # the name is not looked at
    imgs, masks = [np.zeros((40, 50, 3), np.uint8), np.zeros((33, 35, 3), np.uint8)], [np.zeros((40, 50), np.uint8), np.zeros((33, 35), np.uint8)]
    assert det.detect(imgs) == [("features", 0), ("features", 1)] and stub.calls[-1][0][0] is imgs[0] and stub.calls[-1][1] is None
    assert det.detect_with_masks(imgs, masks) == [("features", 0), ("features", 1)] and stub.calls[-1][1][1] is masks[1]
    assert det.detect_features(imgs[1], mask=masks[1]) == ("features", 0) and stub.calls[-1][1][0] is masks[1]
    with pytest.raises(S.StitchingError, match="^image and mask lists must be of same length$"):
        det.detect_with_masks(imgs, masks[:1])
    with pytest.raises(S.StitchingError, match=r"^Resolution of mask 2 \(40, 50\) does not match the resolution of image 2 \(33, 35\)\.$"):
        det.detect_with_masks(imgs, [masks[0], masks[0]])
    monkeypatch.setitem(sys.modules, "cv2", None)  # import cv2 now fails
    with pytest.raises(S.StitchingError, match="needs OpenCV"):
        S.FeatureDetector("orb")
    with pytest.raises(S.StitchingError, match="needs OpenCV"):
        S.FeatureDetector.draw_keypoints(imgs[0], None)
    with pytest.raises(KeyError):
        S.FeatureDetector("surf")


def test_image_features_and_estimator_construction_need_no_gpu():
    with pytest.raises(S.StitchingError, match="scale above 1"):
        S.FeatureEstimator(scale=1.0)
    e = S.FeatureEstimator()
    assert (e.nfeatures, e.nlevels, e.scale, e.fast_threshold) == (500, 8, 1.2, 20)
    assert (e.MAX_SIDE, e.MAX_LEVELS, e.MAX_FEATURES) == (32767, 16, 65536)
    i32 = lambda *v: np.array(v, np.int32)  # noqa: E731
    f = S.ImageFeatures(3, (200, 150), [(200, 150), (167, 125)], i32(0, 1), i32(20, 30), i32(40, 50), i32(0, 35), np.array([7, -2], np.int64),
                        np.zeros((2, 32), np.uint8))
    k0, k1 = f.getKeypoints()
    assert len(f) == 2 and f.img_idx == 3 and f.img_size == (200, 150)
    assert (k0.pt, k0.size, k0.angle, k0.response, k0.octave) == ((20.0, 40.0), 31.0, 0.0, 7.0, 0)
    assert k1.pt == ((30 + 0.5) * 200 / 167 - 0.5, (50 + 0.5) * 150 / 125 - 0.5) and k1.size == 31.0 * 200 / 167
    assert (k1.angle, k1.response, k1.octave) == (350.0, -2.0, 1)


def main():
    """python -m tests.test_features_contract [seed]: measure the matching share and write it, with the seed, as the "matching" entry of
    profiles/features.json (the other entries are kept).  The test above then holds later changes to within a tenth of it."""
    seed = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    share, n = matching_share(seed, upright=False)
    wrong, _ = matching_share(seed, upright=True)
    doc = json.load(open(PROFILE)) if os.path.exists(PROFILE) else {}
    doc["matching"] = {"seed": seed, "share": round(share, 4), "keypoints": n, "share_with_every_bin_forced_to_0": round(wrong, 4),
                       "what": "python -m tests.test_features_contract: tests/numpy_features.py (CPU, no device involved) on a seeded 320 x 240 "
                               "texture and its copy rotated by 30 degrees and shrunk by 1 / 1.2; the share of keypoints whose Hamming-nearest "
                               "descriptor in the copy lies within 3 px of the true position"}
    with open(PROFILE, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc["matching"]))


if __name__ == "__main__":
    main()
