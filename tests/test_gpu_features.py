"""The project's own corner detector and binary descriptor on the MI355X (stitching_amd.FeatureEstimator, csrc/stx_features.hip) against
its contract tests/numpy_features.py, byte for byte, every array: sizes from the smallest legal level and around the wavefront and tile
edges, inputs where ties are common, selection that cuts among ties, masks, batches of unequal sizes, residency, determinism, the limits
and the FeatureDetector wrapper.  The contract's result of an input is computed once and shared."""
import numpy as np
import pytest

import stitching_amd as S
from tests import numpy_features as N

pytestmark = pytest.mark.gpu

ARRAYS = (("level", np.int32), ("x", np.int32), ("y", np.int32), ("bin", np.int32), ("R", np.int64), ("descriptors", np.uint8))
# (w, h): one legal position; one legal column / row; every width and height around the wavefront (64), the score tile (32 + 32 of
# border) and the blur tile; several levels with a dropped tail
SIZES = ((33, 33), (33, 50), (50, 33), (63, 129), (64, 128), (65, 127), (127, 65), (128, 64), (129, 63), (200, 150))
KINDS = ("noise", "three", "dot", "checker", "flat")


def _smooth(a):
    """light smoothing: the mean of a pixel and its right / lower neighbours (wrapping)"""
    a = a.astype(np.uint16)
    return ((a + np.roll(a, 1, 0) + np.roll(a, 1, 1) + np.roll(a, (1, 1), (0, 1)) + 2) // 4).astype(np.uint8)


def _image(kind, w, h, seed=0):
    rs = np.random.RandomState(1000 + seed)
    if kind == "noise":
        return _smooth(rs.randint(0, 256, (h, w, 3)))
    if kind == "three":  # 3 grey values in cells of 3 x 3: equal scores and equal responses (R = 0 on flat windows) are common
        cells = rs.randint(0, 3, ((h + 2) // 3, (w + 2) // 3))
        g = np.array([40, 120, 220], np.uint8)[np.kron(cells, np.ones((3, 3), np.int64))[:h, :w]]
        return np.repeat(g[:, :, None], 3, axis=2)
    if kind == "dot":
        a = np.zeros((h, w, 3), np.uint8)
        a[h // 2, w // 2] = 255
        return a
    if kind == "checker":
        yy, xx = np.mgrid[0:h, 0:w]
        return np.repeat((((yy // 8 + xx // 8) % 2) * 200 + 20).astype(np.uint8)[:, :, None], 3, axis=2)
    return np.full((h, w, 3), 100, np.uint8)


_REFS = {}


def _ref(key, img, mask=None, **kw):
    """the contract's result for a named input, computed once"""
    if key not in _REFS:
        _REFS[key] = N.detect(img, mask, **kw)
    return _REFS[key]


def _same(got, want):
    for name, dtype in ARRAYS:
        g = getattr(got, name)
        assert isinstance(g, np.ndarray) and g.dtype == dtype and g.shape == want[name].shape, (name, g.dtype, g.shape, want[name].shape)
        assert np.array_equal(g, want[name]), (name, int(np.count_nonzero(g != want[name])))
    assert got.level_sizes == want["level_sizes"]


def _check(key, img, mask=None, **kw):
    before = img.copy()
    got = S.FeatureEstimator(**kw).detect([img], None if mask is None else [mask])
    assert len(got) == 1 and got[0].img_idx == 0 and got[0].img_size == (img.shape[1], img.shape[0])
    want = _ref(key, img, mask, **kw)
    _same(got[0], want)
    assert np.array_equal(img, before)
    return got[0]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_sizes(gpu_ctx, size):
    w, h = size
    f = _check(("noise", size), _image("noise", w, h), fast_threshold=5, nfeatures=4000)
    if size == (200, 150):
        assert len(f.level_sizes) == 8 and len(set(f.level.tolist())) >= 4 and len(f) > 100
        assert len(_check(("noise", size, 12), _image("noise", w, h), nlevels=12).level_sizes) == 9  # 150 / 1.2**9 = 29.07 < 33: levels 9 .. 11 are dropped


def test_one_legal_position(gpu_ctx):
    f = _check(("dot", 33), _image("dot", 33, 33))
    assert (f.x.tolist(), f.y.tolist(), f.level.tolist()) == ([16], [16], [0])
    assert len(_check(("dot", 33, "off"), np.roll(_image("dot", 33, 33), 1, axis=1))) == 0  # one pixel beside it: outside the border


@pytest.mark.parametrize("kind", KINDS)
def test_inputs(gpu_ctx, kind):
    f = _check((kind, 131, 97), _image(kind, 131, 97), fast_threshold=10)
    assert (len(f) == 0) == (kind == "flat")
    if kind == "three":
        assert len(_check((kind, 200, 150), _image(kind, 200, 150), nfeatures=3000, fast_threshold=10)) > 200


@pytest.mark.parametrize("kind", ("noise", "three"))
@pytest.mark.parametrize("nfeatures", (1, 5, 60000))
def test_selection_counts(gpu_ctx, kind, nfeatures):
    """1 and 5 cut among ties (three grey values); 60000 is above every candidate count"""
    f = _check((kind, "n", nfeatures), _image(kind, 200, 150), nfeatures=nfeatures, fast_threshold=10)
    assert 0 < len(f) <= nfeatures


@pytest.mark.parametrize("nlevels", (1, 8))
@pytest.mark.parametrize("threshold", (0, 254))
def test_levels_and_thresholds(gpu_ctx, nlevels, threshold):
    f = _check(("noise", "lt", nlevels, threshold), _image("noise", 200, 150), nlevels=nlevels, fast_threshold=threshold, nfeatures=60000)
    assert (len(f) > 1000 // (9 - nlevels)) if threshold == 0 else len(f) == 0
    d = _check(("dot", "lt", nlevels, threshold), _image("dot", 90, 70), nlevels=nlevels, fast_threshold=threshold)
    assert len(d) >= 1  # a score of 255 passes a threshold of 254


@pytest.mark.parametrize("kind", ("random", "zero", "quadrant"))
def test_masks(gpu_ctx, kind):
    w, h = 200, 150
    rs = np.random.RandomState(5)
    mask = {"random": (rs.rand(h, w) < 0.5) * rs.choice([255, 1, 7], (h, w)), "zero": np.zeros((h, w)),
            "quadrant": np.pad(np.full((h // 2, w // 2), 255), ((0, h - h // 2), (w - w // 2, 0)))}[kind].astype(np.uint8)
    before = mask.copy()
    f = _check(("noise", "mask", kind), _image("noise", w, h), mask, fast_threshold=5, nfeatures=2000)
    assert np.array_equal(mask, before)
    free = _ref(("noise", "mask", None), _image("noise", w, h), None, fast_threshold=5, nfeatures=2000)
    assert (len(f) == 0) if kind == "zero" else (0 < len(f) < len(free["x"]))
    if kind == "quadrant":
        kp = f.getKeypoints()
        assert all(k.pt[0] > w // 2 - 1 and k.pt[1] < h // 2 for k in kp)


BATCH = (("noise", 200, 150), ("three", 97, 131), ("checker", 64, 33), ("noise", 32, 80), ("dot", 129, 129))


def test_batch_equals_single_calls(gpu_ctx):
    """5 images of unequal sizes (one too small for any level), masks on some of them"""
    imgs = [_image(k, w, h, seed=i) for i, (k, w, h) in enumerate(BATCH)]
    rs = np.random.RandomState(9)
    masks = [None, (rs.rand(131, 97) < 0.7).astype(np.uint8) * 255, None, np.full((80, 32), 255, np.uint8), None]
    est = S.FeatureEstimator(nfeatures=300, fast_threshold=10)
    got = est.detect(imgs, masks)
    assert [f.img_idx for f in got] == list(range(5)) and len(got[3]) == 0 and got[3].level_sizes == []
    assert est.info["keypoints"] == sum(len(f) for f in got) and est.info["candidates"] >= est.info["keypoints"]
    for i, (img, mask) in enumerate(zip(imgs, masks)):
        _same(got[i], _ref(("batch", i), img, mask, nfeatures=300, fast_threshold=10))
        one = S.FeatureEstimator(nfeatures=300, fast_threshold=10).detect([img], [mask])[0]
        for name, _ in ARRAYS:
            assert np.array_equal(getattr(one, name), getattr(got[i], name)), (i, name)


def test_device_images_stay_and_are_unchanged(gpu_ctx):
    img, mask = _image("noise", 200, 150), (np.random.RandomState(3).rand(150, 200) < 0.6).astype(np.uint8) * 255
    d_img, d_mask = S.DeviceImage.from_numpy(img, gpu_ctx), S.DeviceImage.from_numpy(mask, gpu_ctx)
    got = S.FeatureEstimator().detect([d_img, d_img[:100, :120]], [d_mask, None])
    _same(got[0], _ref(("resident", 0), img, mask))
    _same(got[1], _ref(("resident", 1), np.ascontiguousarray(img[:100, :120]), None))  # a view: pitched rows
    assert np.array_equal(d_img.numpy(), img) and np.array_equal(d_mask.numpy(), mask)


def test_two_runs_return_identical_bytes(gpu_ctx):
    imgs = [_image("three", 200, 150), _image("noise", 129, 63, seed=4)]
    est = S.FeatureEstimator(nfeatures=40, fast_threshold=0)
    a, b = est.detect(imgs), est.detect(imgs)
    for fa, fb in zip(a, b):
        assert len(fa) > 0
        for name, _ in ARRAYS:
            assert getattr(fa, name).tobytes() == getattr(fb, name).tobytes(), name


def test_limits_are_refused(gpu_ctx):
    ok = _image("noise", 40, 40)
    with pytest.raises(S.StitchingError, match="sides up to 32767"):
        S.FeatureEstimator().detect([np.zeros((33, 32768, 3), np.uint8)])
    with pytest.raises(S.StitchingError, match="17 levels: 1 .. 16"):
        S.FeatureEstimator(nlevels=17).detect([ok])
    with pytest.raises(S.StitchingError, match="65537 features per image: 1 .. 65536"):
        S.FeatureEstimator(nfeatures=65537).detect([ok])
    with pytest.raises(S.StitchingError, match=r"Resolution of mask 2 \(10, 12\) does not match the resolution of image 2 \(40, 40\)\."):
        S.FeatureEstimator().detect([ok, ok], [None, np.zeros((10, 12), np.uint8)])
    with pytest.raises(S.StitchingError, match="needs u8x3 images"):
        S.FeatureEstimator().detect([ok[:, :, 0].copy()])
    with pytest.raises(S.StitchingError, match="needs u8x3 images"):
        S.FeatureEstimator().detect([ok.astype(np.float32)])
    with pytest.raises(S.StitchingError, match="same length"):
        S.FeatureEstimator().detect([ok], [None, None])


def test_feature_detector_wrapper(gpu_ctx):
    imgs = [_image("noise", 200, 150), _image("checker", 97, 131)]
    masks = [np.full((150, 200), 255, np.uint8), np.pad(np.full((60, 97), 9, np.uint8), ((0, 71), (0, 0)))]
    det = S.FeatureDetector(estimator=S.FeatureEstimator())
    assert S.FeatureDetector.DEFAULT_DETECTOR == "orb" and list(S.FeatureDetector.DETECTOR_CHOICES) == ["orb", "sift"]
    got, direct = det.detect_with_masks(imgs, masks), S.FeatureEstimator().detect(imgs, masks)
    plain, one = det.detect(imgs), det.detect_features(imgs[1], mask=masks[1])
    for i in range(2):
        _same(got[i], _ref(("wrapper", i), imgs[i], masks[i]))
        for name, _ in ARRAYS:
            assert np.array_equal(getattr(got[i], name), getattr(direct[i], name))
    _same(plain[0], _ref(("wrapper", 0), imgs[0], masks[0]))  # a mask of 255 everywhere changes nothing
    _same(one, _ref(("wrapper", 1), imgs[1], masks[1]))
    kp = got[0].getKeypoints()
    k = int(np.argmax(got[0].level))
    (w0, h0), (wl, hl) = got[0].img_size, got[0].level_sizes[got[0].level[k]]
    assert kp[k].pt == ((got[0].x[k] + 0.5) * w0 / wl - 0.5, (got[0].y[k] + 0.5) * h0 / hl - 0.5) and kp[k].size == 31.0 * w0 / wl
    assert kp[k].angle == 10.0 * got[0].bin[k] and kp[k].response == float(got[0].R[k]) and kp[k].octave == got[0].level[k] > 0
    with pytest.raises(S.StitchingError, match="image and mask lists must be of same length"):
        det.detect_with_masks(imgs, masks[:1])
    with pytest.raises(S.StitchingError, match=r"Resolution of mask 2 \(150, 200\) does not match the resolution of image 2 \(131, 97\)\."):
        det.detect_with_masks(imgs, [masks[0], masks[0]])
