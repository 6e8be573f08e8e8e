"""The constructed feature inputs (tests/constructed_features.py) on the MI355X: every family through S.FeatureEstimator(...).detect
against the contract tests/numpy_features.py, all six arrays and level_sizes, 0 differing bytes.  What each family reaches, and that it
tells the contract from a one-mistake variant of it, is asserted without a GPU in tests/test_constructed_features.py; here only the
device is asked.  The contract's result of an input is computed once and shared (test_gpu_features._ref)."""
import numpy as np
import pytest

import stitching_amd as S
from tests import constructed_features as CF
from tests import numpy_features as N
from tests.test_gpu_constructed_inputs import _pitched
from tests.test_gpu_features import ARRAYS, _check, _ref, _same

pytestmark = pytest.mark.gpu

SELECTION_IDS = ("255", "256", "257", "511", "512", "513", "count-1", "count", "count+1")  # of CF.selection_sizes(count)
MASK_KW = dict(nlevels=3, nfeatures=2000)
BATCH_KW = dict(nfeatures=300, fast_threshold=10)


def _places(f):
    return list(zip(f.x.tolist(), f.y.tolist()))


def _views(key, ctx, img, mask=None, **kw):
    """detect on `img` (and `mask`) as views into larger device buffers: the contract's result, and views and surroundings unchanged"""
    views = [_pitched(img, ctx, 200)] + ([] if mask is None else [_pitched(mask, ctx, 255)])
    got = S.FeatureEstimator(**kw).detect([views[0][0]], None if mask is None else [views[1][0]])
    _same(got[0], _ref(key, img, mask, **kw))
    for _, check in views:
        check()
    return got[0]


def test_response_between_2_31_and_2_32(gpu_ctx):
    img, facts = CF.high_response()
    f = _check(("cf", "high_response"), img, nlevels=1)
    assert _places(f) == [facts["keypoint"]] and f.R.tolist() == [CF.PATCH_R] and 2 ** 31 <= CF.PATCH_R < 2 ** 32


@pytest.mark.parametrize("nfeatures", (1, 2, 3))
def test_negative_responses_rank_behind_every_other(gpu_ctx, nfeatures):
    img, facts = CF.negative_response()
    f = _check(("cf", "negative_response", nfeatures), img, nlevels=1, nfeatures=nfeatures)
    assert _places(f) == ([facts["positive"]] + facts["negatives"])[:nfeatures]
    assert all((r > 0) == (k == 0) for k, r in enumerate(f.R.tolist()))


@pytest.mark.parametrize("size", CF.TILED_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_tiled_copies(gpu_ctx, size):
    """coordinates up to 403 in the key, 13 score tiles and 7 blur tiles in a row, copies on the first and last column and row of a tile"""
    img, facts = CF.tiled(*size)
    f = _check(("cf", "tiled", size, 2000), img, nlevels=1, nfeatures=2000)
    # metamorphic, on the device's result: the copies differ in nothing but their place
    assert _places(f) == facts["keypoints"] and set(f.R.tolist()) == {CF.PATCH_R} and len(set(f.bin.tolist())) == 1
    assert len(f) > 1 and np.all(f.descriptors == f.descriptors[0])
    for n in (37, 5):  # a cut inside a run of equal R: the first by (y, x) stay
        assert _places(_check(("cf", "tiled", size, n), img, nlevels=1, nfeatures=n)) == facts["keypoints"][:n]


@pytest.mark.parametrize("size", CF.TILED_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_tiled_copies_as_pitched_views(gpu_ctx, size):
    img, facts = CF.tiled(*size)
    assert _places(_views(("cf", "tiled", size, 2000), gpu_ctx, img, nlevels=1, nfeatures=2000)) == facts["keypoints"]


def test_plateau_across_score_tile_borders(gpu_ctx):
    img, facts = CF.plateau()
    assert _places(_check(("cf", "plateau"), img, nlevels=1)) == [facts["dot"]]


def test_orientation_ties_go_to_the_smaller_bin(gpu_ctx):
    img, facts = CF.orientation_ties()
    f = _check(("cf", "orientation_ties"), img, nlevels=1)
    bins = dict(zip(_places(f), f.bin.tolist()))
    assert {kind: bins[p] for kind, p in facts["keypoints"].items()} == {kind: facts["bins"][kind][0] for kind in CF.TIE_KINDS}


@pytest.mark.parametrize("k", range(9), ids=SELECTION_IDS)
def test_selection_sizes(gpu_ctx, k):
    """the chunk edges of the survivor and ranking loops of feat_select, and both sides of `count > keep`"""
    img, facts = CF.selection_level()
    count = len(_ref(("cf", "selection", "all"), img, None, nlevels=1, nfeatures=60000, fast_threshold=facts["threshold"])["x"])
    assert count > facts["at_least"]
    n = CF.selection_sizes(count)[k]
    f = _check(("cf", "selection", n), img, nlevels=1, nfeatures=n, fast_threshold=facts["threshold"])
    assert len(f) == min(n, count)


@pytest.mark.parametrize("pick", (0, 1), ids=("level2", "level0_x256"))
def test_single_pixel_masks(gpu_ctx, pick):
    img, _ = CF.tiled()
    size = (img.shape[1], img.shape[0])
    free = _ref(("cf", "mask", None), img, None, **MASK_KW)
    picks = CF.pick_mask_keypoints(free, size)
    k, other = picks[pick], picks[1 - pick]
    pixel = CF.mask_pixel(int(free["x"][k]), int(free["y"][k]), free["level_sizes"][free["level"][k]], size)
    one_at = CF.mask_pixel(int(free["x"][other]), int(free["y"][other]), free["level_sizes"][free["level"][other]], size)
    only, rest = CF.single_pixel_masks(size, pixel, one_at)
    before = only.copy(), rest.copy()
    f = _check(("cf", "mask", pick, "only"), img, only, **MASK_KW)
    assert (f.level.tolist(), _places(f)) == ([int(free["level"][k])], [(int(free["x"][k]), int(free["y"][k]))])
    assert len(_check(("cf", "mask", pick, "rest"), img, rest, **MASK_KW)) == len(free["x"]) - 1
    assert np.array_equal(only, before[0]) and np.array_equal(rest, before[1])
    if pick == 1:  # once with image and mask as pitched views
        assert len(_views(("cf", "mask", pick, "only"), gpu_ctx, img, only, **MASK_KW)) == 1


@pytest.mark.parametrize("scale,nlevels", CF.SCALES)
def test_scales(gpu_ctx, scale, nlevels):
    img, _ = CF.selection_level()
    f = _check(("cf", "scale", scale), img, scale=scale, nlevels=nlevels, fast_threshold=10)
    assert f.level_sizes == N.level_sizes(200, 150, nlevels, scale) and len(f.level_sizes) == {1.05: 16, 1.5: 4, 2.0: 3}[scale]
    assert set(f.level.tolist()) == set(range(len(f.level_sizes)))


def test_batch_of_24_equals_single_calls(gpu_ctx):
    """more than 32 level descriptors under the tile bisection; the first and the last image have no level; one image is listed twice"""
    imgs, facts = CF.batch()
    before = [a.copy() for a in imgs]
    est = S.FeatureEstimator(**BATCH_KW)
    got = est.detect(imgs)
    assert [f.img_idx for f in got] == list(range(24)) and all(np.array_equal(a, b) for a, b in zip(imgs, before))
    assert est.info["levels"] == sum(len(f.level_sizes) for f in got) > 32 and est.info["keypoints"] == sum(len(f) for f in got)
    for i, (img, f) in enumerate(zip(imgs, got)):
        _same(f, _ref(("cf", "batch", facts["twice"][0] if i == facts["twice"][1] else i), img, None, **BATCH_KW))
        assert (len(f.level_sizes) == 0) == (i in facts["no_level"]) and len(f) <= 300 * bool(f.level_sizes)
        one = S.FeatureEstimator(**BATCH_KW).detect([img])[0]
        for name, _ in ARRAYS:
            assert np.array_equal(getattr(one, name), getattr(f, name)), (i, name)
    a, b = (got[i] for i in facts["twice"])
    assert all(np.array_equal(getattr(a, name), getattr(b, name)) for name, _ in ARRAYS) and len(a) > 0


def test_batch_without_any_level(gpu_ctx):
    imgs, _ = CF.too_small_batch()
    est = S.FeatureEstimator()
    got = est.detect(imgs)
    assert len(got) == len(imgs) and est.info == {"levels": 0, "candidates": 0, "keypoints": 0}
    for i, (img, f) in enumerate(zip(imgs, got)):
        _same(f, _ref(("cf", "small", i), img, None))
        assert len(f) == 0 and f.level_sizes == [] and f.img_idx == i and f.img_size == (img.shape[1], img.shape[0])
