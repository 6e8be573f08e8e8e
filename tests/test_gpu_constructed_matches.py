"""The constructed matcher families (tests/constructed_matches.py) on the MI355X: the same inputs through S.MatchEstimator for the
models each family names, against the contracts (tests/numpy_matches.py, tests/numpy_affine.py) exactly as tests/test_gpu_matches.py
compares — every integer array and the float64 bits of H_sample equal, H and confidence at the project's rtol = 1e-9 — and the
families' facts once more on the device's own output.  The inputs are read back unchanged.  Families whose path is in match_2nn also run
with STX_MATCH_TRAIN=uniform.  What each family reaches, that its facts hold, and that it tells the contract from a subtly wrong variant is
asserted without a GPU in tests/test_constructed_matches.py; here only the device is asked."""
import numpy as np
import pytest

import stitching_amd as S
from tests import affine_rigs as AR
from tests import constructed_matches as CM
from tests.test_gpu_matches import _same

pytestmark = pytest.mark.gpu


def _run(model, name, *args):
    """the device on a case under `model` against the contract's result of it (computed once) -> case, the device's entries"""
    case = CM.built(name, *args)
    F = AR.package_features(case.features)
    before = [(f.descriptors.copy(), f.x.copy(), f.y.copy(), f.level.copy()) for f in F]
    est = S.MatchEstimator(model="homography" if model == "homography" else "affine", full_affine=model == "affine_full", **case.kw)
    assert est.model == model
    got = est.match(F)
    _same(got, CM.contract(model, name, *args))
    for f, c, (d, x, y, l) in zip(F, case.features, before):
        assert np.array_equal(f.descriptors, d) and np.array_equal(f.x, x) and np.array_equal(f.y, y) and np.array_equal(f.level, l)
        assert np.array_equal(f.descriptors, c["descriptors"]) and np.array_equal(f.x, c["x"]) and np.array_equal(f.y, c["y"])
    n = len(F)
    assert est.info["pairs"] == sum(1 for e in got if 0 <= e.src_img_idx < e.dst_img_idx)
    assert est.info["matches"] == sum(len(got[i * n + j].matches) for i in range(n) for j in range(i + 1, n))
    return case, got


@pytest.mark.parametrize("train", ("lds", "uniform"))
def test_tiles(train, monkeypatch):
    if train == "uniform":
        monkeypatch.setenv("STX_MATCH_TRAIN", "uniform")
    case, got = _run("homography", "tiles")
    CM.assert_rows(case, got)


@pytest.mark.parametrize("train", ("lds", "uniform"))
@pytest.mark.parametrize("conf", CM.RATIO_CONFS)
def test_ratio_edges(conf, train, monkeypatch):
    if train == "uniform":
        monkeypatch.setenv("STX_MATCH_TRAIN", "uniform")
    case, got = _run("homography", "ratio_edges", conf)
    CM.assert_rows(case, got)


@pytest.mark.parametrize("which", CM.PLACEMENTS)
def test_placements(which):
    case, got = _run("homography", "placements", which)
    CM.assert_rows(case, got)
    assert len(got[1].matches) == len(case.facts["rows"][(0, 1)])
    if which == "none":
        assert set(case.facts["kept_same_t"]) <= {tuple(r) for r in got[1].matches.tolist()}


def test_pair_shapes():
    case, got = _run("homography", "pair_shapes")
    CM.assert_rows(case, got)
    assert len(got[1 * 4 + 2].matches) == 0 and got[1 * 4 + 2].src_img_idx == 1


@pytest.mark.parametrize("threshold", (3.0, 0.0))
@pytest.mark.parametrize("model", CM.MODELS)
def test_threshold(model, threshold):
    case, got = _run(model, "threshold", model, threshold)
    CM.assert_rows(case, got)
    CM.assert_winner(case, got, exact_k=False)


@pytest.mark.parametrize("iters", CM.TIES_ITERS)
@pytest.mark.parametrize("model", CM.MODELS)
def test_hypothesis_ties(model, iters):
    case, got = _run(model, "hypothesis_ties", model, iters)
    CM.assert_rows(case, got)
    CM.assert_winner(case, got, exact_k=True)


def test_many_pairs():
    case, got = _run("homography", "many_pairs")
    CM.assert_many(case, got)


@pytest.mark.parametrize("seed", CM.SEEDS)
@pytest.mark.parametrize("model", CM.MODELS)
def test_seeds(model, seed):
    case, got = _run(model, "seeds", model, seed)
    CM.assert_rows(case, got)
    CM.assert_winner(case, got, exact_k=True)
