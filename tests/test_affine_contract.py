"""tests/numpy_affine.py is a registration and not just a definition: its closed forms fit what numpy's solver fits, its RANSAC finds a
planted similarity and a planted affine map through 30 % outliers, and on grids of tiles with known transforms it recovers them within
twice the error recorded in profiles/affine.json (tools/bench_affine.py --contract-only wrote it from this very code; the rigs are
seeded, so the margin covers another LAPACK only).  Also its rules one by one, the host-side pieces of the package that need no GPU
against it, the wrappers' acceptance and refusals and AffineComposer's settings.  The device is compared with the contract in
tests/test_gpu_affine_matches.py, test_gpu_affine_cameras.py and test_gpu_affine_stitch.py."""
import math
import warnings

import numpy as np
import pytest

import stitching_amd as S
from stitching_amd import camera_estimation as CE
from stitching_amd import match_estimation as ME
from tests import affine_rigs as AR
from tests import camera_rigs as CR
from tests import numpy_affine as NA
from tests import numpy_cameras as NC
from tests import numpy_matches as NM


# ---- the hypothesis ------------------------------------------------------------------------------------------------------------------------
def _apply(h, p):
    q = h.reshape(3, 3) @ np.array([p[0], p[1], 1.0])
    return q[:2] / q[2]


def test_closed_forms_against_a_linear_solve():
    """both closed forms against np.linalg.solve of the same sample, for samples of both orientations; and they take the sample's own
    points onto their partners"""
    rs = np.random.RandomState(1)
    seen = set()
    for _ in range(200):
        src, dst = rs.uniform(0, 640, (3, 2)), rs.uniform(0, 640, (3, 2))
        # full: 6 unknowns, 6 equations
        A = np.zeros((6, 6))
        for k in range(3):
            A[2 * k, 0:3] = A[2 * k + 1, 3:6] = [src[k, 0], src[k, 1], 1.0]
        want = np.linalg.solve(A, dst.reshape(6))
        h = NA.closed_form_full(src, dst)
        seen.add(bool(h[8] < 0))
        assert h[6] == 0 and h[7] == 0 and not np.signbit(h[6:8]).any()
        assert np.allclose(h[:6] / h[8], want, rtol=1e-9, atol=1e-9 * np.abs(want).max())
        det = np.linalg.det(np.array([[src[0, 0], src[1, 0], src[2, 0]], [src[0, 1], src[1, 1], src[2, 1]], [1.0, 1.0, 1.0]]))
        assert h[8] == pytest.approx(det, rel=1e-9)
        # partial: 4 unknowns a, b, tx, ty, 4 equations
        A = np.array([[src[0, 0], -src[0, 1], 1, 0], [src[0, 1], src[0, 0], 0, 1], [src[1, 0], -src[1, 1], 1, 0], [src[1, 1], src[1, 0], 0, 1]])
        a, b, tx, ty = np.linalg.solve(A, dst[:2].reshape(4))
        h = NA.closed_form_partial(src[:2], dst[:2])
        assert h[8] > 0 and h[0] == h[4] and h[1] == -h[3] and h[6] == 0 and h[7] == 0
        assert np.allclose(h[:6] / h[8], [a, -b, tx, b, a, ty], rtol=1e-9, atol=1e-9 * max(abs(tx), abs(ty)))
        for k in range(2):
            assert np.allclose(_apply(h, src[k]), dst[k], atol=1e-8)
    assert seen == {True, False}  # clockwise and counter-clockwise samples


def test_planted_maps_are_reproduced():
    """a planted similarity to 4e-14 and a planted affine map to 1e-12 of the largest entry, for both orientations of the sample"""
    rs = np.random.RandomState(2)
    for _ in range(100):
        src = rs.uniform(0, 640, (3, 2))
        for order in ([0, 1, 2], [0, 2, 1]):
            s = src[order]
            hom = np.concatenate([s, np.ones((3, 1))], axis=1)
            xyuv = np.concatenate([s, (hom @ AR.AFFINE.T)[:, :2]], axis=1)
            h, ok = NA.hypothesis(xyuv, [0, 1, 2], "affine_full")
            assert ok and h[8] > 0 and np.abs(h.reshape(3, 3) / h[8] - AR.AFFINE).max() <= 1e-12 * np.abs(AR.AFFINE).max()
            xyuv = np.concatenate([s, (hom @ AR.SIMILARITY.T)[:, :2]], axis=1)
            h, ok = NA.hypothesis(xyuv, [0, 1], "affine_partial")
            assert ok and np.abs(h.reshape(3, 3) / h[8] - AR.SIMILARITY).max() <= 4e-14 * np.abs(AR.SIMILARITY).max()


def test_sign_rule_and_degenerate_samples():
    """a clockwise sample of the full model is negated to h8 > 0 and then fits as its mirror does; coincident points (both models) and
    collinear points (full) give h8 == 0 and no inliers"""
    pts = np.array([[10.0, 10.0], [200.0, 30.0], [50.0, 300.0], [120.0, 140.0]])
    xyuv = np.concatenate([pts, (np.concatenate([pts, np.ones((4, 1))], axis=1) @ AR.AFFINE.T)[:, :2]], axis=1)
    raw = NA.closed_form_full(xyuv[[0, 2, 1], 0:2], xyuv[[0, 2, 1], 2:4])
    assert raw[8] < 0
    h, ok = NA.hypothesis(xyuv, [0, 2, 1], "affine_full")
    assert ok and h[8] == -raw[8] and np.array_equal(h[:6], -raw[:6]) and not np.signbit(h[6:8]).any()
    assert NM.inliers(h, xyuv, np.float64(1e-6)).all() and not NM.inliers(raw, xyuv, np.float64(9.0)).any()  # W < 0 without the rule
    same = np.tile(np.array([[77.0, 55.0, 80.0, 59.0]]), (8, 1))
    for model, idx in (("affine_partial", [0, 1]), ("affine_full", [0, 1, 2])):
        h, ok = NA.hypothesis(same, idx, model)
        assert not ok and h[8] == 0
        k, hs, mask = NA.ransac(same, 1, 16, 3.0, 0x5EED, model)
        assert k == 0 and not mask.any() and hs[8] == 0
    t = np.arange(8.0)
    line = np.stack([100 + 10 * t, 50 + 5 * t, 103 + 10 * t, 54 + 5 * t], axis=1)
    h, ok = NA.hypothesis(line, [0, 3, 6], "affine_full")
    assert not ok and h[8] == 0
    assert not NA.ransac(line, 1, 32, 3.0, 0x5EED, "affine_full")[2].any()
    assert NA.ransac(line, 1, 32, 3.0, 0x5EED, "affine_partial")[2].all()  # two points of a line do fix a similarity


def test_sampler_draws_distinct_indices():
    for s in (2, 3):
        for m in (6, 7, 64, 1000):
            for k in range(300):
                idx = NA.sample(0x5EED, 5, k, m, s)
                assert len(idx) == s == len(set(idx)) and all(0 <= i < m for i in idx)
                assert idx == NM.sample(0x5EED, 5, k, m)[:s]  # the homography's sampler, cut short
    # every index is drawn: m = 6, many hypotheses
    assert {i for k in range(200) for i in NA.sample(1, 1, k, 6, 2)} == set(range(6))


@pytest.mark.parametrize("model,A", [("affine_partial", AR.SIMILARITY), ("affine_full", AR.AFFINE)])
def test_contract_finds_a_planted_map_through_outliers(model, A):
    """300 matches, 30 % of them wrong, two pyramid levels (positions quantised to 2 px at level 1): at least 60 % inliers, the linear
    part within 0.01, the translation within 1 px"""
    feats = AR.planted_pair(310, 300, A)
    e = NA.match(feats, model=model, ransac_iters=200)[1]
    assert len(e["matches"]) == 300 and e["num_inliers"] >= 180 and e["confidence"] > 1
    assert np.array_equal(e["H"][2], [0.0, 0.0, 1.0])
    assert np.abs(e["H"][:2, :2] - A[:2, :2]).max() < 0.01 and np.abs(e["H"][:2, 2] - A[:2, 2]).max() < 1.0
    if model == "affine_partial":
        assert e["H"][0, 0] == e["H"][1, 1] and e["H"][0, 1] == -e["H"][1, 0]
    back = NA.match(feats, model=model, ransac_iters=200)[2]
    assert np.allclose(back["H"] @ e["H"], np.eye(3), atol=1e-9)
    # the similarity model cannot fit the sheared map as well as the full model does
    if model == "affine_full":
        assert NA.match(feats, model="affine_partial", ransac_iters=200)[1]["num_inliers"] < e["num_inliers"]


def test_refits():
    rs = np.random.RandomState(3)
    src = rs.uniform(0, 640, (40, 2))
    hom = np.concatenate([src, np.ones((40, 1))], axis=1)
    for A, full in ((AR.SIMILARITY, False), (AR.AFFINE, True), (AR.SIMILARITY, True)):
        dst = (hom @ A.T)[:, :2]
        for fn in (lambda s, d: NA.refit(s, d, "affine_full" if full else "affine_partial"), lambda s, d: ME.refit_affine(s, d, full)):
            h = fn(src, dst)
            assert np.allclose(h, A, rtol=0, atol=1e-9) and np.array_equal(h[2], [0.0, 0.0, 1.0])
        noisy = dst + rs.normal(0, 0.5, dst.shape)
        assert np.allclose(ME.refit_affine(src, noisy, full), NA.refit(src, noisy, "affine_full" if full else "affine_partial"), rtol=1e-12, atol=1e-12)
    with np.errstate(all="ignore"):
        flat = NA.refit_partial(np.full((8, 2), 5.0), np.full((8, 2), 9.0))
    assert NM.inverse(flat) is None  # every match on one point: no H


# ---- the sum, the Jacobian ---------------------------------------------------------------------------------------------------------------
def test_ordered_sum_of_the_terms_against_fsum():
    """|ordered - exact| <= 2^-40 sum |term| on the affine terms of real edges (tests/test_cameras_contract.py has the argument)"""
    feats, matches, _ = AR.rig("grid3x2")
    p = NA.start_parameters(NA.estimate(feats, matches))
    V = NA.variants(p)
    pts = [NA.uncentred(f) for f in feats]
    for i, j in NC.edges(matches, 6):
        terms = NA.match_terms(V[i], V[j], NC.edge_points(feats, matches, 6, i, j, pts))
        assert terms.shape[1] == 45 and len(terms) >= 8
        got = NC.ordered_sum(terms)
        for a in range(45):
            assert abs(got[a] - math.fsum(terms[:, a])) <= 2.0 ** -40 * math.fsum(np.abs(terms[:, a])), (i, j, a)


def test_gradient_against_finite_differences():
    """2 g is the gradient of E: against central differences of E over the assembled system with a step of 1e-4.  The residual is
    linear in the moving camera's parameters and a rational function of the other's: truncation of either difference at most h^2 / 6
    relative (2e-7), rounding of E (1e3 * 2^-52 / 1e-4 = 2e-9 absolute) — bound 1e-5 of the largest gradient entry, as for the rays."""
    feats, matches, _ = AR.rig("grid2x2")
    p = NA.start_parameters(NA.estimate(feats, matches))
    p = p + np.random.RandomState(4).uniform(-1, 1, p.shape) * (0.01, 0.01, 2.0, 2.0)
    ed = NC.edges(matches, 4)
    total = lambda q: NC.assemble(4, ed, *NA.normal_equations(feats, matches, q))  # noqa: E731
    E, g, A = total(p)
    fd = np.zeros(16)
    for k in range(16):
        step = np.zeros(16)
        step[k] = 1e-4
        fd[k] = (total(p + step.reshape(4, 4))[0] - total(p - step.reshape(4, 4))[0]) / 2e-4
    worst = np.abs(2 * g - fd).max() / np.abs(fd).max()
    print(f"gradient 2 g against finite differences of E: {worst:.3g} of the largest entry; E = {E:.1f}")
    assert worst < 1e-5
    assert np.array_equal(A, A.T) and (np.linalg.eigvalsh(A) > -1e-6 * np.abs(A).max()).all()  # J^T J


# ---- the rigs ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", AR.CASES)
def test_contract_recovers_the_planted_tiles(name):
    """the largest corner error relative to the centre tile within twice what profiles/affine.json records for this rig"""
    (idx, cams, info), rec = AR.measure(name)
    bound = 2.0 * AR.recorded(name)
    print(f"{name}: {rec} (bound: {bound})")
    assert idx == list(range(rec["tiles"]))
    assert 0 < rec["corner_error_px"] <= bound
    assert info["accepted"] >= 1 and info["last_E"] < info["first_E"] and info["evaluations"] <= 100
    assert rec["rms_px"] < 1.5  # the noise: 0.5 px and the rounding to pixels, in both images
    assert all(c["R"].dtype == np.float32 and (c["focal"], c["aspect"], c["ppx"], c["ppy"]) == (1.0, 1.0, 0.0, 0.0) for c in cams)
    _, centre = NC.spanning_tree(NC.subset_matches(AR.rig(name)[1] if name != "texture" else AR.texture_case()[1], idx), len(idx))
    assert np.allclose(cams[centre]["R"], np.eye(3), atol=1e-6)


def test_estimate_and_failures():
    feats, matches, _ = AR.rig("row5")
    _, centre = NC.spanning_tree(matches, 5)
    T = NA.transforms(matches, 5)
    assert centre == 2 and np.array_equal(T[2], np.eye(3))
    assert np.allclose(T[1], matches[1 * 5 + 2]["H"]) and np.allclose(T[0], matches[1 * 5 + 2]["H"] @ matches[0 * 5 + 1]["H"])
    assert np.allclose(T[3], np.linalg.inv(matches[2 * 5 + 3]["H"]))
    cut = [dict(e) for e in matches]
    for k in (2 * 5 + 3, 3 * 5 + 2):
        cut[k] = NM.empty()
    with pytest.raises(NC.ContractError, match="Homography estimation failed."):
        NA.estimate(feats, cut)
    F, M = CR.to_package(feats, cut)
    with pytest.raises(S.StitchingError, match="Homography estimation failed."):
        S.CameraSolver(model="affine").estimate(F, M)
    # a = b = 0 and parameters that are not finite
    zero = lambda p: (np.zeros(4), np.zeros((4, 8)), np.zeros((4, 36)))  # noqa: E731
    bad = [np.zeros((3, 3), np.float32)] * 5
    with pytest.raises(NC.ContractError, match="adjusting failed"):
        NA.adjust(feats, matches, bad, evaluate=zero)
    assert not np.isfinite(NA.variants(np.zeros((1, 4)))[0, 0]).all()  # d == 0: the base variant is not finite


# ---- the package's host steps ------------------------------------------------------------------------------------------------------------
def test_host_helpers_equal_the_contract():
    rs = np.random.RandomState(5)
    p = np.concatenate([rs.uniform(0.5, 2.0, (7, 1)), rs.uniform(-0.5, 0.5, (7, 1)), rs.uniform(-2000, 2000, (7, 2))], axis=1)
    p[3, :2] = 0.0  # d == 0 at the base: not finite there, finite where a or b has moved
    va, vb = CE.similarity_variants(p), NA.variants(p)
    assert va.shape == (7, 9, 8) and np.array_equal(va.view(np.uint64), vb.view(np.uint64))
    assert not np.isfinite(va[3, 0]).all() and np.isfinite(va[3, 1:5]).all() and np.isfinite(va[[0, 1, 2, 4, 5, 6]]).all()
    for c in (0, 6):  # the second half is the inverse of the first
        for v in range(9):
            assert np.allclose(CE.similarity_matrix(va[c, v, 4:]) @ CE.similarity_matrix(va[c, v, :4]), np.eye(3), atol=1e-9)
    feats = AR.planted_pair(6, 50, AR.AFFINE)
    for f, F in zip(feats, AR.package_features(feats)):
        assert np.array_equal(ME.level0_points(F), NA.uncentred(f))
        assert np.array_equal(ME.level0_points(F) - (320.0, 240.0), ME.centred_points(F))  # 640 x 480: exact in float64
    feats, matches, _ = AR.rig("grid3x2")
    F, M = CR.to_package(feats, matches)
    assert all(np.array_equal(a, b) for a, b in zip(CE.tree_transforms(M, 6), NA.transforms(matches, 6)))
    start = NA.start_parameters(NA.estimate(feats, matches))
    assert np.array_equal(np.array([CE.similarity_parameters(R) for R in NA.estimate(feats, matches)]), start)
    ed = NC.edges(matches, 6)
    offsets, xyuv = CE.edge_points(F, M, ed, [ME.level0_points(f) for f in F])
    want = [NC.edge_points(feats, matches, 6, i, j, [NA.uncentred(f) for f in feats]) for i, j in ed]
    assert offsets.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist() and np.array_equal(xyuv, np.concatenate(want))


@pytest.mark.parametrize("name", ["grid2x2", "row5"])
def test_solver_host_steps_with_the_contract_evaluation(name):
    """CameraSolver(model="affine") with the numpy evaluation in place of the device: everything else of register() is the package's own
    code.  Linear parts within 1e-9, translations within 1e-9 of the panorama's extent."""
    feats, matches, _ = AR.rig(name)
    F, M = CR.to_package(feats, matches)
    solver = S.CameraSolver(model="affine")
    idx, cams = solver.register(F, M, evaluate=lambda p, v: NA.normal_equations(feats, matches, p))
    (widx, wcams, winfo), _ = AR.measure(name)
    assert list(idx) == widx and all(solver.info[k] == winfo[k] for k in ("edges", "matches", "evaluations", "accepted"))
    extent = max(np.abs(np.asarray(c["R"], np.float64)[:2, 2]).max() for c in wcams) + max(AR.TILE)
    for cam, want in zip(cams, wcams):
        assert cam.R.dtype == np.float32 and (cam.focal, cam.aspect, cam.ppx, cam.ppy) == (1.0, 1.0, 0.0, 0.0)
        assert np.allclose(cam.R[:2, :2], want["R"][:2, :2], rtol=0, atol=1e-9) and np.allclose(cam.R[:2, 2], want["R"][:2, 2], rtol=0, atol=1e-9 * extent)
        assert np.array_equal(cam.R[2], [0.0, 0.0, 1.0])
    est = solver.estimate(F, M)
    assert all(np.array_equal(e.R, R) and e.focal == 1.0 for e, R in zip(est, NA.estimate(feats, matches)))
    calls = []
    few = S.CameraSolver(model="affine", max_evals=2)
    few.adjust(F, M, est, evaluate=lambda p, v: (calls.append(v.shape), NA.normal_equations(feats, matches, p))[1])
    assert len(calls) == 2 == few.info["evaluations"] and calls[0] == (len(feats), 9, 8)
    with pytest.raises(S.StitchingError, match="adjusting failed"):
        zero = [S.CameraParams(focal=1.0, R=np.zeros((3, 3), np.float32)) for _ in feats]
        solver.adjust(F, M, zero, evaluate=lambda p, v: (np.zeros(len(M)), np.zeros((len(M), 8)), np.zeros((len(M), 36))))


# ---- the models' names, the wrappers -------------------------------------------------------------------------------------------------------
def test_models_and_their_refusals():
    assert S.MatchEstimator().model == "homography" and S.MatchEstimator(model="homography", full_affine=True).model == "homography"
    assert S.MatchEstimator(model="affine").model == "affine_partial" and S.MatchEstimator(model="affine", full_affine=True).model == "affine_full"
    assert S.MatchEstimator(0.3, -1, 500, 3.0, 1).seed == 1  # the positional arguments are what they were
    for bad in ("Affine", "affine_partial", "affine_full", "similarity", "", None, 1):
        with pytest.raises(S.StitchingError, match="model"):
            S.MatchEstimator(model=bad)
    solver = S.CameraSolver()
    assert (solver.model, solver.wave_correct, solver.conf_thresh, solver.max_evals) == ("rotation", "horiz", 1.0, 100)
    affine = S.CameraSolver(model="affine")
    assert (affine.model, affine.wave_correct) == ("affine", "no") and S.CameraSolver(model="affine", wave_correct="no").wave_correct == "no"
    for kind in ("horiz", "vert"):
        with pytest.raises(S.StitchingError, match="wave correction"):
            S.CameraSolver(model="affine", wave_correct=kind)
        with pytest.raises(S.StitchingError, match="wave correction"):
            affine.correct([], kind=kind)
    with pytest.raises(S.StitchingError):
        S.CameraSolver(model="affine", wave_correct="auto")
    with pytest.raises(S.StitchingError, match="model"):
        S.CameraSolver(model="homography")
    cams = [S.CameraParams(focal=1.0, R=np.eye(3, dtype=np.float32))]
    assert affine.correct(cams)[0] is cams[0] and affine.correct(cams, kind="no")[0].R is cams[0].R


def test_wrappers_accept_affine_with_an_affine_object_only():
    class Duck:  # an estimator of the user's without a model: the name "affine" is not its
        def match(self, features):
            return []

    for est in (S.MatchEstimator(model="affine"), S.MatchEstimator(model="affine", full_affine=True)):
        assert S.FeatureMatcher("affine", estimator=est).estimator is est
        assert S.FeatureMatcher("homography", estimator=est).estimator is est  # the name is looked at only to refuse "affine"
    for est in (S.MatchEstimator(), Duck()):
        with pytest.raises(S.StitchingError, match="only a homography is fitted there"):
            S.FeatureMatcher("affine", estimator=est)
    with pytest.raises(S.StitchingError, match="at construction"):
        S.FeatureMatcher("affine", estimator=S.MatchEstimator(model="affine"), try_use_gpu=True)
    affine, rotation = S.CameraSolver(model="affine"), S.CameraSolver()
    assert S.CameraEstimator("affine", solver=affine).solver is affine and S.CameraAdjuster("affine", solver=affine).solver is affine
    with pytest.raises(S.StitchingError, match="has no counterpart in the solver"):
        S.CameraEstimator("affine", solver=rotation)
    with pytest.raises(S.StitchingError, match='"affine" camera adjuster has no counterpart'):
        S.CameraAdjuster("affine", solver=rotation)
    for solver in (affine, rotation):
        with pytest.raises(S.StitchingError, match="reproj"):
            S.CameraAdjuster("reproj", solver=solver)
        with pytest.raises(S.StitchingError, match="xxxxx"):
            S.CameraAdjuster("affine" if solver is affine else "ray", refinement_mask="x_xxx", solver=solver)
        with pytest.raises(S.StitchingError, match="auto"):
            S.WaveCorrector("auto", solver=solver)
    # and the affine names are handed on: estimate and adjust with the contract's evaluation through the wrappers
    feats, matches, _ = AR.rig("grid2x2")
    F, M = CR.to_package(feats, matches)
    est = S.CameraEstimator("affine", solver=affine).estimate(F, M)
    assert all(np.array_equal(a.R, R) for a, R in zip(est, NA.estimate(feats, matches)))

    class Spy:
        model = "affine"

        def adjust(self, features, matches, cameras, conf_thresh=None):
            return ("adjusted", cameras, conf_thresh)

    assert S.CameraAdjuster("affine", solver=Spy(), confidence_threshold=0.4).adjust(F, M, est) == ("adjusted", est, 0.4)
    assert S.WaveCorrector("no", solver=affine).correct(est)[0].R is est[0].R


def test_affine_composer_settings_and_warning():
    assert "AffineComposer" in S.__all__ and issubclass(S.AffineComposer, S.Composer)
    assert S.AffineComposer.AFFINE_DEFAULTS == {"warper_type": "affine", "compensator": "no"}
    assert S.AffineComposer.DEFAULT_SETTINGS == dict(S.Composer.DEFAULT_SETTINGS, warper_type="affine", compensator="no")
    assert S.Composer.DEFAULT_SETTINGS["warper_type"] == "spherical" and S.Composer.DEFAULT_SETTINGS["compensator"] == "gain_blocks"
    assert S.Composer.REGISTRATION_MODELS == ("homography", "rotation") and S.AffineComposer.REGISTRATION_MODELS == ("affine", "affine")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        c = S.AffineComposer(finder="voronoi", warper_type="affine")  # the default itself, and a setting that is no affine default
    assert c.settings["warper_type"] == "affine" and c.settings["compensator"] == "no" and c.settings["finder"] == "voronoi"
    assert c.registration is None and callable(c.stitch)
    with pytest.warns(S.StitchingWarning, match=r"You are overwriting an affine default \(warper_type=affine\) with another value \(plane\). "
                                                 "Make sure this is intended"):
        c = S.AffineComposer(warper_type="plane")
    assert c.settings["warper_type"] == "plane"
    with pytest.warns(S.StitchingWarning, match=r"\(compensator=no\) with another value \(gain\)"):
        S.AffineComposer(compensator="gain")
    for bad in ("matcher_type", "estimator", "adjuster", "wave_correct_kind"):
        with pytest.raises(S.StitchingError, match="Invalid Argument: " + bad):
            S.AffineComposer(**{bad: "affine"})
