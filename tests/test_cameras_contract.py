"""tests/numpy_cameras.py is a solver and not just a definition: on point rigs with known cameras and on four rendered views of a texture
it finds rotations within 0.5 degrees and focals within 1 %.  Also its rules one by one (subset, focals, spanning tree, the ordered sum,
the Jacobian, wave correction), the host-side pieces of the package that need no GPU against it, the wrappers' refusals and that
Composer's settings are what they were.  The device is compared with the contract in tests/test_gpu_cameras.py."""
import json
import math
import os
import warnings

import numpy as np
import pytest

import stitching_amd as S
from stitching_amd import camera_estimation as CE
from tests import camera_rigs as CR
from tests import numpy_cameras as NC
from tests import numpy_matches as NM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "cameras.json")
CASES, measure = CR.CASES, CR.measure


@pytest.mark.parametrize("name", CASES)
def test_contract_finds_the_cameras(name):
    """rotation relative to the centre camera within 0.5 degrees, focal within 1 %: twice what the prototype measured"""
    (idx, cams, info), rec = measure(name)
    print(f"{name}: {rec} (recorded: {json.load(open(PROFILE))['contract'].get(name)})")
    assert idx == list(range(rec["cameras"]))
    assert rec["rotation_error_deg"] < 0.5 and rec["focal_error_percent"] < 1.0
    assert info["accepted"] >= 1 and info["last_E"] < info["first_E"] and info["evaluations"] <= 100
    assert all(c["R"].dtype == np.float32 and c["aspect"] == 1.0 for c in cams)


def test_texture_recipe_is_the_feature_tests():
    from tests.test_features_contract import _texture

    assert np.array_equal(CR.texture(60, 90, 7), _texture(60, 90, 7))


def test_texture_case_is_a_chain():
    feats, matches, _ = CR.texture_case()
    conf = [[matches[i * 4 + j]["confidence"] for j in range(4)] for i in range(4)]
    print("confidences", np.round(conf, 2).tolist(), "matches of (0, 3):", len(matches[3]["matches"]))
    assert conf[0][1] > 1 and conf[1][2] > 1 and conf[2][3] > 1
    assert matches[3]["H"] is None and conf[0][3] == 0
    (_, cams, _), _ = measure("texture")
    assert all((c["ppx"], c["ppy"]) == (160.0, 120.0) for c in cams)


# ---- subset --------------------------------------------------------------------------------------------------------------------------------
def _entries(n, conf):
    """n * n entries with the given confidences {(i, j): c}, as dicts and as the package's objects"""
    d = [NM.empty() for _ in range(n * n)]
    for (i, j), c in conf.items():
        d[i * n + j]["confidence"] = d[j * n + i]["confidence"] = c
    return d, [S.MatchesInfo(confidence=e["confidence"]) for e in d]


def _both_subsets(n, conf, thresh=1.0):
    d, m = _entries(n, conf)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        a = NC.subset(d, n, thresh)
        b = S.CameraSolver(conf_thresh=thresh).subset([None] * n, m)
        c = S.Subsetter(thresh, solver=S.CameraSolver()).subset([str(k) for k in range(n)], [None] * n, m)
    assert a == list(b) == list(c)
    return a


def test_subset_rules():
    assert _both_subsets(4, {(0, 1): 2, (1, 2): 2, (2, 3): 2}) == [0, 1, 2, 3]
    assert _both_subsets(5, {(0, 4): 2, (1, 2): 2, (2, 3): 2}) == [1, 2, 3]            # the largest
    assert _both_subsets(5, {(1, 3): 2, (0, 4): 2}) == [0, 4]                          # a tie: the one with the smallest index
    assert _both_subsets(6, {(3, 5): 2, (1, 2): 2, (0, 4): 1.5, (2, 4): 0.99}) == [0, 4]
    assert _both_subsets(3, {(0, 1): 1.0, (1, 2): 0.999999}) == [0, 1]                 # >= at the threshold
    assert _both_subsets(3, {(0, 1): 1.0, (1, 2): 0.5}, thresh=0.5) == [0, 1, 2]
    assert _both_subsets(3, {}, thresh=0.0) == [0, 1, 2]                               # every pair has a confidence of 0
    assert _both_subsets(4, {(0, 3): 3, (1, 3): 3}) == [0, 1, 3]                       # joined through a later image
    d, m = _entries(3, {(0, 1): 2})
    with pytest.warns(NC.ContractWarning, match="Not all images"):
        NC.subset(d, 3)
    with pytest.warns(S.StitchingWarning, match="Not all images are included in the final panorama"):
        S.CameraSolver().subset([None] * 3, m)
    with pytest.warns(S.StitchingWarning, match="Not all images are included in the final panorama"):
        S.Subsetter(solver=S.CameraSolver()).subset(["a", "b", "c"], [None] * 3, m)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        _both = S.CameraSolver().subset([None] * 2, _entries(2, {(0, 1): 1.0})[1])
    assert _both == [0, 1]
    d, m = _entries(3, {(0, 1): 0.99})
    with pytest.raises(NC.ContractError, match="No match exceeds the given confidence threshold"):
        NC.subset(d, 3)
    with pytest.raises(S.StitchingError, match="No match exceeds the given confidence threshold"):
        S.CameraSolver().subset([None] * 3, m)
    with pytest.raises(S.StitchingError, match="No match exceeds the given confidence threshold"):
        S.Subsetter(solver=S.CameraSolver()).subset(["a", "b", "c"], [None] * 3, m)
    grid = list(range(16))
    want = [5, 7, 13, 15]
    assert NC.subset_matches(grid, [1, 3]) == want == S.CameraSolver.subset_matches(grid, [1, 3]) == S.Subsetter.subset_matches(grid, [1, 3])
    assert S.Subsetter.subset_list("abcd", [1, 3]) == ["b", "d"]


# ---- focals --------------------------------------------------------------------------------------------------------------------------------
def _krk(f0, f1, R0, R1):
    """the homography that takes points of camera 0 to camera 1 (principal points at the origin)"""
    return np.diag([f1, f1, 1.0]) @ R1.T @ R0 @ np.diag([1 / f0, 1 / f0, 1.0])


def test_focals_closed_form():
    rs = np.random.RandomState(5)
    worst = 0.0
    for _ in range(200):
        f0, f1 = rs.uniform(300, 3000, 2)
        H = _krk(f0, f1, CR.rotation(*rs.uniform(-15, 15, 3)), CR.rotation(*(rs.uniform(-1, 1, 3) * (40, 15, 15))))
        H = H / H[2, 2] * rs.choice([-1.0, 1.0])  # any scale, either sign
        for fn in (NC.focals_from_homography, CE.focals_from_homography):
            g0, g1 = fn(H)
            worst = max(worst, abs(g0 - f0) / f0, abs(g1 - f1) / f1)
    print(f"focals of K R K^-1 homographies: {worst:.3g} relative")
    assert worst < 1e-9
    shift = np.array([[1.0, 0, 30.0], [0, 1.0, -12.0], [0, 0, 1.0]])
    assert NC.focals_from_homography(shift) == (None, None) == CE.focals_from_homography(shift)
    assert NC.focals_from_homography(np.zeros((3, 3))) == (None, None) == CE.focals_from_homography(np.zeros((3, 3)))


def _with_H(n, Hs, inliers=None):
    d = [NM.empty() for _ in range(n * n)]
    for (i, j), H in Hs.items():
        e = NM.empty()
        e.update({"src_img_idx": i, "dst_img_idx": j, "H": np.asarray(H, np.float64), "confidence": 2.0,
                  "num_inliers": (inliers or {}).get((i, j), 10)})
        d[i * n + j], d[j * n + i] = e, NM.mirrored(e, i, j)
    return d, [S.MatchesInfo(e["src_img_idx"], e["dst_img_idx"], None, None, e["num_inliers"], e["H"], e["confidence"]) for e in d]


def test_median_and_fallback():
    R = [CR.rotation(y, 2.0, 1.0) for y in (0.0, 20.0, 40.0, 60.0)]
    feats = [CR._features(np.zeros((0, 2)), (800, 600)) for _ in range(4)]
    F, _ = CR.to_package(feats, [])
    # three pairs whose sqrt(f0 f1) are 500, 700 and 900: n - 1 values, the middle one
    d, m = _with_H(4, {(0, 1): _krk(500, 500, R[0], R[1]), (1, 2): _krk(700, 700, R[1], R[2]), (2, 3): _krk(900, 900, R[2], R[3])})
    assert NC.initial_focal(feats, d, 4) == pytest.approx(700.0, rel=1e-9) and CE.starting_focal(F, m) == pytest.approx(700.0, rel=1e-9)
    # an even count: the mean of the two middle values
    d, m = _with_H(4, {(0, 1): _krk(500, 500, R[0], R[1]), (1, 2): _krk(700, 700, R[1], R[2]), (2, 3): _krk(900, 900, R[2], R[3]),
                       (0, 2): _krk(1000, 1000, R[0], R[2])})
    assert NC.initial_focal(feats, d, 4) == pytest.approx(800.0, rel=1e-9) and CE.starting_focal(F, m) == pytest.approx(800.0, rel=1e-9)
    assert NC.initial_focal(feats, d, 4) == CE.starting_focal(F, m)
    # a focal of unequal cameras: the geometric mean
    d, m = _with_H(2, {(0, 1): _krk(400, 900, R[0], R[1])})
    assert NC.initial_focal(feats[:2], d, 2) == pytest.approx(600.0, rel=1e-9) == CE.starting_focal(F[:2], m)
    # fewer than n - 1: the mean of width + height
    d, m = _with_H(4, {(0, 1): _krk(500, 500, R[0], R[1]), (1, 2): np.array([[1.0, 0, 30], [0, 1, 5], [0, 0, 1]]), (2, 3): _krk(900, 900, R[2], R[3])})
    assert NC.initial_focal(feats, d, 4) == 1400.0 == CE.starting_focal(F, m)


def test_spanning_tree_and_centre():
    I = np.eye(3)
    chain = {(k, k + 1): I for k in range(4)}
    for fn, pick in ((NC.spanning_tree, 0), (CE.spanning_tree, 1)):
        use = lambda n, Hs, inl=None: fn(_with_H(n, Hs, inl)[pick], n)  # noqa: E731
        adj, centre = use(5, chain)
        assert centre == 2 and adj == [[1], [0, 2], [1, 3], [2, 4], [3]]
        assert use(4, {(0, 1): I, (1, 2): I, (2, 3): I})[1] == 1                       # two centres: the smaller index
        adj, centre = use(4, {(0, 3): I, (1, 3): I, (2, 3): I})
        assert centre == 3 and adj == [[3], [3], [3], [0, 1, 2]]
        # a triangle: the heaviest two edges are kept; among equal weights the earlier pair
        assert use(3, {(0, 1): I, (0, 2): I, (1, 2): I}, {(0, 1): 10, (0, 2): 30, (1, 2): 20})[0] == [[2], [2], [0, 1]]
        assert use(3, {(0, 1): I, (0, 2): I, (1, 2): I})[0] == [[1, 2], [0], [0]]
        assert use(4, {(0, 1): I, (2, 3): I}) == (None, -1)                            # not connected
    d, m = _with_H(4, {(0, 1): I, (2, 3): I})
    feats = [CR._features(np.zeros((0, 2)), (800, 600)) for _ in range(4)]
    with pytest.raises(NC.ContractError, match="Homography estimation failed."):
        NC.estimate(feats, d)
    with pytest.raises(S.StitchingError, match="Homography estimation failed."):
        S.CameraSolver().estimate(CR.to_package(feats, [])[0], m)
    # only the entry (to, from) was fitted: its inverse is used
    R = [CR.rotation(0, 0, 0), CR.rotation(25, 3, -2), CR.rotation(-20, -1, 4)]
    d, m = _with_H(3, {(0, 1): _krk(600, 600, R[0], R[1]), (0, 2): _krk(600, 600, R[0], R[2]), (1, 2): _krk(600, 600, R[1], R[2])},
                   {(0, 1): 30, (0, 2): 20, (1, 2): 10})
    d[1]["H"], m[1].H = None, None  # (0, 1) gone, (1, 0) stays: still the heaviest edge of the tree; the focals come from the other two
    assert NC.spanning_tree(d, 3) == ([[1, 2], [0], [0]], 0) == CE.spanning_tree(m, 3)
    for cams in (NC.estimate(feats[:3], d), [(c.focal, c.R) for c in S.CameraSolver().estimate(CR.to_package(feats[:3], [])[0], m)]):
        assert [c[0] for c in cams] == pytest.approx([600.0] * 3, rel=1e-9)
        assert max(CR.angle_deg(c[1], Rt) for c, Rt in zip(cams, R)) < 1e-4 and cams[0][1].dtype == np.float32


# ---- the sum, the Jacobian ---------------------------------------------------------------------------------------------------------------
def test_ordered_sum_against_fsum():
    """|ordered - exact| <= 2^-40 sum |term|: a lane adds at most m / 256 terms and the fold 8 more, each with a relative error of 2^-53
    of a partial sum that is at most sum |term| — (m / 256 + 8) 2^-53 < 2^-40 for every m below 2 million"""
    rs = np.random.RandomState(8)
    for m in (0, 1, 5, 255, 256, 257, 1000, 5000):
        terms = rs.standard_normal((m, 45)) * 10.0 ** rs.uniform(-3, 6, (m, 45))
        got = NC.ordered_sum(terms)
        assert got.shape == (45,)
        for a in range(45):
            assert abs(got[a] - math.fsum(terms[:, a])) <= 2.0 ** -40 * math.fsum(np.abs(terms[:, a])), (m, a)
    ones = np.zeros((600, 45))
    ones[:, 0] = 1.0
    assert NC.ordered_sum(ones)[0] == 600.0 and not NC.ordered_sum(np.zeros((0, 45))).any()
    # the order is the contract's: lanes first, then halvings — not numpy's pairwise sum
    x = np.zeros((512, 45))
    x[0, 0], x[256, 0], x[1, 0] = 1.0, 2.0 ** -53, 2.0 ** -53  # lane 0 rounds its small term away; lane 1 keeps its own until the fold
    assert NC.ordered_sum(x)[0] == 1.0 and math.fsum(x[:, 0]) > 1.0


def test_jacobian_against_finite_differences():
    """2 g is the gradient of E: against central differences of E over the assembled system with a step of 1e-4.  Both are central
    differences of smooth functions with steps h <= 1e-3: truncation h^2 / 6 relative (2e-7), rounding of E (1e4 * 2^-52 / 1e-4 = 2e-8
    absolute) — bound 1e-5 of the largest gradient entry."""
    feats, matches, _ = CR.rig("row3")
    cams = NC.estimate(feats, matches)
    p = np.array([[f] + list(NC.rodrigues_vector(R)) for f, R in cams])
    p = p + np.random.RandomState(9).uniform(-1, 1, p.shape) * (5.0, 0.01, 0.01, 0.01)
    ed = NC.edges(matches, 3)
    total = lambda q: NC.assemble(3, ed, *NC.normal_equations(feats, matches, q))  # noqa: E731
    E, g, A = total(p)
    fd = np.zeros(12)
    for k in range(12):
        step = np.zeros(12)
        step[k] = 1e-4
        fd[k] = (total(p + step.reshape(3, 4))[0] - total(p - step.reshape(3, 4))[0]) / 2e-4
    worst = np.abs(2 * g - fd).max() / np.abs(fd).max()
    print(f"gradient 2 g against finite differences of E: {worst:.3g} of the largest entry; E = {E:.1f}")
    assert worst < 1e-5
    assert np.array_equal(A, A.T) and (np.linalg.eigvalsh(A) > -1e-6 * np.abs(A).max()).all()  # J^T J


# ---- wave correction ---------------------------------------------------------------------------------------------------------------------
def test_wave_correction():
    level = [CR.rotation(y, 0.0, 0.0).astype(np.float32) for y in (-40.0, -15.0, 15.0, 40.0)]
    for fn in (lambda Rs, kind: NC.wave_correct(Rs, kind), CE.wave_corrected):
        out = fn(level, "horiz")
        assert all(o.dtype == np.float32 for o in out) and max(CR.angle_deg(a, b) for a, b in zip(out, level)) < 1e-3  # left alone
        skew = [CR.rotation(y, 0.0, 0.0) for y in (-10.0, 15.0, 40.0)]  # level but not centred: turned about the vertical only
        out = fn(skew, "horiz")
        assert all(abs(o[1, 1] - 1.0) < 1e-6 for o in out) and CR.angle_deg(out[1], np.eye(3)) < 1e-3
        tilt = CR.rotation(0.0, 8.0, 5.0)
        waved = [tilt @ R for R in level]
        back = fn(waved, "horiz")
        assert max(CR.angle_deg(a, b) for a, b in zip(back, level)) < 1e-3  # the common tilt is taken out
        assert all(np.array_equal(a, b) for a, b in zip(fn(waved, "no"), waved))
        up = [CR.rotation(0.0, p, 0.0) for p in (-30.0, 0.0, 30.0)]  # a vertical sweep: "vert" brings the x axes' common direction onto row 1
        assert all(abs(abs(o[1, 0]) - 1.0) < 1e-6 for o in fn([tilt @ R for R in up], "vert"))
    rs = np.random.RandomState(10)
    rig = [CR.rotation(*(rs.uniform(-1, 1, 3) * (60, 10, 10))) for _ in range(6)]
    for kind in ("horiz", "vert"):
        a, b = NC.wave_correct(rig, kind), NC.wave_correct(rig, kind, flip=True)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))  # independent of the eigenvector's sign
        assert all(np.allclose(x, y, rtol=0, atol=1e-7) for x, y in zip(a, CE.wave_corrected(rig, kind)))
    with pytest.raises(NC.ContractError):
        NC.wave_correct(rig, "auto")
    cams = [S.CameraParams(focal=500.0, ppx=1.0, ppy=2.0, R=R.astype(np.float32)) for R in rig]
    out = S.CameraSolver(wave_correct="vert").correct(cams)
    assert all(np.array_equal(o.R, w) for o, w in zip(out, NC.wave_correct([c.R for c in cams], "vert")))
    assert all((o.focal, o.ppx, o.ppy) == (500.0, 1.0, 2.0) for o in out) and all(np.array_equal(c.R, R.astype(np.float32)) for c, R in zip(cams, rig))
    via = S.WaveCorrector("vert", solver=S.CameraSolver()).correct(cams)
    assert all(np.array_equal(o.R, v.R) for o, v in zip(out, via))


# ---- the package's host steps ------------------------------------------------------------------------------------------------------------
def test_host_helpers_equal_the_contract():
    rs = np.random.RandomState(11)
    for _ in range(50):
        r = rs.uniform(-1, 1, 3) * 10.0 ** rs.uniform(-4, 0)  # below a half turn
        a, b = CE.rotation_matrix(r), NC.rodrigues(r)
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)) and np.allclose(a @ a.T, np.eye(3), atol=1e-14)
        # two texts of the inverse (the package goes through the quaternion): both give r back
        assert np.allclose(CE.rotation_vector(a), r, rtol=1e-9, atol=1e-15) and np.allclose(NC.rodrigues_vector(b), r, rtol=1e-9, atol=1e-15)
    assert np.array_equal(CE.rotation_matrix(np.zeros(3)), np.eye(3)) and np.array_equal(NC.rodrigues(np.zeros(3)), np.eye(3))
    # half turns and turns next to them, about axes with every pattern of signs and with zero components: the vector's sign is free
    # there, the rotation it stands for is not
    axes = [np.array(a, np.float64) for a in ((0, 1, 0), (1, 0, 0), (0, 0, 1), (1, 1, 1), (1, -1, 1), (-1, 1, 1), (1, 1, -1), (-1, -1, 1),
                                              (0.2, -3, 0.5), (-2, 0.1, -0.3), (0.3, 0.4, -5), (1, -1, 0), (0, 1, -1), (-1, 0, 1))]
    for axis in axes:
        for angle in (math.pi, math.pi - 1e-9, math.pi - 1e-5, math.pi - 1e-3, 3.0):
            R = CE.rotation_matrix(axis / np.linalg.norm(axis) * angle)
            for inverse in (CE.rotation_vector, NC.rodrigues_vector):
                v = inverse(R)
                assert abs(np.linalg.norm(v) - angle) < 1e-7 and np.allclose(CE.rotation_matrix(v), R, rtol=0, atol=1e-9), (axis, angle, inverse)
    p = np.concatenate([rs.uniform(300, 3000, (7, 1)), rs.uniform(-2, 2, (7, 3))], axis=1)
    p[3, 1:] = 0.0  # no turn at the base: its variants turn by the step alone
    va, vb = CE.camera_variants(p), NC.variants(p)
    assert va.shape == (7, 9, 10) and np.array_equal(va.view(np.uint64), vb.view(np.uint64))
    assert np.array_equal(va[:, 0, 0], p[:, 0]) and np.array_equal(va[:, 1, 0], p[:, 0] + 1e-3) and np.array_equal(va[:, 2, 0], p[:, 0] - 1e-3)
    assert np.array_equal(va[:, 3:, 0], np.repeat(p[:, :1], 6, axis=1))
    feats, matches, _ = CR.rig("two_rows6")
    F, M = CR.to_package(feats, matches)
    ed = NC.edges(matches, 6)
    assert CE.ray_edges(M, 6, 1.0) == ed
    offsets, xyuv = CE.edge_points(F, M, ed)
    want = [NC.edge_points(feats, matches, 6, i, j) for i, j in ed]
    assert offsets.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist() and np.array_equal(xyuv, np.concatenate(want))
    E, g, B = NC.normal_equations(feats, matches, p[:6])
    got = CE.assemble_system(6, ed, np.concatenate([E[:, None], g, B], axis=1))
    for a, b in zip(got, NC.assemble(6, ed, E, g, B)):
        assert np.array_equal(np.asarray(a), np.asarray(b))


@pytest.mark.parametrize("name", ["row5", "two_rows6"])
def test_solver_host_steps_with_the_contract_evaluation(name):
    """CameraSolver with the numpy evaluation in place of the device: everything else of register() is the package's own code"""
    feats, matches, _ = CR.rig(name)
    F, M = CR.to_package(feats, matches)
    solver = S.CameraSolver()
    idx, cams = solver.register(F, M, evaluate=lambda p, v: NC.normal_equations(feats, matches, p))
    (widx, wcams, winfo), _ = measure(name)
    assert list(idx) == widx and all(solver.info[k] == winfo[k] for k in ("edges", "matches", "evaluations", "accepted"))
    assert CR.parameters_agree(solver.info["parameters"], winfo["parameters"], NC.spanning_tree(matches, len(feats))[1])
    for cam, want in zip(cams, wcams):
        assert cam.focal == pytest.approx(want["focal"], rel=1e-9) and np.allclose(cam.R, want["R"], rtol=1e-9, atol=0.0)
        assert (cam.ppx, cam.ppy, cam.aspect) == (400.0, 300.0, 1.0) and cam.R.dtype == np.float32
    est = solver.estimate(F, M)
    assert all(e.focal == pytest.approx(f, rel=1e-9) and np.array_equal(e.R, R) for e, (f, R) in zip(est, NC.estimate(feats, matches)))


def test_adjustment_failures():
    """max_evals bounds the evaluations; a system that cannot be solved is a run of rejected steps, not an error"""
    feats, matches, _ = CR.rig("row3")
    F, M = CR.to_package(feats, matches)
    calls = []
    solver = S.CameraSolver(max_evals=3)
    solver.adjust(F, M, solver.estimate(F, M), evaluate=lambda p, v: (calls.append(1), NC.normal_equations(feats, matches, p))[1])
    assert len(calls) == 3 == solver.info["evaluations"]
    _, info = NC.adjust(feats, matches, NC.estimate(feats, matches), max_evals=3)
    assert info["evaluations"] == 3 and info["accepted"] == solver.info["accepted"]
    solver = S.CameraSolver()
    cams = solver.estimate(F, M)
    out = solver.adjust(F, M, cams, evaluate=lambda p, v: (np.ones(3), np.ones((3, 8)), np.zeros((3, 36))))  # A = 0: singular whatever lam is
    assert solver.info["evaluations"] == 1 and solver.info["accepted"] == 0
    assert all(o.focal == pytest.approx(c.focal) for o, c in zip(out, cams))
    with pytest.raises(S.StitchingError):
        solver.adjust(F, M, cams[:2])


# ---- the wrappers --------------------------------------------------------------------------------------------------------------------------
def test_wrappers_and_their_refusals():
    solver = S.CameraSolver()
    assert (solver.conf_thresh, solver.wave_correct, solver.max_evals) == (1.0, "horiz", 100) and solver.info is None
    assert (S.CameraSolver.MAX_CAMERAS, S.CameraSolver.MAX_MATCHES) == (1024, 131072)
    assert {"CameraSolver", "Subsetter", "CameraEstimator", "CameraAdjuster", "WaveCorrector"} <= set(S.__all__)
    for kw in ({"wave_correct": "auto"}, {"wave_correct": "diagonal"}, {"max_evals": 0}):
        with pytest.raises(S.StitchingError):
            S.CameraSolver(**kw)
    # the reference's names and defaults
    assert S.Subsetter.DEFAULT_CONFIDENCE_THRESHOLD == 1 and S.Subsetter.DEFAULT_MATCHES_GRAPH_DOT_FILE is None
    assert tuple(S.CameraEstimator.CAMERA_ESTIMATOR_CHOICES) == ("homography", "affine") and S.CameraEstimator.DEFAULT_CAMERA_ESTIMATOR == "homography"
    assert tuple(S.CameraAdjuster.CAMERA_ADJUSTER_CHOICES) == ("ray", "reproj", "affine", "no")
    assert S.CameraAdjuster.DEFAULT_CAMERA_ADJUSTER == "ray" and S.CameraAdjuster.DEFAULT_REFINEMENT_MASK == "xxxxx"
    assert tuple(S.WaveCorrector.WAVE_CORRECT_CHOICES) == ("horiz", "vert", "auto", "no") and S.WaveCorrector.DEFAULT_WAVE_CORRECTION == "horiz"
    # with a solver: what it has no counterpart for is refused
    with pytest.raises(S.StitchingError, match="affine"):
        S.CameraEstimator("affine", solver=solver)
    with pytest.raises(S.StitchingError):
        S.CameraEstimator(solver=solver, is_focals_estimated=True)
    for name in ("reproj", "affine"):
        with pytest.raises(S.StitchingError, match=name):
            S.CameraAdjuster(name, solver=solver)
    with pytest.raises(S.StitchingError, match="xxxxx"):
        S.CameraAdjuster(refinement_mask="x_xxx", solver=solver)
    with pytest.raises(S.StitchingError, match="xxxxx"):
        S.CameraAdjuster(solver=solver).set_refinement_mask("xxx_x")
    with pytest.raises(S.StitchingError, match="auto"):
        S.WaveCorrector("auto", solver=solver)
    with pytest.raises(S.StitchingError, match="dot file"):
        S.Subsetter(matches_graph_dot_file="graph.txt", solver=solver)
    with pytest.raises(S.StitchingError):
        S.Subsetter(solver=solver).get_matches_graph(["a"], [])
    # and what it has is handed on
    feats, matches, _ = CR.rig("row3")
    F, M = CR.to_package(feats, matches)
    est = S.CameraEstimator(solver=solver).estimate(F, M)
    assert all(np.array_equal(a.R, b.R) and a.focal == b.focal for a, b in zip(est, solver.estimate(F, M)))
    assert S.CameraAdjuster("no", solver=solver).adjust(F, M, est) is est
    class Spy:  # the wrappers hand their own setting on as an argument of the call: the solver they share is not written
        def adjust(self, features, matches, cameras, conf_thresh=None):
            return ("adjusted", features, matches, cameras, conf_thresh)

        def correct(self, cameras, kind=None):
            return ("corrected", cameras, kind)

    assert S.CameraAdjuster(solver=Spy(), confidence_threshold=0.4).adjust(F, M, est) == ("adjusted", F, M, est, 0.4)
    assert S.WaveCorrector("vert", solver=Spy()).correct(est) == ("corrected", est, "vert")
    lower = S.CameraSolver(conf_thresh=5.0)  # no pair is that confident: no edge, unless the call's own threshold is used
    ran = []
    lower.adjust(F, M, est, conf_thresh=1.0, evaluate=lambda p, v: (ran.append(1), NC.normal_equations(feats, matches, p))[1])
    assert lower.info["edges"] == 3 and ran and lower.conf_thresh == 5.0
    assert S.WaveCorrector("no", solver=solver).correct(est)[0].R is est[0].R
    with pytest.raises(S.StitchingError):
        solver.correct(est, kind="auto")
    try:
        import cv2  # noqa: F401
    except ImportError:
        for make in (S.Subsetter, S.CameraEstimator, S.CameraAdjuster, S.WaveCorrector, lambda: S.CameraEstimator("affine"),
                     lambda: S.CameraAdjuster("reproj"), lambda: S.WaveCorrector("auto")):
            with pytest.raises(S.StitchingError, match="OpenCV.*solver="):  # the names stay cv2's: they do not fall to the solver
                make()


def test_composer_settings_are_unchanged():
    assert S.Composer.DEFAULT_SETTINGS == {
        "medium_megapix": 0.6, "warper_type": "spherical", "low_megapix": 0.1, "crop": True, "compensator": "gain_blocks", "nr_feeds": 1,
        "block_size": 32, "finder": "dp_color", "final_megapix": -1, "blender_type": "multiband", "blend_strength": 5}
    for bad in ("confidence_threshold", "wave_correct_kind", "camera_solver", "adjuster"):
        with pytest.raises(S.StitchingError, match="Invalid Argument: " + bad):
            S.Composer(**{bad: 1})
    c = S.Composer(finder="voronoi")
    assert c.registration is None and callable(c.stitch)
