"""The reprojection adjustment's contract (tests/numpy_reproj.py) on the CPU: its ordered sum and gradient, that it is a solver on rigs with
a planted principal-point offset and aspect (tests/reproj_rigs.py), what the refinement mask does, and the host steps and refusals of
stitching_amd.CameraSolver(model="reproj") and CameraAdjuster with the contract's evaluation in the device's place.  No GPU."""
import math

import numpy as np
import pytest

import stitching_amd as S
from stitching_amd import camera_estimation as CE
from tests import camera_rigs as CR
from tests import numpy_cameras as NC
from tests import numpy_reproj as NR
from tests import reproj_rigs as RR


def _params(name, seed, scale=(5.0, 2.0, 2.0, 0.01, 0.01, 0.01, 0.01)):
    feats, matches, truth = RR.rig(name)
    p = RR.truth_parameters(truth)
    return feats, matches, p + np.random.RandomState(seed).uniform(-1, 1, p.shape) * scale


# ---- the sums --------------------------------------------------------------------------------------------------------------------------------
def test_ordered_sum_of_the_terms():
    """the contract's ordered sum of every one of the 120 terms against math.fsum: 256 lanes of at most ceil(m / 256) additions and eight
    halvings, each rounding by 2^-53 of a partial sum that is at most sum |term| — far inside 2^-40 sum |term|"""
    feats, matches, p = _params("row5", 1)
    V = NR.variants(p)
    i, j = NC.edges(matches, 5)[0]
    terms = NR.match_terms(V[i], V[j], NC.edge_points(feats, matches, 5, i, j))
    assert terms.shape[1] == NR.SUMS == 1 + 14 + 105 == 1 + len(NR.TRIU) + 14 and len(terms) > 50
    got = NC.ordered_sum(terms)
    worst = 0.0
    for t in range(NR.SUMS):
        exact, size = math.fsum(terms[:, t]), math.fsum(np.abs(terms[:, t]))
        if size == 0:  # camera j's cx against its cy or aspect: one moves the residual's first component only, the other its second
            assert got[t] == 0 and NR.TRIU[t - 15] in ((8, 9), (8, 10))
            continue
        worst = max(worst, abs(got[t] - exact) / size)
        assert abs(got[t] - exact) <= 2.0 ** -40 * size, (t, got[t], exact)
    print(f"ordered sum against fsum: {worst:.3g} of sum |term| at most")
    assert not NC.ordered_sum(np.zeros((0, NR.SUMS))).any() and not np.signbit(NC.ordered_sum(np.zeros((0, NR.SUMS)))).any()


def test_jacobian_against_finite_differences():
    """2 g is the gradient of E: against central differences of E over the assembled system with a step of 1e-4 — numpy_cameras' check on
    the new residual, with its reasoning (truncation h^2 / 6 relative, rounding of E): 1e-5 of the largest gradient entry."""
    feats, matches, p = _params("row5", 2)
    n = 5
    ed = NC.edges(matches, n)
    total = lambda q: NR.assemble(n, ed, *NR.normal_equations(feats, matches, q))  # noqa: E731
    E, g, A = total(p)
    fd = np.zeros(7 * n)
    for k in range(7 * n):
        step = np.zeros(7 * n)
        step[k] = 1e-4
        fd[k] = (total(p + step.reshape(n, 7))[0] - total(p - step.reshape(n, 7))[0]) / 2e-4
    worst = np.abs(2 * g - fd).max() / np.abs(fd).max()
    print(f"gradient 2 g against finite differences of E: {worst:.3g} of the largest entry; E = {E:.1f}")
    assert worst < 1e-5
    assert np.array_equal(A, A.T) and (np.linalg.eigvalsh(A) > -1e-6 * np.abs(A).max()).all()  # J^T J


def test_variants_and_host_helpers_equal_the_contract():
    rs = np.random.RandomState(3)
    p = np.concatenate([rs.uniform(300, 3000, (6, 1)), rs.uniform(-40, 40, (6, 2)), rs.uniform(0.8, 1.25, (6, 1)), rs.uniform(-2, 2, (6, 3))], axis=1)
    p[2, 4:] = 0.0  # no turn at the base
    va, vb = CE.reproj_variants(p), NR.variants(p)
    assert va.shape == (6, 15, 18) and va.dtype == np.float64 and np.array_equal(va.view(np.uint64), vb.view(np.uint64))
    # what a variant is: P = R K^-1 and Q = K R^T, so Q P = I up to rounding, and Q's last row is R's last column
    for c in range(6):
        f, cx, cy, a = p[c, :4]
        K = np.array([[f, 0, cx], [0, f * a, cy], [0, 0, 1.0]])
        R = NC.rodrigues(p[c, 4:])
        assert np.allclose(va[c, 0, :9].reshape(3, 3), R @ np.linalg.inv(K), rtol=1e-12, atol=1e-15)
        assert np.allclose(va[c, 0, 9:].reshape(3, 3), K @ R.T, rtol=1e-12, atol=1e-12)
    for _ in range(50):  # the start's rotation vector, to the bit: the weakly observed parameters amplify a last-bit difference
        R = CE.rotation_matrix(rs.uniform(-1, 1, 3) * 10.0 ** rs.uniform(-4, 0.4)).astype(np.float32)
        assert np.array_equal(CE.rotation_vector(R).view(np.uint64), NR.rotation_vector(R).view(np.uint64))
    assert CE.free_parameters("xxxxx") == NR.free_parameters("xxxxx") == [0, 1, 2, 3, 4, 5, 6]
    assert CE.free_parameters("x_x_x") == NR.free_parameters("x_x_x") == [0, 1, 2, 4, 5, 6]  # the aspect is held
    assert CE.free_parameters("_x_x_") == NR.free_parameters("_x_x_") == [3, 4, 5, 6]        # the skew's character changes nothing
    assert CE.free_parameters("x____") == NR.free_parameters("x____") == [0, 4, 5, 6]
    assert CE.free_parameters("__x__") == [1, 4, 5, 6] and CE.free_parameters("____x") == [2, 4, 5, 6]
    feats, matches, q = _params("two_rows6", 4)
    ed = NC.edges(matches, 6)
    E, g, B = NR.normal_equations(feats, matches, q)
    assert E.shape == (len(ed),) and g.shape == (len(ed), 14) and B.shape == (len(ed), 105)
    got = CE.assemble_system(6, ed, np.concatenate([E[:, None], g, B], axis=1), width=7)
    for a, b in zip(got, NR.assemble(6, ed, E, g, B)):
        assert np.array_equal(np.asarray(a), np.asarray(b))


# ---- the contract is a solver ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(RR.RIGS))
def test_the_contract_is_a_solver(name):
    """800 x 600 images at focal 700 with a planted offset of (12, -9) px and an aspect of 1.02, 0.5 px of noise and rounding; from 1.03 x
    the focal, no offset, aspect 1 and rotations off by up to 1 degree.  Derived, not tuned: E falls; under "xxxxx" the final rms is at
    most 1.02 x the rms of the planted truth on the same points (a least-squares minimum lies at or below the truth's residual; 2 % for
    the lam > 1e12 stop); the models are nested, so E("xxxxx") <= E("x_x_x") <= E("x____") within 1e-6 relative; held parameters come back
    with the bits they started with.  The principal point and the aspect themselves are NOT asserted: a row of pure rotations observes
    them weakly (profiles/reproj.json records what came back)."""
    feats, matches, truth = RR.rig(name)
    n = len(feats)
    last = {}
    for mask in RR.MASKS:
        (cams, info), rec, E_truth = RR.measure(name, mask)
        last[mask] = info["last_E"]
        print(f"{name} {mask}: {rec['evaluations']} evaluations, {rec['accepted']} accepted, rms {rec['rms_start_px']} -> {rec['rms_end_px']} px "
              f"(truth {rec['rms_truth_px']}), rotation {rec['rotation_error_deg']} deg, focal {rec['focal_error_percent']} %, "
              f"camera 0 offset {rec['offset_px'][0]} aspect {rec['aspect'][0]}")
        assert info["last_E"] < info["first_E"] and info["accepted"] >= 1
        held = [k for k in range(7) if k not in NR.free_parameters(mask)]
        got, start = info["parameters"], info["start"]
        assert np.array_equal(got[:, held].view(np.uint64), start[:, held].view(np.uint64))
        assert not np.array_equal(got[:, 4:], start[:, 4:]) and (got[:, 0] != start[:, 0]).all()
        for cam, q, feat in zip(cams, got, feats):
            w0, h0 = feat["img_size"]
            assert cam[1].dtype == np.float32 and (cam[0], cam[2], cam[3], cam[4]) == (q[0], w0 / 2 + q[1], h0 / 2 + q[2], q[3])
        if mask == "xxxxx":
            assert RR.rms(info["last_E"], info["matches"]) <= 1.02 * RR.rms(E_truth, info["matches"])
        else:
            assert all(cam[4] == 1.0 for cam in cams)
        if mask == "x____":
            assert all((cam[2], cam[3]) == (400.0, 300.0) for cam in cams)
    assert last["xxxxx"] <= last["x_x_x"] * (1 + 1e-6) and last["x_x_x"] <= last["x____"] * (1 + 1e-6)
    if name == "two_rows6":  # two rows observe all of it: test_cameras_contract.py's bound for rotation and focal
        _, rec, _ = RR.measure(name, "xxxxx")
        assert rec["rotation_error_deg"] < 0.5 and rec["focal_error_percent"] < 1.0


# ---- the package's host steps ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", ["xxxxx", "x_x_x"])
def test_solver_host_steps_with_the_contract_evaluation(mask):
    """CameraSolver(model="reproj").adjust with the numpy evaluation in place of the device: the start, the free parameters, the loop and
    the cameras are the package's own code"""
    feats, matches, _ = RR.rig("row5")
    F, M = CR.to_package(feats, matches)
    start = [S.CameraParams(focal=f, aspect=a, ppx=px, ppy=py, R=np.asarray(R).astype(np.float32)) for f, R, px, py, a in RR.start_cameras("row5")]
    contract_start = [(c.focal, c.R, c.ppx, c.ppy, c.aspect) for c in start]  # the float32 R both start from
    solver = S.CameraSolver(model="reproj", refinement_mask="xxxxx" if mask != "xxxxx" else "x____")
    cams = solver.adjust(F, M, start, evaluate=lambda p, v: NR.normal_equations(feats, matches, p), refinement_mask=mask)
    wcams, winfo = NR.adjust(feats, matches, contract_start, mask)
    assert all(solver.info[k] == winfo[k] for k in ("edges", "matches", "evaluations", "accepted")), (solver.info, winfo)
    assert solver.info["refinement_mask"] == mask
    got, want = solver.info["parameters"], winfo["parameters"]
    centre = NC.spanning_tree(matches, 5)[1]
    assert CR.parameters_agree(got[:, [0, 4, 5, 6]], want[:, [0, 4, 5, 6]], centre)
    held = [k for k in range(7) if k not in NR.free_parameters(mask)]
    assert np.array_equal(got[:, held].view(np.uint64), solver.info["start"][:, held].view(np.uint64))
    for cam, w in zip(cams, wcams):
        assert cam.focal == pytest.approx(w[0], rel=1e-9) and cam.aspect == pytest.approx(w[4], rel=1e-9)
        assert cam.ppx == pytest.approx(w[2], rel=1e-9) and cam.ppy == pytest.approx(w[3], rel=1e-9)
        assert cam.R.dtype == np.float32 and np.allclose(cam.R, w[1], rtol=1e-9, atol=1e-9)
    # wave correction carries the principal point and the aspect through
    level = S.CameraSolver(model="reproj", wave_correct="horiz").correct(cams)
    assert all((a.focal, a.ppx, a.ppy, a.aspect) == (b.focal, b.ppx, b.ppy, b.aspect) for a, b in zip(level, cams))


def test_register_with_the_contract_evaluation():
    feats, matches, _ = RR.rig("two_rows6")
    F, M = CR.to_package(feats, matches)
    solver = S.CameraSolver(model="reproj")
    idx, cams = solver.register(F, M, evaluate=lambda p, v: NR.normal_equations(feats, matches, p))
    widx, wcams, winfo = NR.register(feats, matches)
    assert list(idx) == list(widx) and all(solver.info[k] == winfo[k] for k in ("edges", "matches", "evaluations", "accepted"))
    for cam, w in zip(cams, wcams):
        assert cam.focal == pytest.approx(w["focal"], rel=1e-9) and cam.aspect == pytest.approx(w["aspect"], rel=1e-9)
        assert cam.ppx == pytest.approx(w["ppx"], rel=1e-9) and cam.ppy == pytest.approx(w["ppy"], rel=1e-9)
        assert cam.R.dtype == np.float32 and np.allclose(cam.R, w["R"], rtol=1e-9, atol=1e-9)
    est = solver.estimate(F, M)
    assert all((e.ppx, e.ppy, e.aspect) == (400.0, 300.0, 1.0) for e in est)  # the rotation model's estimate


# ---- refusals and surface --------------------------------------------------------------------------------------------------------------------
def test_refusals_and_surface():
    assert "reproj" in CE.MODELS
    solver = S.CameraSolver(model="reproj")  # construction needs no GPU
    assert (solver.model, solver.refinement_mask, solver.wave_correct, solver.info) == ("reproj", "xxxxx", "horiz", None)
    assert S.CameraSolver(model="reproj", refinement_mask="x_x_x").refinement_mask == "x_x_x"
    for bad in ("xxxx", "xxxxxx", "xxxxX", "xx-xx", "", None, 5):
        with pytest.raises(S.StitchingError, match="refinement mask"):
            S.CameraSolver(model="reproj", refinement_mask=bad)
        with pytest.raises(NC.ContractError):
            NR.free_parameters(bad)
    for model in ("rotation", "affine"):
        assert S.CameraSolver(model=model, refinement_mask="xxxxx").refinement_mask == "xxxxx"
        with pytest.raises(S.StitchingError, match="xxxxx"):
            S.CameraSolver(model=model, refinement_mask="x_xxx")
    with pytest.raises(S.StitchingError, match="unknown camera model"):
        S.CameraSolver(model="reprojection")
    feats, matches, _ = RR.rig("row5")
    F, M = CR.to_package(feats, matches)
    with pytest.raises(S.StitchingError, match="xxxxx"):  # the override of one call is checked like the constructor's
        S.CameraSolver().adjust(F, M, S.CameraSolver().estimate(F, M), refinement_mask="x____", evaluate=lambda p, v: None)
    with pytest.raises(S.StitchingError, match="refinement mask"):
        solver.adjust(F, M, solver.estimate(F, M), refinement_mask="x", evaluate=lambda p, v: None)
    # the adjuster: "reproj" and a mask go with a solver whose own model says so, and with no other
    adj = S.CameraAdjuster("reproj", solver=solver)
    assert adj.solver is solver and adj.refinement_mask == "xxxxx"
    assert S.CameraAdjuster("reproj", refinement_mask="x_x_x", solver=solver).refinement_mask == "x_x_x"
    adj.set_refinement_mask("x____")
    assert adj.refinement_mask == "x____" and solver.refinement_mask == "xxxxx"  # the solver it shares is not written
    with pytest.raises(S.StitchingError, match="refinement mask"):
        adj.set_refinement_mask("x___")
    with pytest.raises(S.StitchingError, match="refinement mask"):
        S.CameraAdjuster("reproj", refinement_mask="abcde", solver=solver)
    with pytest.raises(S.StitchingError, match='"affine" camera adjuster has no counterpart'):
        S.CameraAdjuster("affine", solver=solver)
    for other in (S.CameraSolver(), S.CameraSolver(model="affine")):
        with pytest.raises(S.StitchingError, match='"reproj" camera adjuster has no counterpart'):
            S.CameraAdjuster("reproj", solver=other)

    class Spy:
        model = "reproj"

        def adjust(self, features, matches, cameras, conf_thresh=None, refinement_mask=None):
            return ("adjusted", cameras, conf_thresh, refinement_mask)

    assert S.CameraAdjuster("reproj", "x_x_x", 0.4, solver=Spy()).adjust(F, M, "cams") == ("adjusted", "cams", 0.4, "x_x_x")
    assert S.CameraAdjuster("no", solver=solver).adjust(F, M, "cams") == "cams"
    # not finite, and the failure conditions of the parameters
    p = RR.truth_parameters(RR.rig("row5")[2])
    p[1, 3] = np.nan
    with pytest.raises(S.StitchingError, match="finite"):
        solver._check_params(p, 5)
    with pytest.raises(S.StitchingError, match="Camera parameters adjusting failed"):
        bad = [S.CameraParams(focal=c.focal, aspect=-1.0, ppx=c.ppx, ppy=c.ppy, R=c.R) for c in solver.estimate(F, M)]
        S.CameraSolver(model="reproj", max_evals=1).adjust(F, M, bad, evaluate=lambda p, v: NR.normal_equations(feats, matches, p))
