"""The affine model of the project's own camera solver on the MI355X (stitching_amd.CameraSolver(model="affine"), csrc/stx_cameras.hip)
against its contract tests/numpy_affine.py: every one of the 45 float64 sums of every edge with equal bits; the whole solver's indices
and counts equal, its transforms within 1e-9 (the same numpy calls on equal sums).  Inputs are synthetic features and match entries (no
images); the contract's result of an input is computed once."""
import ctypes as C

import numpy as np
import pytest

import stitching_amd as S
from tests import affine_rigs as AR
from tests import camera_rigs as CR
from tests import numpy_affine as NA
from tests import numpy_cameras as NC
from tests.test_gpu_cameras import _problem, _same_bits

pytestmark = pytest.mark.gpu


def _params(seed, n):
    """rows a, b, tx, ty: scales of 0.8 .. 1.25, turns within 15 degrees, translations within 800 px"""
    rs = np.random.RandomState(seed)
    scale, turn = rs.uniform(0.8, 1.25, n), np.deg2rad(rs.uniform(-15, 15, n))
    return np.stack([scale * np.cos(turn), scale * np.sin(turn), rs.uniform(-800, 800, n), rs.uniform(-800, 800, n)], axis=1)


def _check(what, feats, matches, params):
    """the device's normal equations against the contract's; the inputs stay as they were"""
    F, M = CR.to_package(feats, matches)
    keep = params.copy()
    before = [(e.matches.copy(), e.inliers_mask.copy()) for e in M]
    solver = S.CameraSolver(model="affine")
    got = solver.normal_equations(F, M, params)
    want = NA.normal_equations(feats, matches, params)
    _same_bits(got, want, what)
    assert np.array_equal(params, keep)
    assert all(np.array_equal(e.matches, a) and np.array_equal(e.inliers_mask, b) for e, (a, b) in zip(M, before))
    ed = NC.edges(matches, len(feats))
    assert solver.info["edges"] == len(ed) == len(got[0])
    assert solver.info["matches"] == sum(int(matches[i * len(feats) + j]["num_inliers"]) for i, j in ed)
    return got


def test_one_match():
    """a single match: the sums are its terms, so this isolates the products and differences from the order of the sum"""
    feats, matches = _problem(1, 2, {(0, 1): 1})
    E, g, B = _check("one match", feats, matches, _params(1, 2))
    assert E[0] > 0 and np.abs(g).max() > 0 and (B[0, [0, 8, 15, 21, 26, 30, 33, 35]] > 0).all()  # the diagonal of J^T J


@pytest.mark.parametrize("count", [255, 256, 257, 513])
def test_counts_at_the_chunk_and_fold_boundaries(count):
    feats, matches = _problem(200 + count, 2, {(0, 1): count})
    _check(f"{count} matches", feats, matches, _params(count, 2))


def test_an_empty_edge_between_two_busy_ones():
    feats, matches = _problem(3, 3, {(0, 1): 300, (0, 2): 0, (1, 2): 70})
    E, g, B = _check("empty edge", feats, matches, _params(3, 3))
    assert E[1] == 0 and not g[1].any() and not B[1].any() and E[0] > 0 and E[2] > 0
    assert not np.signbit(np.concatenate([E[1:2], g[1], B[1]])).any()  # 45 zeros, all +0.0


def test_two_edges_sharing_a_camera():
    """3 cameras, the edges (0, 1) and (1, 2): camera 1 is the second camera of one edge and the first of the other"""
    feats, matches = _problem(4, 3, {(0, 1): 130, (1, 2): 200})
    assert NC.edges(matches, 3) == [(0, 1), (1, 2)]
    p = _params(4, 3)
    E, g, B = _check("shared camera", feats, matches, p)
    assert len(E) == 2 and E[0] != E[1]
    _check("shared camera, moved", feats, matches, p + np.random.RandomState(5).uniform(-1, 1, p.shape) * (0.05, 0.05, 20.0, 20.0))


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def _launches(ctx):
    return sum(e["calls"] for e in ctx.prof_results() if e["kernel"] in ("affine_normal_equations", "ray_normal_equations"))


def test_refusals_come_before_a_launch():
    ctx = S.get_context()
    L = ctx._lib
    ip, llp, dp = C.POINTER(C.c_int), C.POINTER(C.c_longlong), C.POINTER(C.c_double)
    ctx.prof_reset()
    ctx.prof_enable(True)
    try:
        cams, offsets, pts = np.array([0, 1], np.int32), np.array([0, 2], np.int64), np.arange(8.0)
        h = C.c_void_p()
        assert L.stx_ray_problem_create(ctx.handle, 1, cams.ctypes.data_as(ip), offsets.ctypes.data_as(llp), pts.ctypes.data_as(dp), C.byref(h)) == 0
        try:
            out, info = np.full(45, 7.0), np.zeros(4)
            good = NA.variants(_params(8, 2))
            assert good.shape == (2, 9, 8) and np.isfinite(good).all()
            for bad_at, bad in ((3, np.nan), (76, np.inf), (143, -np.inf)):
                v = good.copy()
                v.reshape(-1)[bad_at] = bad
                assert L.stx_affine_problem_eval(h, 2, v.ctypes.data_as(dp), out.ctypes.data_as(dp), info.ctypes.data_as(dp)) == -1
            assert L.stx_affine_problem_eval(h, 1, good.ctypes.data_as(dp), out.ctypes.data_as(dp), info.ctypes.data_as(dp)) == -1  # fewer cameras than named
            assert L.stx_affine_problem_eval(h, 1025, good.ctypes.data_as(dp), out.ctypes.data_as(dp), info.ctypes.data_as(dp)) == -1
            assert L.stx_affine_problem_eval(None, 2, good.ctypes.data_as(dp), out.ctypes.data_as(dp), info.ctypes.data_as(dp)) == -1
            assert (out == 7.0).all() and _launches(ctx) == 0
            assert L.stx_affine_problem_eval(h, 2, good.ctypes.data_as(dp), out.ctypes.data_as(dp), info.ctypes.data_as(dp)) == 0
            assert _launches(ctx) == 1 and info[0] == 1 and info[1] == 2 and np.isfinite(out).all() and out[0] > 0
        finally:
            assert L.stx_ray_problem_free(h) == 0
        # through the class: a = b = 0 at the base makes variants that are not finite; parameters that are not finite
        feats, matches = _problem(9, 2, {(0, 1): 10})
        F, M = CR.to_package(feats, matches)
        solver = S.CameraSolver(model="affine")
        p = _params(9, 2)
        p[1, :2] = 0.0
        with pytest.raises(S.StitchingError, match="not finite"):
            solver.normal_equations(F, M, p)
        p[1, 2] = np.nan
        with pytest.raises(S.StitchingError, match="finite"):
            solver.normal_equations(F, M, p)
        with pytest.raises(S.StitchingError, match="1024"):
            solver.register([F[0]] * 1025, [])
        assert _launches(ctx) == 1
    finally:
        ctx.prof_enable(False)


# ---- the whole solver ----------------------------------------------------------------------------------------------------------------------
def test_register_equals_the_contract():
    """The 3 x 2 rig.  Indices and counts equal.  The host steps are the same numpy calls on sums with equal bits, so they differ by the
    rounding of differently written expressions at most: linear parts within 1e-9, translations within 1e-9 of the panorama's extent —
    an absolute scale, unlike the rays', because the centre's translation is 0 up to rounding."""
    feats, matches, truth = AR.rig("grid3x2")
    F, M = CR.to_package(feats, matches)
    solver = S.CameraSolver(model="affine")
    idx, cams = solver.register(F, M)
    (widx, wcams, winfo), rec = AR.measure("grid3x2")
    assert list(idx) == list(widx) == list(range(6))
    for key in ("edges", "matches", "evaluations", "accepted"):
        assert solver.info[key] == winfo[key], (key, solver.info[key], winfo[key])
    assert solver.info["first_E"] == pytest.approx(winfo["first_E"], rel=1e-9) and solver.info["last_E"] == pytest.approx(winfo["last_E"], rel=1e-9)
    assert solver.info["device_ms"] > 0 and solver.info["device_ms_with_copy"] >= solver.info["device_ms"]
    extent = max(np.abs(np.asarray(c["R"], np.float64)[:2, 2]).max() for c in wcams) + max(AR.TILE)
    for cam, want in zip(cams, wcams):
        assert cam.R.dtype == np.float32 and (cam.focal, cam.aspect, cam.ppx, cam.ppy) == (1.0, 1.0, 0.0, 0.0)
        assert np.allclose(cam.R[:2, :2], want["R"][:2, :2], rtol=0, atol=1e-9), (cam.R, want["R"])
        assert np.allclose(cam.R[:2, 2], want["R"][:2, 2], rtol=0, atol=1e-9 * extent), (cam.R, want["R"])
        assert np.array_equal(cam.R[2], [0.0, 0.0, 1.0])
    _, centre = NC.spanning_tree(matches, 6)
    err = AR.corner_error([c.R for c in cams], truth, centre)
    print(f"grid3x2: {solver.info['evaluations']} evaluations, {solver.info['accepted']} accepted, E {solver.info['first_E']:.1f} -> "
          f"{solver.info['last_E']:.1f}, corner error {err:.4f} px (contract {rec['corner_error_px']}), device {solver.info['device_ms']:.3f} ms")
    assert err <= 2.0 * AR.recorded("grid3x2")
