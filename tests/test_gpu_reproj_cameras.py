"""The reprojection model of the project's own camera solver on the MI355X (stitching_amd.CameraSolver(model="reproj"),
csrc/stx_cameras.hip) against its contract tests/numpy_reproj.py: every one of the 120 float64 sums of every edge with equal bits; the
whole solver's counts equal, its parameters within 1e-9 (the same numpy calls on equal sums), held parameters with the bits they started
with.  Inputs are synthetic features and match entries (no images) except for Composer.stitch; the contract's result of an input is
computed once."""
import ctypes as C

import numpy as np
import pytest

import stitching_amd as S
from tests import camera_rigs as CR
from tests import numpy_cameras as NC
from tests import numpy_reproj as NR
from tests import reproj_rigs as RR
from tests.test_gpu_cameras import _problem, _same_bits

pytestmark = pytest.mark.gpu

DIAGONAL = [k * 14 - k * (k - 1) // 2 for k in range(14)]  # of J^T J within B (105)


def _params(seed, n):
    """rows focal, cx, cy, aspect, Rodrigues vector: focals of 630 .. 770 on 800 x 600 images, offsets within 20 px, aspects of 0.95 ..
    1.05, turns within 0.15 rad a component — two cameras are at most 30 degrees apart and a pixel's ray at most 36 degrees off its
    camera's axis, so every point is in front of both cameras and no sum is NaN"""
    rs = np.random.RandomState(seed)
    return np.concatenate([700.0 * rs.uniform(0.9, 1.1, (n, 1)), rs.uniform(-20, 20, (n, 2)), rs.uniform(0.95, 1.05, (n, 1)),
                           rs.uniform(-0.15, 0.15, (n, 3))], axis=1)


def _check(what, feats, matches, params):
    """the device's normal equations against the contract's; the inputs stay as they were"""
    F, M = CR.to_package(feats, matches)
    keep = params.copy()
    before = [(e.matches.copy(), e.inliers_mask.copy()) for e in M]
    solver = S.CameraSolver(model="reproj")
    got = solver.normal_equations(F, M, params)
    want = NR.normal_equations(feats, matches, params)
    assert all(np.isfinite(w).all() for w in want), what
    assert got[1].shape[1:] == (14,) and got[2].shape[1:] == (105,)
    _same_bits(got, want, what)
    assert np.array_equal(params, keep)
    assert all(np.array_equal(e.matches, a) and np.array_equal(e.inliers_mask, b) for e, (a, b) in zip(M, before))
    ed = NC.edges(matches, len(feats))
    assert solver.info["edges"] == len(ed) == len(got[0])
    assert solver.info["matches"] == sum(int(matches[i * len(feats) + j]["num_inliers"]) for i, j in ed)
    return got


def test_one_match():
    """a single match: the sums are its terms, so this isolates the products, differences and divisions from the order of the sum"""
    feats, matches = _problem(1, 2, {(0, 1): 1})
    p = _params(1, 2)
    E, g, B = _check("one match", feats, matches, p)
    V = NR.variants(p)
    terms = NR.match_terms(V[0], V[1], NC.edge_points(feats, matches, 2, 0, 1))
    # as values: a term of -0.0 (camera j's cx against its cy or aspect) added to a lane's +0.0 is +0.0
    assert terms.shape == (1, 120) and np.array_equal(np.concatenate([E, g[0], B[0]]), terms[0])
    assert E[0] > 0 and np.abs(g).max() > 0 and (B[0, DIAGONAL] > 0).all()


@pytest.mark.parametrize("count", [255, 256, 257, 513])
def test_counts_at_the_chunk_and_fold_boundaries(count):
    feats, matches = _problem(300 + count, 2, {(0, 1): count})
    _check(f"{count} matches", feats, matches, _params(count, 2))


def test_an_empty_edge_between_two_busy_ones():
    feats, matches = _problem(3, 3, {(0, 1): 300, (0, 2): 0, (1, 2): 70})
    E, g, B = _check("empty edge", feats, matches, _params(3, 3))
    assert E[1] == 0 and not g[1].any() and not B[1].any() and E[0] > 0 and E[2] > 0
    assert not np.signbit(np.concatenate([E[1:2], g[1], B[1]])).any()  # 120 zeros, all +0.0


def test_two_edges_sharing_a_camera():
    """3 cameras, the edges (0, 1) and (1, 2): camera 1 is the second camera of one edge and the first of the other"""
    feats, matches = _problem(4, 3, {(0, 1): 130, (1, 2): 200})
    assert NC.edges(matches, 3) == [(0, 1), (1, 2)]
    p = _params(4, 3)
    E, g, B = _check("shared camera", feats, matches, p)
    assert len(E) == 2 and E[0] != E[1]
    _check("shared camera, moved", feats, matches, p + np.random.RandomState(5).uniform(-1, 1, p.shape) * (20.0, 3.0, 3.0, 0.01, 0.02, 0.02, 0.02))


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def _launches(ctx):
    return sum(e["calls"] for e in ctx.prof_results() if e["kernel"] in ("reproj_normal_equations", "affine_normal_equations", "ray_normal_equations"))


def test_refusals_come_before_a_launch():
    ctx = S.get_context()
    L = ctx._lib
    ip, llp, dp = C.POINTER(C.c_int), C.POINTER(C.c_longlong), C.POINTER(C.c_double)
    ctx.prof_reset()
    ctx.prof_enable(True)
    try:
        cams, offsets, pts = np.array([0, 1], np.int32), np.array([0, 2], np.int64), np.array([10.0, 20.0, -30.0, 15.0, -50.0, 5.0, -90.0, 2.0])
        h = C.c_void_p()
        assert L.stx_ray_problem_create(ctx.handle, 1, cams.ctypes.data_as(ip), offsets.ctypes.data_as(llp), pts.ctypes.data_as(dp), C.byref(h)) == 0
        try:
            out, info = np.full(120, 7.0), np.zeros(4)
            good = NR.variants(_params(8, 2))
            assert good.shape == (2, 15, 18) and np.isfinite(good).all()
            for bad_at, bad in ((3, np.nan), (271, np.inf), (539, -np.inf)):
                v = good.copy()
                v.reshape(-1)[bad_at] = bad
                assert L.stx_reproj_problem_eval(h, 2, v.ctypes.data_as(dp), out.ctypes.data_as(dp), info.ctypes.data_as(dp)) == -1
            assert L.stx_reproj_problem_eval(h, 1, good.ctypes.data_as(dp), out.ctypes.data_as(dp), info.ctypes.data_as(dp)) == -1  # fewer cameras than named
            assert L.stx_reproj_problem_eval(h, 1025, good.ctypes.data_as(dp), out.ctypes.data_as(dp), info.ctypes.data_as(dp)) == -1
            assert L.stx_reproj_problem_eval(None, 2, good.ctypes.data_as(dp), out.ctypes.data_as(dp), info.ctypes.data_as(dp)) == -1
            assert (out == 7.0).all() and _launches(ctx) == 0
            assert L.stx_reproj_problem_eval(h, 2, good.ctypes.data_as(dp), out.ctypes.data_as(dp), info.ctypes.data_as(dp)) == 0
            assert _launches(ctx) == 1 and info[0] == 1 and info[1] == 2 and np.isfinite(out).all() and out[0] > 0
            assert [e["calls"] for e in ctx.prof_results() if e["kernel"] == "reproj_normal_equations"] == [1]
        finally:
            assert L.stx_ray_problem_free(h) == 0
        # through the class: a focal of 0 at the base makes variants that are not finite; parameters that are not finite
        feats, matches = _problem(9, 2, {(0, 1): 10})
        F, M = CR.to_package(feats, matches)
        solver = S.CameraSolver(model="reproj")
        p = _params(9, 2)
        p[1, 0] = 0.0
        with pytest.raises(S.StitchingError, match="not finite"):
            solver.normal_equations(F, M, p)
        p[1, 3] = np.nan
        with pytest.raises(S.StitchingError, match="finite"):
            solver.normal_equations(F, M, p)
        with pytest.raises(S.StitchingError, match="1024"):
            solver.register([F[0]] * 1025, [])
        assert _launches(ctx) == 1
    finally:
        ctx.prof_enable(False)


# ---- the whole solver ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", ["xxxxx", "x_x_x"])
def test_adjust_equals_the_contract(mask):
    """The 5-camera rig from its planted start.  Counts equal.  The host steps are the same numpy calls on sums with equal bits: focal
    and rotation by camera_rigs.parameters_agree's rule (1e-9 relative, free of the gauge), the principal point and the aspect of the
    cameras returned within 1e-9 relative; held parameters come back with the bits they started with."""
    feats, matches, _ = RR.rig("row5")
    F, M = CR.to_package(feats, matches)
    start = [S.CameraParams(focal=f, aspect=a, ppx=px, ppy=py, R=np.asarray(R).astype(np.float32)) for f, R, px, py, a in RR.start_cameras("row5")]
    solver = S.CameraSolver(model="reproj", refinement_mask=mask)
    cams = solver.adjust(F, M, start)
    wcams, winfo = NR.adjust(feats, matches, [(c.focal, c.R, c.ppx, c.ppy, c.aspect) for c in start], mask)
    for key in ("edges", "matches", "evaluations", "accepted"):
        assert solver.info[key] == winfo[key], (key, solver.info[key], winfo[key])
    assert solver.info["first_E"] == pytest.approx(winfo["first_E"], rel=1e-9) and solver.info["last_E"] == pytest.approx(winfo["last_E"], rel=1e-9)
    got, want = solver.info["parameters"], winfo["parameters"]
    assert got.dtype == np.float64 and CR.parameters_agree(got[:, [0, 4, 5, 6]], want[:, [0, 4, 5, 6]], NC.spanning_tree(matches, 5)[1])
    held = [k for k in range(7) if k not in NR.free_parameters(mask)]
    assert np.array_equal(got[:, held].view(np.uint64), solver.info["start"][:, held].view(np.uint64))
    assert np.array_equal(solver.info["start"].view(np.uint64)[:, :4], winfo["start"].view(np.uint64)[:, :4])
    assert solver.info["device_ms"] > 0 and solver.info["device_ms_with_copy"] >= solver.info["device_ms"]
    for cam, w in zip(cams, wcams):
        assert cam.focal == pytest.approx(w[0], rel=1e-9) and cam.aspect == pytest.approx(w[4], rel=1e-9)
        assert cam.ppx == pytest.approx(w[2], rel=1e-9) and cam.ppy == pytest.approx(w[3], rel=1e-9)
        assert cam.R.dtype == np.float32 and np.allclose(cam.R, w[1], rtol=1e-9, atol=1e-9)
    if mask == "x_x_x":
        assert all(c.aspect == 1.0 for c in cams)
    print(f"row5 {mask}: {solver.info['evaluations']} evaluations, {solver.info['accepted']} accepted, E {solver.info['first_E']:.1f} -> "
          f"{solver.info['last_E']:.1f}, device {solver.info['device_ms']:.3f} ms")


# ---- frames in, panorama out ---------------------------------------------------------------------------------------------------------------
def test_composer_stitch_with_a_reproj_solver():
    imgs, _ = CR.texture_views()
    composer = S.Composer(finder="voronoi")
    solver = S.CameraSolver(model="reproj")
    pano = composer.stitch(imgs, camera_solver=solver)
    reg = composer.registration
    assert reg["indices"] == [0, 1, 2, 3] and len(reg["cameras"]) == 4 and reg["info"]["accepted"] >= 1 and reg["info"] is solver.info
    feats = S.FeatureEstimator().detect(imgs)  # MEDIUM is the images' own size: 0.08 megapixels
    widx, wcams, winfo = NR.register(feats, S.MatchEstimator().match(feats))
    assert list(widx) == [0, 1, 2, 3]
    for key in ("edges", "matches", "evaluations", "accepted"):
        assert reg["info"][key] == winfo[key], (key, reg["info"][key], winfo[key])
    for got, want in zip(reg["cameras"], wcams):
        assert got.focal == pytest.approx(want["focal"], rel=1e-9) and got.aspect == pytest.approx(want["aspect"], rel=1e-9)
        assert got.ppx == pytest.approx(want["ppx"], rel=1e-9) and got.ppy == pytest.approx(want["ppy"], rel=1e-9)
        assert got.R.dtype == np.float32 and np.allclose(got.R, want["R"], rtol=1e-9, atol=1e-9)
    out = np.asarray(pano.numpy())
    assert out.ndim == 3 and out.shape[2] == 3 and out.shape[1] > CR.VIEW_W and out.shape[0] > 0 and out.any()
    print(f"stitch: panorama {out.shape}, focals {[round(c.focal, 1) for c in reg['cameras']]}, "
          f"principal points {[(round(c.ppx, 1), round(c.ppy, 1)) for c in reg['cameras']]}, aspects {[round(c.aspect, 4) for c in reg['cameras']]}")
