"""The project's own camera solver on the MI355X (stitching_amd.CameraSolver, csrc/stx_cameras.hip) against its contract
tests/numpy_cameras.py: every one of the 45 float64 sums of every edge with equal bits; the whole solver's indices and counts equal, its
focals and rotations within 1e-9 (the same numpy calls on equal sums).  Inputs are synthetic features and match entries (no images)
except for the texture case and Composer.stitch; the contract's result of an input is computed once."""
import ctypes as C

import numpy as np
import pytest

import stitching_amd as S
from stitching_amd import _lib
from tests import camera_rigs as CR
from tests import numpy_cameras as NC
from tests import numpy_matches as NM

pytestmark = pytest.mark.gpu


def _problem(seed, n, edges, size=(800, 600), per_image=600, at_limit=False, extra=None):
    """features and match entries made for the kernel: edges {(i, j): inliers}; every edge's matches carry as many non-inliers again,
    interleaved, and a confidence of 2; `extra` pairs get a confidence of exactly 1 (no edge: the rule is >).  at_limit: the points lie
    on the first and last pixels of the image."""
    rs = np.random.RandomState(seed)
    w, h = size
    feats = []
    for _ in range(n):
        if at_limit:
            xy = np.stack([rs.choice([0, 1, w - 2, w - 1], per_image), rs.choice([0, 1, h - 2, h - 1], per_image)], axis=1)
        else:
            xy = np.stack([rs.randint(0, w, per_image), rs.randint(0, h, per_image)], axis=1)
        feats.append(CR._features(xy, size))
    matches = [NM.empty() for _ in range(n * n)]
    for (i, j), m in list(edges.items()) + [(p, 5) for p in (extra or [])]:
        total = 2 * m if m else 7
        mt = np.stack([rs.randint(0, per_image, total), rs.randint(0, per_image, total), rs.randint(0, 80, total)], axis=1).astype(np.int32)
        mask = np.zeros(total, np.uint8)
        mask[rs.permutation(total)[:m]] = 1
        e = NM.empty()
        e.update({"src_img_idx": i, "dst_img_idx": j, "matches": mt, "inliers_mask": mask, "num_inliers": m,
                  "confidence": 2.0 if (i, j) in edges else 1.0})
        matches[i * n + j], matches[j * n + i] = e, NM.mirrored(e, i, j)
    return feats, matches


def _params(seed, n, focal=700.0, turn=0.4):
    rs = np.random.RandomState(seed)
    return np.concatenate([focal * rs.uniform(0.9, 1.1, (n, 1)), rs.uniform(-turn, turn, (n, 3))], axis=1)


def _same_bits(got, want, what):
    for name, g, w in zip(("E", "g", "B"), got, want):
        assert g.dtype == np.float64 and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        bad = np.flatnonzero(g.view(np.uint64).ravel() != w.view(np.uint64).ravel())
        assert bad.size == 0, (what, name, int(bad.size), "first at", int(bad[0]), float(g.ravel()[bad[0]]), float(w.ravel()[bad[0]]))


def _check(what, feats, matches, params):
    """the device's normal equations against the contract's; the inputs stay as they were"""
    F, M = CR.to_package(feats, matches)
    keep = params.copy()
    before = [(e.matches.copy(), e.inliers_mask.copy()) for e in M]
    solver = S.CameraSolver()
    got = solver.normal_equations(F, M, params)
    want = NC.normal_equations(feats, matches, params)
    _same_bits(got, want, what)
    assert np.array_equal(params, keep)
    assert all(np.array_equal(e.matches, a) and np.array_equal(e.inliers_mask, b) for e, (a, b) in zip(M, before))
    ed = NC.edges(matches, len(feats))
    assert solver.info["edges"] == len(ed) == len(got[0])
    assert solver.info["matches"] == sum(int(matches[i * len(feats) + j]["num_inliers"]) for i, j in ed)
    return got


def test_one_match():
    """a single match: the sums are its terms, so this isolates the square root and the division (and the products) from the order"""
    feats, matches = _problem(1, 2, {(0, 1): 1})
    E, g, B = _check("one match", feats, matches, _params(1, 2))
    assert E[0] > 0 and np.abs(g).max() > 0 and (B[0, [0, 8, 15, 21, 26, 30, 33, 35]] > 0).all()  # the diagonal of J^T J


@pytest.mark.parametrize("count", [6, 64, 65, 255, 256, 257, 513])
def test_counts_at_the_chunk_and_fold_boundaries(count):
    feats, matches = _problem(100 + count, 2, {(0, 1): count})
    _check(f"{count} matches", feats, matches, _params(count, 2))


def test_an_empty_edge_between_two_busy_ones():
    feats, matches = _problem(3, 3, {(0, 1): 300, (0, 2): 0, (1, 2): 70})
    E, g, B = _check("empty edge", feats, matches, _params(3, 3))
    assert E[1] == 0 and not g[1].any() and not B[1].any() and E[0] > 0 and E[2] > 0


def test_a_missing_edge_and_a_pair_at_the_threshold():
    """3 cameras, the pair (0, 2) at a confidence of exactly 1: in the subset's graph, but no edge of the adjustment"""
    feats, matches = _problem(4, 3, {(0, 1): 130, (1, 2): 200}, extra=[(0, 2)])
    assert NC.edges(matches, 3) == [(0, 1), (1, 2)] and NC.subset(matches, 3) == [0, 1, 2]
    E, _, _ = _check("missing edge", feats, matches, _params(4, 3))
    assert len(E) == 2


def test_many_cameras_and_perturbed_parameters():
    """6 cameras with large turns, every pair an edge of its own size; then the same edges at parameters moved by a step"""
    sizes = {(i, j): 10 + 37 * i + 11 * j for i in range(6) for j in range(i + 1, 6)}
    feats, matches = _problem(5, 6, sizes)
    p = _params(5, 6, turn=2.5)
    _check("six cameras", feats, matches, p)
    _check("six cameras, moved", feats, matches, p + np.random.RandomState(6).uniform(-0.05, 0.05, p.shape) * (20.0, 1.0, 1.0, 1.0))


def test_points_at_the_coordinate_limit():
    feats, matches = _problem(7, 2, {(0, 1): 90}, size=(32767, 32767), at_limit=True)
    assert abs(NM.centred(feats[0])).max() == 16383.5
    _check("coordinate limit", feats, matches, _params(7, 2, focal=20000.0))


# ---- the whole solver ----------------------------------------------------------------------------------------------------------------------
_WHOLE = {"row3": lambda: CR.rig("row3")[:2], "row8": lambda: CR.rig("row8")[:2], "texture": lambda: CR.texture_case()[:2]}


@pytest.mark.parametrize("name", sorted(_WHOLE))
def test_register_equals_the_contract(name):
    """Indices and counts equal.  Focals, rotations and parameters within 1e-9 relative, with no absolute allowance: the host steps are
    the same numpy calls on sums with equal bits, so they differ by rounding of differently written expressions at most (1e-16 per
    operation, a few hundred operations, a system conditioned well below 1e4).  A float32 R within 1e-9 of another is that float32 in
    every entry; the float64 parameters are compared free of the gauge (CR.parameters_agree)."""
    feats, matches = _WHOLE[name]()
    F, M = CR.to_package(feats, matches)
    solver = S.CameraSolver()
    idx, cams = solver.register(F, M)
    widx, wcams, winfo = NC.register(feats, matches)
    assert list(idx) == list(widx)
    for key in ("edges", "matches", "evaluations", "accepted"):
        assert solver.info[key] == winfo[key], (key, solver.info[key], winfo[key])
    assert solver.info["first_E"] == pytest.approx(winfo["first_E"], rel=1e-9) and solver.info["last_E"] == pytest.approx(winfo["last_E"], rel=1e-9)
    assert solver.info["parameters"].dtype == np.float64 and CR.parameters_agree(solver.info["parameters"], winfo["parameters"], NC.spanning_tree(matches, len(feats))[1])
    assert solver.info["device_ms"] > 0 and solver.info["device_ms_with_copy"] >= solver.info["device_ms"]
    for cam, want, f in zip(cams, wcams, [feats[i] for i in widx]):
        assert cam.focal == pytest.approx(want["focal"], rel=1e-9)
        assert cam.R.dtype == np.float32 and np.allclose(cam.R, want["R"], rtol=1e-9, atol=0.0), (cam.R, want["R"])
        size = f.get("img_size") or f["level_sizes"][0]
        assert (cam.ppx, cam.ppy, cam.aspect) == (size[0] / 2, size[1] / 2, 1.0)
    print(f"{name}: {solver.info['evaluations']} evaluations, {solver.info['accepted']} accepted, E {solver.info['first_E']:.1f} -> "
          f"{solver.info['last_E']:.1f}, device {solver.info['device_ms']:.3f} ms")


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def _launches(ctx):
    return sum(e["calls"] for e in ctx.prof_results() if e["kernel"] == "ray_normal_equations")


def test_refusals_come_before_a_launch():
    ctx = S.get_context()
    L = ctx._lib
    ip, llp, dp = C.POINTER(C.c_int), C.POINTER(C.c_longlong), C.POINTER(C.c_double)
    ctx.prof_reset()
    ctx.prof_enable(True)
    try:
        pts = np.arange(8.0)

        def create(cams, offsets):
            cams, offsets = np.array(cams, np.int32), np.array(offsets, np.int64)
            keep = cams.copy(), offsets.copy(), pts.copy()
            h = C.c_void_p()
            rc = L.stx_ray_problem_create(ctx.handle, len(cams) // 2, cams.ctypes.data_as(ip), offsets.ctypes.data_as(llp), pts.ctypes.data_as(dp),
                                          C.byref(h))
            assert np.array_equal(cams, keep[0]) and np.array_equal(offsets, keep[1]) and np.array_equal(pts, keep[2])
            return rc, h

        for cams, offsets in (([1, 1], [0, 2]), ([2, 1], [0, 2]), ([-1, 1], [0, 2]), ([0, 1024], [0, 2]),  # i >= j, a camera out of range
                              ([0, 1, 1, 2], [0, 2, 1]), ([0, 1], [1, 2]), ([0, 1], [0, -1]),                # offsets that do not ascend
                              ([0, 1], [0, 2 * 65536 + 1])):                                              # too many matches on an edge
            rc, h = create(cams, offsets)
            assert rc == -1 and not h, (cams, offsets, rc)  # STX_ERR_INVALID, no handle
            with pytest.raises(S.StitchingError):
                _lib.check(rc)
        rc, h = create([0, 1], [0, 2])
        assert rc == 0 and h
        try:
            out, info = np.full(45, 7.0), np.zeros(4)
            good = NC.variants(_params(8, 2))
            for bad_at, bad in ((3, np.nan), (95, np.inf), (179, -np.inf)):
                v = good.copy()
                v.reshape(-1)[bad_at] = bad
                assert L.stx_ray_problem_eval(h, 2, v.ctypes.data_as(dp), out.ctypes.data_as(dp), info.ctypes.data_as(dp)) == -1
            assert L.stx_ray_problem_eval(h, 1, good.ctypes.data_as(dp), out.ctypes.data_as(dp), info.ctypes.data_as(dp)) == -1  # fewer cameras than named
            assert L.stx_ray_problem_eval(h, 1025, good.ctypes.data_as(dp), out.ctypes.data_as(dp), info.ctypes.data_as(dp)) == -1
            assert (out == 7.0).all() and _launches(ctx) == 0
            assert L.stx_ray_problem_eval(h, 2, good.ctypes.data_as(dp), out.ctypes.data_as(dp), info.ctypes.data_as(dp)) == 0
            assert _launches(ctx) == 1 and info[0] == 1 and info[1] == 2 and np.isfinite(out).all() and out[0] > 0
        finally:
            assert L.stx_ray_problem_free(h) == 0
        # through the class: too many cameras, parameters that are not finite, too many inlier matches on a pair
        feats, matches = _problem(9, 2, {(0, 1): 10})
        F, M = CR.to_package(feats, matches)
        solver = S.CameraSolver()
        with pytest.raises(S.StitchingError, match="1024"):
            solver.normal_equations([F[0]] * 1025, [], np.ones((1025, 4)))
        with pytest.raises(S.StitchingError, match="1024"):
            solver.register([F[0]] * 1025, [])
        p = _params(9, 2)
        p[1, 2] = np.nan
        with pytest.raises(S.StitchingError, match="finite"):
            solver.normal_equations(F, M, p)
        big = 2 * 65536 + 1
        M[1].matches, M[1].inliers_mask = np.zeros((big, 3), np.int32), np.ones(big, np.uint8)
        with pytest.raises(S.StitchingError, match="131072"):
            solver.normal_equations(F, M, _params(9, 2))
        assert _launches(ctx) == 1
    finally:
        ctx.prof_enable(False)


# ---- frames in, panorama out ---------------------------------------------------------------------------------------------------------------
def test_composer_stitch():
    imgs, _ = CR.texture_views()
    before = [a.copy() for a in imgs]
    composer = S.Composer(finder="voronoi")
    pano = composer.stitch(imgs)
    reg = composer.registration
    assert reg["indices"] == [0, 1, 2, 3] and len(reg["cameras"]) == 4 and reg["info"]["accepted"] >= 1
    feats = S.FeatureEstimator().detect(imgs)  # MEDIUM is the images' own size: 0.08 megapixels
    solver = S.CameraSolver()
    idx, cams = solver.register(feats, S.MatchEstimator().match(feats))
    assert list(idx) == [0, 1, 2, 3]
    for got, want in zip(reg["cameras"], cams):
        assert got.focal == want.focal and np.array_equal(got.R, want.R) and (got.ppx, got.ppy) == (want.ppx, want.ppy) == (160.0, 120.0)
    out = np.asarray(pano.numpy())
    assert out.ndim == 3 and out.shape[2] == 3 and out.shape[1] > CR.VIEW_W and out.shape[0] > 0 and out.any()
    assert all(np.array_equal(a, b) for a, b in zip(imgs, before))
    print(f"stitch: panorama {out.shape}, focals {[round(c.focal, 1) for c in cams]}")
