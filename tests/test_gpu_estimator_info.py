"""One timing contract for the seven device estimators on the MI355X: the call succeeds, the device time of `info` is positive, the time
with the copies is no shorter than the time without, and the integer entries of `info` are what the numpy contracts (tests/numpy_*.py)
give for the input.  The two seam finders and the cropper are also called at the C level without an info array — the path on which
no timing event exists — and must return the bytes of the timed call.

Inputs are the smallest with one overlapping pair: two seeded 48 x 32 u8 BGR images with full masks at (0, 0) and (32, 0); features,
matches and cameras take the smallest seeded pairs of tests/constructed_features.py and tests/camera_rigs.py.

Two estimators name their times differently, and FeatureEstimator has none: ExposureEstimator's device time is `stats_ms` (with
`device_lu_ms` for the device solver), and `FeatureEstimator.info` holds counts only, which are checked."""
import ctypes as C

import numpy as np
import pytest

import stitching_amd as S
from stitching_amd import _lib
from stitching_amd.cropper import largest_interior_rectangle
from tests import camera_rigs as CR
from tests import constructed_features as CF
from tests import numpy_cameras as NC
from tests import numpy_color_seams as ZC
from tests import numpy_exposure as X
from tests import numpy_features as NF
from tests import numpy_lir as NL
from tests import numpy_matches as NM
from tests import numpy_seams as Z

pytestmark = pytest.mark.gpu

W, H = 48, 32
CORNERS = [(0, 0), (32, 0)]
SIZES = [(W, H), (W, H)]
IMGS = [np.random.RandomState(40 + k).randint(0, 256, (H, W, 3)).astype(np.uint8) for k in range(2)]
MASKS = [np.full((H, W), 255, np.uint8) for _ in range(2)]
IP, DP = C.POINTER(C.c_int), C.POINTER(C.c_double)


def _timed(info, device="device_ms", with_copy="device_ms_with_copy"):
    assert isinstance(info[device], float) and info[device] > 0, info
    if with_copy in info:
        assert info[with_copy] >= info[device], info


@pytest.mark.parametrize("kind, block, solver", [("gain", 32, "host"), ("gain_blocks", 8, "device")])
def test_exposure(gpu_ctx, kind, block, solver):
    """gain: 2 units, solved by Cramer's rule on the host; gain_blocks with 8-pixel blocks: 48 units, of which the 16 in the overlap
    are unknowns of the LU on the device"""
    est = S.ExposureEstimator(kind, block_size=block, solver=solver)
    est.feed(CORNERS, IMGS, MASKS)
    _, first, units = X.feed(kind, CORNERS, IMGS, MASKS, 1, block, want_stats=True)
    assert len(est.getMatGains()) == 2
    assert est.info["units"] == len(units) == (2 if kind == "gain" else 48) and est.info["pair_jobs"] == len(first)
    assert est.info["solver"] == solver
    _timed(est.info, "stats_ms")
    if solver == "device":
        _timed(est.info, "device_lu_ms")
        assert est.info["u_nonzeros"] >= 16  # at least the diagonal of U
    else:
        assert est.info["device_lu_ms"] == 0.0 and est.info["u_nonzeros"] == 0


def _c_seams(ctx, color, want_info):
    """stx_seam_find("voronoi") / stx_color_seam_find at the C level -> the seam masks as numpy arrays"""
    d_imgs, d_masks = [S.as_device(a, ctx) for a in IMGS] if color else [], [S.as_device(m, ctx) for m in MASKS]
    ss, cs = np.array(SIZES, np.int32), np.array(CORNERS, np.int32)
    ia, ma, outs = (C.c_void_p * len(d_imgs))(*[a._h for a in d_imgs]), (C.c_void_p * 2)(*[m._h for m in d_masks]), (C.c_void_p * 2)()
    info = np.zeros(4, np.float64)
    ip = info.ctypes.data_as(DP) if want_info else None
    if color:
        rc = ctx._lib.stx_color_seam_find(ctx.handle, 2, ss.ctypes.data_as(IP), cs.ctypes.data_as(IP), ia, ma, outs, ip)
    else:
        rc = ctx._lib.stx_seam_find(ctx.handle, _lib.SEAM_KINDS["voronoi"], 2, ss.ctypes.data_as(IP), cs.ctypes.data_as(IP), ma, outs, ip)
    _lib.check(rc)
    return [S.DeviceImage(ctx, C.c_void_p(h)).numpy() for h in outs], info


@pytest.mark.parametrize("color", [False, True], ids=["voronoi", "color"])
def test_seams(gpu_ctx, color):
    est = S.ColorSeamEstimator() if color else S.SeamEstimator("voronoi")
    got = est.find(IMGS, CORNERS, MASKS)
    want = ZC.find(IMGS, CORNERS, MASKS) if color else Z.find("voronoi", CORNERS, MASKS, SIZES)
    assert all(isinstance(g, np.ndarray) and np.array_equal(g, w) for g, w in zip(got, want))
    assert any(not np.array_equal(w, m) for w, m in zip(want, MASKS))  # the pair was cut
    assert est.info["pairs"] == len(Z.pairs(CORNERS, SIZES)) == 1 and est.info["levels"] == 1  # one pair: one level
    _timed(est.info)
    timed, info = _c_seams(gpu_ctx, color, True)
    untimed, zeros = _c_seams(gpu_ctx, color, False)
    assert info[0] == 1 and info[1] == 1 and info[2] > 0 and info[3] >= info[2] and not zeros.any()
    for t, u, w in zip(timed, untimed, want):
        assert t.tobytes() == u.tobytes() == w.tobytes()


def test_crop(gpu_ctx):
    """the panorama mask of the two images, 80 x 32, less a corner of each: one component, no hole"""
    mask = np.full((H, 80), 255, np.uint8)
    mask[:5, :7] = 0
    mask[-3:, -20:] = 0
    cropper = S.Cropper()
    rect = cropper.estimate_largest_interior_rectangle(mask)
    assert tuple(rect) == NL.lir(mask) and cropper.info["contours"] == NL.single_contour(mask) == (1, 0)
    _timed(cropper.info)
    xywh, counts, ms = largest_interior_rectangle(mask, gpu_ctx)
    assert xywh == NL.lir(mask) and counts == (1, 0) and ms > 0
    d = S.as_device(mask, gpu_ctx)
    raw = []
    for want_info in (True, False):
        r, c, info = (C.c_int * 4)(), (C.c_int * 2)(), (C.c_double * 1)()
        _lib.check(gpu_ctx._lib.stx_crop_lir(gpu_ctx.handle, d._h, r, c, info if want_info else None))
        assert (info[0] > 0) == want_info
        raw.append(bytes(r) + bytes(c))
    assert raw[0] == raw[1] and tuple(np.frombuffer(raw[0], np.int32)) == xywh + counts


def _views():
    """two 80 x 64 views of one smoothed-noise image, 16 pixels apart"""
    big = CF.smoothed_noise(96, 64, 3)
    return [np.ascontiguousarray(big[:, :80]), np.ascontiguousarray(big[:, 16:])]


def test_features_and_matches(gpu_ctx):
    imgs = _views()
    est = S.FeatureEstimator(nfeatures=120, fast_threshold=10)
    feats = est.detect(imgs)
    want = [NF.detect(a, nfeatures=120, fast_threshold=10) for a in imgs]
    assert [len(f) for f in feats] == [len(w["x"]) for w in want] and min(len(f) for f in feats) > 20
    assert est.info["levels"] == sum(len(w["level_sizes"]) for w in want) and est.info["keypoints"] == sum(len(w["x"]) for w in want)
    # the candidates of every level of both pyramids, before the quotas cut them (no mask)
    candidates = sum(len(NF.candidates(g, 10)[0]) for a in imgs for g in NF.pyramid(NF.grey(a), 8, 1.2))
    assert est.info["candidates"] == candidates > est.info["keypoints"]
    assert set(est.info) == {"levels", "candidates", "keypoints"}  # no time is taken of the detection

    matcher = S.MatchEstimator(ransac_iters=32)
    got = matcher.match(feats)
    ref = NM.match(feats, ransac_iters=32)
    assert np.array_equal(got[1].matches, ref[1]["matches"]) and len(got[1].matches) >= 6
    assert matcher.info["pairs"] == 1 and matcher.info["matches"] == len(ref[1]["matches"])
    _timed(matcher.info)


def test_cameras(gpu_ctx):
    feats, matches, _ = CR.point_rig(21, 2, per_image=60)
    ed = NC.edges(matches, 2)
    assert ed == [(0, 1)]
    F, M = CR.to_package(feats, matches)
    params = np.array([[700.0, 0.01, -0.02, 0.03], [710.0, -0.02, 0.3, 0.01]])
    solver = S.CameraSolver()
    E, _, _ = solver.normal_equations(F, M, params)
    assert np.array_equal(E.view(np.uint64), NC.normal_equations(feats, matches, params)[0].view(np.uint64))
    assert solver.info["edges"] == 1 and solver.info["matches"] == int(matches[1]["num_inliers"]) > 0
    _timed(solver.info)
