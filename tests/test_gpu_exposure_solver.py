"""The device solver of the exposure gain systems (csrc/stx_solve.hip) against the dense restatement tests/numpy_exposure.py::lu_solve
and against the host solver: every comparison is on the bits (view(np.uint64) / bytes), 0 differing values."""
import numpy as np
import pytest

import stitching_amd as S
from stitching_amd import _lib
from stitching_amd.exposure_estimation import lu_solve_device, solve_gains
from tests import numpy_exposure as X
from tests.test_exposure_estimation import _random_stats
from tests.test_gpu_exposure_estimation import CASES, _case

pytestmark = pytest.mark.gpu

NB = _lib.LU_NB
SIZES = (4, 5, NB - 1, NB, NB + 1, 2 * NB + 3, 257, 1000)


def _same_bits(got, want):
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    assert got.shape == want.shape
    differing = int(np.count_nonzero(got.view(np.uint64) != want.view(np.uint64)))
    assert differing == 0, f"{differing} of {got.size} values differ in their bits"


def _swaps(A):
    """Steps of the restatement's elimination whose pivot is not the diagonal row."""
    A = np.array(A, np.float64)
    n, swaps = A.shape[0], 0
    for i in range(n):
        p = i + int(np.argmax(np.abs(A[i:, i])))
        if p != i:
            A[[i, p]] = A[[p, i]]
            swaps += 1
        alpha = A[i + 1:, i] * (-1.0 / A[i, i])
        A[i + 1:, i:] = A[i + 1:, i:] + alpha[:, None] * A[i, i:][None, :]
    return swaps


def _dominant(n, rng):
    A = rng.uniform(-1.0, 1.0, (n, n))
    A[np.arange(n), np.arange(n)] += n
    return A


def _permuted(n, rng):
    A = rng.standard_normal((n, n))
    A[np.arange(n), np.arange(n)] += 3.0
    return A[rng.permutation(n)]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["dominant", "permuted"])
def test_lu_equals_the_dense_restatement(gpu_ctx, kind, n):
    rng = np.random.default_rng([n, len(kind)])
    A = _dominant(n, rng) if kind == "dominant" else _permuted(n, rng)
    b = rng.uniform(-100.0, 100.0, n)
    if kind == "permuted" and NB - 1 <= n <= 257:
        assert _swaps(A) > (n - 1) // 2  # pivoting swaps in most steps
    want = X.lu_solve(A, b, skip_zeros=False)
    assert np.all(np.isfinite(want))
    got, info = lu_solve_device(A, b, gpu_ctx, want_info=True)
    _same_bits(got, want)
    assert info["u_nonzeros"] >= n
    _same_bits(lu_solve_device(A, b, gpu_ctx), want)  # and again: the same bits run to run


@pytest.mark.parametrize("n", [5, NB + 1, 2 * NB + 3, 150])
def test_lu_pivot_ties_take_the_smallest_row(gpu_ctx, n):
    """Columns whose largest magnitude appears several times, with both signs."""
    rng = np.random.default_rng(900 + n)
    for _ in range(50):
        A = rng.integers(1, 4, (n, n)).astype(np.float64) * rng.choice([-1.0, 1.0], (n, n))
        if np.linalg.matrix_rank(A) == n:
            break
    else:
        raise AssertionError("no regular matrix drawn")
    col0 = np.abs(A[:, 0])
    assert (col0 == col0.max()).sum() > 1 or n < 6
    b = rng.integers(-50, 50, n).astype(np.float64)
    want = X.lu_solve(A, b, skip_zeros=False)
    assert np.all(np.isfinite(want))
    _same_bits(lu_solve_device(A, b, gpu_ctx), want)
    # the tie rule itself, where it decides the result: two rows of equal magnitude and opposite sign in column 0
    T = np.array([[-2.0, 1.0, 0.5, 3.0], [2.0, 1.5, -1.0, 0.25], [1.0, -3.0, 2.0, 1.0], [-2.0, 0.75, 1.0, -1.0]])
    tb = np.array([1.0, 2.0, 3.0, 4.0])
    _same_bits(lu_solve_device(T, tb, gpu_ctx), X.lu_solve(T, tb, skip_zeros=False))


def _block_sparse(n, rng, bs=64):
    """Integer entries in blocks: the diagonal blocks and a few others are filled, the rest is zero (tiles of the trailing update with
    nothing to do); pairs of rows equal up to one diagonal entry with a power-of-two pivot candidate, so that alpha = -1 and the
    update cancels exactly to +0."""
    nb = -(-n // bs)
    A = np.zeros((n, n))
    filled = {(k, k) for k in range(nb)} | {(0, nb - 1), (nb - 1, 0)} | ({(1, nb - 2)} if nb > 3 else set())
    for (r, c) in filled:
        r0, c0 = r * bs, c * bs
        blk = rng.integers(-4, 5, (min(bs, n - r0), min(bs, n - c0))).astype(np.float64)
        A[r0:r0 + blk.shape[0], c0:c0 + blk.shape[1]] = blk
    A[np.arange(n), np.arange(n)] = 64.0
    for t in range(0, min(bs, n) - 1, 2):  # row t + 1 = row t, but for its own diagonal
        A[t + 1] = A[t]
        A[t + 1, t + 1] += 128.0
    return A


@pytest.mark.parametrize("n", [100, 200, 333])
def test_lu_block_sparse_with_exact_cancellations(gpu_ctx, n):
    rng = np.random.default_rng(4000 + n)
    A = _block_sparse(n, rng)
    assert np.linalg.matrix_rank(A) == n
    b = rng.integers(-1000, 1000, n).astype(np.float64)
    b[::7] = 0.0
    want = X.lu_solve(A, b, skip_zeros=False)
    assert np.all(np.isfinite(want))
    _same_bits(X.lu_solve(A, b, skip_zeros=True), want)  # zeros really are passed over without a trace
    got, info = lu_solve_device(A, b, gpu_ctx, want_info=True)
    _same_bits(got, want)
    assert info["u_nonzeros"] < n * (n + 1) // 2  # U kept zeros: cancellations and untouched blocks


def test_lu_singular_matrix_is_an_error(gpu_ctx):
    rng = np.random.default_rng(5)
    A = _dominant(40, rng)
    A[:, 7] = 0.0
    with pytest.raises(S.StitchingError, match="singular at row 7"):
        lu_solve_device(A, np.ones(40), gpu_ctx)
    with pytest.raises(S.StitchingError, match="singular at row 0"):
        lu_solve_device(np.zeros((4, 4)), np.ones(4), gpu_ctx)
    A = _dominant(70, rng)
    A[:, 69] = 0.0
    with pytest.raises(S.StitchingError, match="singular at row 69"):
        lu_solve_device(A, np.ones(70), gpu_ctx)
    # the context still solves afterwards
    A = _dominant(40, rng)
    _same_bits(lu_solve_device(A, np.ones(40), gpu_ctx), X.lu_solve(A, np.ones(40), skip_zeros=False))


def test_lu_refuses_systems_beyond_its_limit(gpu_ctx):
    import ctypes as C

    n = _lib.LU_MAX_N + 1
    x = np.zeros(4)
    dp = C.POINTER(C.c_double)
    rc = gpu_ctx._lib.stx_lu_solve_device(gpu_ctx.handle, n, x.ctypes.data_as(dp), x.ctypes.data_as(dp), x.ctypes.data_as(dp), None)
    assert rc != 0
    msg = gpu_ctx._lib.stx_last_error().decode()
    assert str(n) in msg and str(_lib.LU_MAX_N) in msg


def _pairs(N, I):
    a, b = np.nonzero(np.triu(N))
    return np.stack([a, b], axis=1), np.stack([N[a, b], I[a, b], I[b, a]], axis=1)


@pytest.mark.parametrize("shape,m", [("ring", 4), ("grid", 9), ("disconnected", 40), ("random", 250), ("random", 1200), ("ring", 2048),
                                     ("grid", 3000)])
def test_solve_gains_device_equals_host(gpu_ctx, shape, m):
    rng = np.random.default_rng([m, len(shape)])
    N, I, skip = _random_stats(shape, m, rng)
    pairs, vals = _pairs(N, I)
    host = solve_gains(m, pairs, vals, skip)
    dev = solve_gains(m, pairs, vals, skip, solver="device", ctx=gpu_ctx)
    _same_bits(dev, host)
    assert np.all(dev[skip] == 1.0)


def test_solve_gains_small_systems_stay_on_cramers_rule(gpu_ctx):
    rng = np.random.default_rng(7)
    for m in (1, 2, 3):
        N, I, skip = _random_stats("ring", m, rng, zero_frac=0.0)
        pairs, vals = _pairs(N, I)
        _same_bits(solve_gains(m, pairs, vals, skip, solver="device", ctx=gpu_ctx), solve_gains(m, pairs, vals, skip))


def _feed(kind, solver, corners, imgs, masks, bl, nr_feeds):
    est = S.ExposureEstimator(kind, nr_feeds=nr_feeds, block_size=bl, solver=solver)
    est.feed(corners, imgs, masks)
    assert est.info["solver"] == solver
    return est


@pytest.mark.parametrize("case,nr_feeds", [(c, 1) for c in CASES] + [("n4_affine_bl20", 2), ("n8_negative_bl13", 2), ("special", 2)])
@pytest.mark.parametrize("kind", X.KINDS)
def test_estimator_device_solver_equals_host_solver(oracle, gpu_ctx, kind, case, nr_feeds):
    corners, imgs, masks, bl = _case(oracle, case)
    host = _feed(kind, "host", corners, imgs, masks, bl, nr_feeds)
    dev = _feed(kind, "device", corners, imgs, masks, bl, nr_feeds)
    assert host.info["u_nonzeros"] == 0 and host.info["device_lu_ms"] == 0.0
    assert (dev.info["units"], dev.info["pair_jobs"]) == (host.info["units"], host.info["pair_jobs"])
    hg, dg = host.getMatGains(), dev.getMatGains()
    assert len(hg) == len(dg) == len(imgs)
    for a, b in zip(dg, hg):
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
    want = X.feed(kind, corners, imgs, masks, nr_feeds, bl)
    for g, w in zip(dg, want):
        assert g.shape == w.shape and g.dtype == w.dtype
        if kind == "gain":
            assert np.allclose(g, w, rtol=1e-9, atol=0)
        else:
            assert np.array_equal(g.view(np.uint8), w.view(np.uint8))
    if kind.endswith("_blocks") and case not in ("n1", "special"):  # those two leave no block of two images in common
        assert dev.info["u_nonzeros"] > 0  # the elimination did run on the device


def test_config4_layout_gain_blocks(gpu_ctx):
    """Config 4's low-resolution layout: 64 frames of 365 x 274 on the 16 x 4 grid, 7 744 block unknowns."""
    from tools import bench_exposure as B

    wtype, corners, imgs, masks = B.case("config4_low")
    assert len(imgs) == 64
    dev = _feed("gain_blocks", "device", corners, imgs, masks, 32, 1)
    host = _feed("gain_blocks", "host", corners, imgs, masks, 32, 1)
    assert dev.info["units"] == host.info["units"] == 7744
    print(f"config4_low gain_blocks: host solve {host.info['solve_ms']:.1f} ms, device solve {dev.info['solve_ms']:.1f} ms "
          f"(elimination {dev.info['device_lu_ms']:.1f} ms, tail {dev.info['host_tail_ms']:.1f} ms, U {dev.info['u_nonzeros']} non-zeros)")
    for a, b in zip(dev.getMatGains(), host.getMatGains()):
        assert a.shape == b.shape and a.dtype == np.float32 and a.tobytes() == b.tobytes()
    assert dev.info["u_nonzeros"] >= 7000


def test_config4_columns_channel_blocks(gpu_ctx):
    """4 of config 4's 16 columns, 2 rows: the three systems of "channel_blocks"."""
    from tools import bench_exposure as B

    wtype, corners, imgs, masks = B.grid_case(4, 2)
    assert len(imgs) == 8
    dev = _feed("channel_blocks", "device", corners, imgs, masks, 32, 1)
    host = _feed("channel_blocks", "host", corners, imgs, masks, 32, 1)
    for a, b in zip(dev.getMatGains(), host.getMatGains()):
        assert a.shape == b.shape and a.shape[2] == 3 and a.tobytes() == b.tobytes()
    assert dev.info["u_nonzeros"] > 0


def test_default_solver_is_the_host(oracle, gpu_ctx, monkeypatch):
    monkeypatch.delenv("STITCHING_AMD_EXPOSURE_SOLVER", raising=False)
    assert S.exposure_solver() == "host"
    corners, imgs, masks, bl = _case(oracle, "n3_bl7")
    est = S.ExposureEstimator("gain_blocks", block_size=bl)
    est.feed(corners, imgs, masks)
    assert est.info["solver"] == "host"
    prev = S.set_exposure_solver("device")
    try:
        est.feed(corners, imgs, masks)  # solver=None follows the process-wide mode at every feed
        assert est.info["solver"] == "device"
    finally:
        S.set_exposure_solver(prev)
