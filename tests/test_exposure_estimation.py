"""Exposure-gain estimation without a GPU: known answers of the restatement (tests/numpy_exposure.py), its solve against numpy's,
the host-only C entry stx_exposure_solve against the restatement bit for bit, and the estimator switch."""
import numpy as np
import pytest

import stitching_amd as S
from stitching_amd import config
from stitching_amd.exposure_estimation import solve_gains
from tests import numpy_exposure as X


# ---------------------------------------------------------------------------------------------------------------------------------
# restatement known answers
# ---------------------------------------------------------------------------------------------------------------------------------
def test_block_split():
    r = X.block_rects(33, 10, 32)
    assert [x1 - x0 for x0, _, x1, _ in r] == [17, 16] and all(y1 - y0 == 10 for _, y0, _, y1 in r)
    assert X.block_grid(33, 10, 32) == (2, 1, 17, 10)
    r = X.block_rects(20, 15, 7)
    assert X.block_grid(20, 15, 7) == (3, 3, 7, 5)
    assert [(x0, x1) for x0, y0, x1, _ in r if y0 == 0] == [(0, 7), (7, 14), (14, 20)]
    assert sorted({(y0, y1) for _, y0, _, y1 in r}) == [(0, 5), (5, 10), (10, 15)]
    assert X.block_rects(64, 64, 32) == [(0, 0, 32, 32), (32, 0, 64, 32), (0, 32, 32, 64), (32, 32, 64, 64)]


def _two(mask_a, mask_b, va=100, vb=50, shift=4):
    """Two 8 x 8 images, the second at (shift, 0): they overlap in columns shift .. 7 of the first."""
    imgs = [np.full((8, 8, 3), va, np.uint8), np.full((8, 8, 3), vb, np.uint8)]
    return [(0, 0), (shift, 0)], imgs, [mask_a, mask_b]


def test_overlapping_rectangles_with_disjoint_masks_give_n_one():
    ma = np.zeros((8, 8), np.uint8)
    ma[:, :4] = 255  # the left half only: nothing inside the overlap
    mb = np.full((8, 8), 255, np.uint8)
    corners, imgs, masks = _two(ma, mb)
    units = X.make_units(corners, imgs, False, 32)
    jobs, pairs = X.pair_stats(corners, imgs, masks, units, None)
    assert pairs == [(0, 0), (0, 1), (1, 1)]
    assert jobs[(0, 1)][0] == 0
    N, I, skip = X.stats_matrices(2, jobs)
    assert N[0, 1] == N[1, 0] == 1 and I[0, 1] == I[1, 0] == 0 and skip.all()
    assert N[0, 0] == 32 and N[1, 1] == 64
    assert [g.item() for g in X.feed("gain", corners, imgs, masks)] == [1.0, 1.0]
    # rectangles that do not overlap at all: N stays 0
    corners, imgs, masks = _two(mb, mb, shift=8)
    jobs, pairs = X.pair_stats(corners, imgs, masks, X.make_units(corners, imgs, False, 32), None)
    assert pairs == [(0, 0), (1, 1)]


def test_only_255_counts():
    m = np.full((8, 8), 255, np.uint8)
    mb = m.copy()
    mb[:, :6] = 254  # inside the overlap (columns 0 .. 3 of b) only columns 6, 7 of b are 255 ... which lie outside it
    mb[0, 0] = 255
    corners, imgs, masks = _two(m, mb)
    jobs, _ = X.pair_stats(corners, imgs, masks, X.make_units(corners, imgs, False, 32), None)
    assert jobs[(0, 1)][0] == 1  # one pixel: b's (0, 0)
    assert jobs[(1, 1)][0] == 8 * 2 + 1
    c, sa, sb = jobs[(0, 1)]
    assert sa == [np.sqrt(3 * 100.0 ** 2)] and sb == [np.sqrt(3 * 50.0 ** 2)]


def test_isolated_image_and_empty_mask_get_gain_one():
    rng = np.random.default_rng(3)
    imgs = [rng.integers(0, 256, (20, 30, 3), dtype=np.uint8) for _ in range(4)]
    masks = [np.full((20, 30), 255, np.uint8) for _ in range(4)]
    masks[3][:] = 0  # overlaps image 0 but has no pixels
    corners = [(0, 0), (15, 5), (500, 500), (5, 2)]
    for kind in X.KINDS:
        g = X.feed(kind, corners, imgs, masks, block_size=8)
        assert np.all(g[2] == 1) and np.all(g[3] == 1), kind
        assert not np.all(g[0] == 1), kind


def test_filter_known_answers():
    c = np.full((4, 5), 1.25, np.float32)
    assert np.array_equal(X.filter_gain_map(c), c)
    imp = np.zeros((9, 9), np.float32)
    imp[4, 4] = 1
    k = np.array([1, 4, 6, 4, 1], np.float64) / 16  # [.25 .5 .25] twice
    want = np.zeros((9, 9))
    want[2:7, 2:7] = np.outer(k, k)
    assert np.array_equal(X.filter_gain_map(imp), want.astype(np.float32))
    one = np.array([[2.0], [0.0], [0.0], [0.0]], np.float32)  # 1 wide: only the column pass, REFLECT_101 at the top
    f = X.filter_gain_map(one)
    step = np.array([1.0, 0.5, 0.0, 0.0]) * 0.5 + 0.25 * np.array([0.5 + 0.5, 1.0 + 0.0, 0.5 + 0.0, 0.0])  # second pass by hand
    assert f.shape == (4, 1) and np.allclose(f[:, 0], step) and f.dtype == np.float32
    assert np.array_equal(X.filter_gain_map(np.full((1, 1), 0.7, np.float32)), np.full((1, 1), 0.7, np.float32))
    three = np.stack([imp, 2 * imp, c[0, 0] * np.ones_like(imp)], axis=2)  # channels filtered independently
    f3 = X.filter_gain_map(three)
    assert np.array_equal(f3[..., 0], X.filter_gain_map(imp)) and np.array_equal(f3[..., 2], three[..., 2])


# ---------------------------------------------------------------------------------------------------------------------------------
# random systems from random overlap graphs
# ---------------------------------------------------------------------------------------------------------------------------------
def _graph(shape, m, rng):
    if shape == "ring":
        return [(i, (i + 1) % m) for i in range(m)] if m > 1 else []
    if shape == "grid":
        s = int(np.ceil(np.sqrt(m)))
        e = []
        for u in range(m):
            y, x = divmod(u, s)
            for v in (u + 1 if x + 1 < s else None, u + s, u + s + 1 if x + 1 < s else None):
                if v is not None and v < m:
                    e.append((u, v))
        return e
    if shape == "disconnected":  # two rings and isolated units
        h = m // 2
        return [(i, i + 1) for i in range(h - 1)] + [(i, i + 1) for i in range(h, m - 3)]
    # random sparse: each unit linked to a few random partners
    return [(u, int(v)) for u in range(m) for v in rng.integers(0, m, 3) if v != u]


def _random_stats(shape, m, rng, zero_frac=0.1):
    """-> N, I (dense m x m), skip; entries of a gain feed (N integer counts, I mean norms)."""
    N = np.zeros((m, m))
    I = np.zeros((m, m))
    skip = np.ones(m, bool)
    for u in range(m):
        N[u, u] = rng.integers(1, 1025)
        I[u, u] = rng.uniform(20, 400)
    for a, b in _graph(shape, m, rng):
        a, b = min(a, b), max(a, b)
        c = 0 if rng.random() < zero_frac else int(rng.integers(1, 1025))
        N[a, b] = N[b, a] = max(1, c)
        if c:
            skip[a] = skip[b] = False
            I[a, b], I[b, a] = rng.uniform(5, 440), rng.uniform(5, 440)
    return N, I, skip


def _abi_gains(N, I, skip):
    m = N.shape[0]
    a, b = np.nonzero(np.triu(N))
    vals = np.stack([N[a, b], I[a, b], I[b, a]], axis=1)
    return solve_gains(m, np.stack([a, b], axis=1), vals, skip)


@pytest.mark.parametrize("m", [1, 2, 3, 4, 5, 8, 17, 60, 150, 320])
def test_restatement_solve_agrees_with_numpy(m):
    rng = np.random.default_rng(100 + m)
    for shape in ("ring", "grid", "random"):
        N, I, skip = _random_stats(shape, m, rng, zero_frac=0.0)
        skip[:] = False  # solve the whole system
        A, b, idx = X.assemble(N, I, skip)
        assert A.shape == (m, m)
        assert np.allclose(A, A.T, rtol=1e-12, atol=0)  # symmetric up to the order of the products
        x = X.cv_solve(A, b)
        ref = np.linalg.solve(A, b)
        assert np.max(np.abs(x - ref) / np.abs(ref)) <= 1e-9, shape


@pytest.mark.parametrize("shape", ["ring", "grid", "disconnected", "random"])
@pytest.mark.parametrize("m", [1, 2, 3, 4, 9, 40, 250])
def test_abi_solve_equals_restatement_bit_for_bit(shape, m):
    rng = np.random.default_rng([ord(shape[0]), len(shape), m])
    N, I, skip = _random_stats(shape, m, rng)
    want = X.single_feed_gains(N, I, skip)
    got = _abi_gains(N, I, skip)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    if (~skip).sum() > 3:
        dense = X.single_feed_gains(N, I, skip, skip_zeros=False)  # the zero-skipping elimination is the dense loop's bits
        assert np.array_equal(dense.view(np.uint64), want.view(np.uint64))


@pytest.mark.parametrize("shape,m", [("grid", 3000), ("ring", 2048), ("random", 1200)])
def test_abi_solve_large_systems(shape, m):
    rng = np.random.default_rng(m)
    N, I, skip = _random_stats(shape, m, rng)
    want = X.single_feed_gains(N, I, skip)
    got = _abi_gains(N, I, skip)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert np.all(np.isfinite(got)) and np.all(got > 0)


def test_abi_small_systems_take_the_small_branch():
    """m = 1, 2, 3 non-skipped units: Cramer's rule, which is not the LU's bits in general."""
    rng = np.random.default_rng(7)
    differ = 0
    for trial in range(40):
        m = 2 + trial % 2
        N, I, skip = _random_stats("ring", m, rng, zero_frac=0.0)
        got = _abi_gains(N, I, skip)
        want = X.single_feed_gains(N, I, skip)
        assert np.array_equal(got, want)
        A, b, _ = X.assemble(N, I, skip)
        differ += not np.array_equal(X.lu_solve(A, b), got)
    assert differ > 0
    assert np.array_equal(_abi_gains(np.full((1, 1), 5.0), np.zeros((1, 1)), np.ones(1, bool)), [1.0])


def test_abi_solve_rejects_bad_pairs():
    with pytest.raises(S.StitchingError):
        solve_gains(2, [[1, 0]], [[1, 1, 1]], [False, False])
    with pytest.raises(S.StitchingError):
        solve_gains(2, [[0, 2]], [[1, 1, 1]], [False, False])


def test_restatement_feed_shapes():
    rng = np.random.default_rng(11)
    imgs = [rng.integers(0, 256, (37, 50, 3), dtype=np.uint8), rng.integers(0, 256, (40, 33, 3), dtype=np.uint8)]
    masks = [np.full(i.shape[:2], 255, np.uint8) for i in imgs]
    corners = [(-10, -3), (20, 5)]
    shapes = {k: [g.shape for g in X.feed(k, corners, imgs, masks)] for k in X.KINDS}
    dtypes = {k: {g.dtype for g in X.feed(k, corners, imgs, masks)} for k in X.KINDS}
    assert shapes["gain"] == [(1, 1), (1, 1)] and shapes["channel"] == [(3, 1), (3, 1)]
    assert shapes["gain_blocks"] == [(2, 2), (2, 2)] and shapes["channel_blocks"] == [(2, 2, 3), (2, 2, 3)]
    assert dtypes["gain"] == {np.dtype(np.float64)} and dtypes["gain_blocks"] == {np.dtype(np.float32)}


# ---------------------------------------------------------------------------------------------------------------------------------
# the switch
# ---------------------------------------------------------------------------------------------------------------------------------
def test_switch_default_is_opencv(monkeypatch):
    monkeypatch.delenv("STITCHING_AMD_EXPOSURE_ESTIMATOR", raising=False)
    monkeypatch.setattr(config, "_exposure_estimator", None)
    assert S.exposure_estimator() == "opencv"
    try:
        import cv2  # noqa: F401
    except ImportError:
        c = S.ExposureErrorCompensator("gain_blocks")
        assert c.compensator is None
        with pytest.raises(S.StitchingError):
            c.feed([], [], [])


def test_switch_device_builds_the_estimator_with_create_default_rules(monkeypatch):
    monkeypatch.setattr(config, "_exposure_estimator", None)
    monkeypatch.delenv("STITCHING_AMD_EXPOSURE_ESTIMATOR", raising=False)
    assert S.set_exposure_estimator("device") == "opencv"
    E = S.ExposureErrorCompensator
    for kind in ("gain", "gain_blocks"):
        e = E(kind, nr_feeds=3, block_size=7).compensator
        assert isinstance(e, S.ExposureEstimator) and (e.kind, e.nr_feeds, e.block_size) == (kind, 1, 32)
    for kind in ("channel", "channel_blocks"):
        e = E(kind, nr_feeds=3, block_size=7).compensator
        assert isinstance(e, S.ExposureEstimator) and (e.kind, e.nr_feeds, e.block_size) == (kind, 3, 7)
    assert E("no").compensator is None
    E("gain").feed([], [], [])  # empty lists: a no-op, no cv2 needed
    other = object()
    assert E("gain", estimator=other).compensator is other
    assert S.set_exposure_estimator("opencv") == "device"


def test_switch_env_var(monkeypatch):
    for val, want in (("device", "device"), ("opencv", "opencv"), ("", "opencv")):
        monkeypatch.setattr(config, "_exposure_estimator", None)
        monkeypatch.setenv("STITCHING_AMD_EXPOSURE_ESTIMATOR", val)
        assert S.exposure_estimator() == want
    monkeypatch.setattr(config, "_exposure_estimator", None)
    monkeypatch.setenv("STITCHING_AMD_EXPOSURE_ESTIMATOR", "cuda")
    with pytest.raises(S.StitchingError):
        S.exposure_estimator()
    monkeypatch.setattr(config, "_exposure_estimator", "opencv")
    with pytest.raises(S.StitchingError):
        S.set_exposure_estimator("bogus")
    assert S.exposure_estimator() == "opencv"


def test_estimator_rejects_bad_arguments():
    with pytest.raises(S.StitchingError):
        S.ExposureEstimator("no")
    with pytest.raises(S.StitchingError):
        S.ExposureEstimator("gain", nr_feeds=0)
    e = S.ExposureEstimator("channel")
    e.feed([], [], [])
    assert e.getMatGains() == []
    m = np.full((4, 4), 255, np.uint8)
    for img, mask in ((np.zeros((4, 4), np.uint8), m), (np.zeros((4, 4, 3), np.float32), m), (np.zeros((4, 4, 4), np.uint8), m),
                      (np.zeros((4, 4, 3), np.uint8), np.zeros((4, 5), np.uint8)), (np.zeros((4, 4, 3), np.uint8), np.zeros((4, 4, 3), np.uint8))):
        with pytest.raises(S.StitchingError):
            e.feed([(0, 0)], [img], [mask])
