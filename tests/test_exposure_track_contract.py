"""The contract of exposure tracking (tests/numpy_exposure_track.py) on the CPU: it tells itself from its near variants on constructed
inputs, the product's host update (stitching_amd.exposure_tracking.track_update) equals it in every bit, and a simulated exposure step
converges at the rate the tracker is given.  No GPU."""
import numpy as np
import pytest

import stitching_amd as S
from stitching_amd.exposure_tracking import _TrackedCompensator, track_update
from tests import constructed_exposure_tracks as CT
from tests import numpy_exposure_track as NT


def loop(c, **kw):
    return NT.pair_stats_loop(c["rects"], c["masks"], c["imgs"], c["stride"], **kw)


@pytest.mark.parametrize("name", sorted(CT.CASES))
def test_vectorised_form_equals_the_per_pixel_loop(name):
    c = CT.CASES[name]()
    pairs, self_counts, stats = CT.expected(c)
    assert np.array_equal(stats, loop(c))
    # c_ii by a loop over the rectangle's own pixels
    for (x, y, w, h), m, cii in zip(c["rects"], c["masks"], self_counts):
        s = c["stride"]
        assert cii == sum(1 for Y in range(y, y + h) for X in range(x, x + w) if X % s == 0 and Y % s == 0 and m[Y - y, X - x] == 255)


def test_the_cases_reach_what_they_name():
    ex = {k: CT.expected(f()) for k, f in CT.CASES.items()}
    assert len(ex["single"][0]) == 0 and ex["single"][1][0] > 0
    assert len(ex["apart"][0]) == 0
    assert ex["thin_strip"][0].tolist() == [[0, 1]] and not ex["thin_strip"][2].any()
    for k in ("negative_s3", "negative_s8", "s1_tiles", "three"):
        assert (ex[k][2][:, 0] > 0).all() and not ex[k][2][:, 7].any(), k
    assert ex["s1_tiles"][2][0, 0] == 150 * 40
    assert len(ex["three"][0]) == 3
    full = CT.expected(CT.case(CT.CASES["grey_mask"]()["rects"], 2, 7))
    assert 0 < ex["grey_mask"][2][0, 0] < full[2][0, 0]
    assert ex["saturated_first"][2][0, 7] > 0 and ex["saturated_first"][2][0, 0] > 0
    e = ex["empty_next_to_full"]
    assert e[0].tolist() == [[0, 1], [0, 2], [1, 2]] and e[2][0, 0] > 0 and not e[2][1:].any() and e[1][2] == 0


def test_floor_mod_is_told_from_truncation_on_negative_corners():
    for name in ("negative_s3", "negative_s8"):
        c = CT.CASES[name]()
        x0 = max(r[0] for r in c["rects"])
        assert x0 < 0 and x0 % c["stride"] != 0   # where C's (x + s - 1) / s is not the ceiling
        assert not np.array_equal(loop(c), loop(c, floor_mod=False)), name
    c = CT.CASES["three"]()   # no negative intersection corner off the lattice ... the variants agree
    c["rects"], c["masks"], c["imgs"] = c["rects"][:2], c["masks"][:2], c["imgs"][:2]
    assert np.array_equal(loop(c), loop(c, floor_mod=False))


def test_grey_mask_values_do_not_count():
    c = CT.CASES["grey_mask"]()
    assert any((m == 128).any() for m in c["masks"])
    right, wrong = loop(c), loop(c, white=False)
    assert wrong[0, 0] > right[0, 0]


def test_saturated_samples_are_rejected():
    c = CT.CASES["saturated_first"]()
    right, wrong = loop(c), loop(c, saturation=False)
    assert right[0, 7] > 0 and wrong[0, 7] == 0 and wrong[0, 0] == right[0, 0] + right[0, 7]
    assert wrong[0, 1:4].sum() != right[0, 1:4].sum()


# ---- the update -----------------------------------------------------------------------------------------------------------------------
def chain(n):
    """neighbours overlap, and every second pair of next-neighbours"""
    return [(a, b) for a in range(n) for b in range(a + 1, n) if b - a == 1 or (b - a == 2 and a % 2 == 0)]


def random_stats(rng, pairs, empty=()):
    st = np.zeros((len(pairs), 8), np.int64)
    for j in range(len(pairs)):
        if j in empty:
            st[j, 7] = 5
            continue
        c = int(rng.integers(50, 5000))
        st[j, 0] = c
        st[j, 1:7] = rng.integers(40 * c, 200 * c, 6)
        st[j, 7] = int(rng.integers(0, 30))
    return st


@pytest.mark.parametrize("n", [1, 2, 3, 5])
@pytest.mark.parametrize("kind", ["gain", "channel"])
def test_track_update_equals_the_contract_bitwise(n, kind):
    """n = 1: nothing to solve; 2 and 3: cv::solve's Cramer branch; 5: its LU"""
    rng = np.random.default_rng(100 * n + len(kind))
    pairs = chain(n)
    planes = NT.planes_of(kind)
    r = rng.uniform(0.6, 1.7, (n, planes))
    counts = rng.integers(0, 9000, n)
    for empty in ((), (0,)) if pairs else ((),):
        st = random_stats(rng, pairs, empty)
        for rate in (1.0, 0.25):
            want, winfo = NT.track_update(kind, r, pairs, counts, st, rate=rate)
            got, ginfo = track_update(kind, r, np.array(pairs, np.int32).reshape(-1, 2), counts, st, rate=rate)
            assert got.dtype == np.float64 and got.tobytes() == want.tobytes(), (n, kind, rate, got, want)
            assert ginfo == winfo
    if n >= 2:
        assert not np.array_equal(want, r)
    # a tight clip is hit, identically
    want, _ = NT.track_update(kind, r, pairs, counts, st, rate=1.0, limits=(0.9, 1.1))
    got, _ = track_update(kind, r, pairs, counts, st, rate=1.0, limits=(0.9, 1.1))
    assert got.tobytes() == want.tobytes() and got.min() >= 0.9 and got.max() <= 1.1


def test_a_failed_solve_keeps_the_plane_and_is_counted():
    pairs, counts = [(0, 1)], np.array([10, 10])
    st = random_stats(np.random.default_rng(5), pairs)
    r = np.array([[1.2, 1.0, 0.9], [0.8, 1.1, 1.0]])

    def bad(N, I, skip):
        return np.array([np.nan, 1.0])

    got, info = NT.track_update("channel", r, pairs, counts, st, solve=bad)
    assert info["solve_failures"] == 3 and np.array_equal(got, r)
    # the product meets one through non-finite residuals: 1 / 0 poisons the system
    r0 = np.array([[0.0], [1.0]])
    with np.errstate(all="ignore"):
        got, info = track_update("gain", r0, pairs, counts, st)
        want, winfo = NT.track_update("gain", r0, pairs, counts, st)
    assert info["solve_failures"] == winfo["solve_failures"] == 1 and np.array_equal(got, r0) and np.array_equal(want, r0)


def test_division_by_r_makes_the_estimate_absolute():
    """rate = 1: r_next is r* of the frame itself, whatever r the images were made with.  Residuals of powers of two scale the integer
    sums exactly, so the right rule gives the same bits; the rule without the division gives a feedback product."""
    rng = np.random.default_rng(11)
    pairs, counts = chain(3), np.array([4000, 4000, 4000])
    base = random_stats(rng, pairs)
    base[:, 7] = 0
    base[:, 1:7] *= 2   # even sums: halving them below is exact
    r = np.array([[2.0], [0.5], [1.0]])
    scaled = base.copy()
    for j, (a, b) in enumerate(pairs):
        scaled[j, 1:4] = (base[j, 1:4] * r[a, 0]).astype(np.int64)
        scaled[j, 4:7] = (base[j, 4:7] * r[b, 0]).astype(np.int64)
        assert np.array_equal(scaled[j, 1:4], base[j, 1:4] * r[a, 0]) and np.array_equal(scaled[j, 4:7], base[j, 4:7] * r[b, 0])
    one = np.ones((3, 1))
    want, _ = NT.track_update("gain", one, pairs, counts, base, rate=1.0)
    right, _ = NT.track_update("gain", r, pairs, counts, scaled, rate=1.0)
    wrong, _ = NT.track_update("gain", r, pairs, counts, scaled, rate=1.0, decompensate=False)
    assert right.tobytes() == want.tobytes()
    assert np.abs(wrong - want).max() > 0.05
    got, _ = track_update("gain", r, pairs, counts, scaled, rate=1.0)
    assert got.tobytes() == want.tobytes()


def simulate(exposure, r, scene, pairs, c=10000):
    """what the lattice would sum: camera a shows scene[j] * exposure[a] * r[a] on pair j, in all three channels, c samples"""
    st = np.zeros((len(pairs), 8), np.int64)
    for j, (a, b) in enumerate(pairs):
        st[j, 0] = c
        st[j, 1:4] = int(round(scene[j] * exposure[a] * r[a, 0] * c))
        st[j, 4:7] = int(round(scene[j] * exposure[b] * r[b, 0] * c))
    return st


def test_an_exposure_step_converges_at_the_rate_and_stays():
    """Camera 1 steps from 1.0 to 1.3.  The target is single_feed_gains of that frame's absolute means.  Every update moves the
    residuals `rate` of the way to the gains solved from integer sums of c = 10000 samples: a mean is off by at most 0.5 / c = 5e-5
    grey levels of about 100, 5e-7 relative, and the gain system (diagonally dominant by its prior) does not amplify that beyond a
    few times — 1e-5 bounds the noise floor with room.  So |r_k - r*| <= (1 - rate)^k |r_0 - r*| + 1e-5."""
    n, rate = 4, 0.25
    pairs, counts = chain(n), np.full(n, 20000)
    scene = np.array([90.0, 110.0, 100.0, 120.0])[:len(pairs)]
    after = np.array([1.0, 1.3, 1.0, 1.0])
    target_stats = simulate(after, np.ones((n, 1)), scene, pairs)   # the same c: N weighs the system
    target, _ = NT.track_update("gain", np.ones((n, 1)), pairs, counts, target_stats, rate=1.0)
    assert abs(target[1, 0] - 1.0) > 0.05
    r = np.ones((n, 1))
    for _ in range(3):   # before the step nothing moves: equal cameras solve to 1
        r, _ = track_update("gain", r, pairs, counts, simulate(np.ones(n), r, scene, pairs), rate=rate)
    assert np.abs(r - 1.0).max() < 1e-5
    e0 = np.abs(r - target).max()
    for k in range(1, 41):
        r, info = track_update("gain", r, pairs, counts, simulate(after, r, scene, pairs), rate=rate)
        assert info["solve_failures"] == 0
        assert np.abs(r - target).max() <= (1.0 - rate) ** k * e0 + 1e-5, k
    assert np.abs(r - target).max() < 2e-5
    for _ in range(200):
        r, _ = track_update("gain", r, pairs, counts, simulate(after, r, scene, pairs), rate=rate)
        assert np.abs(r - target).max() < 2e-5


# ---- effective gains and the class ----------------------------------------------------------------------------------------------------
class _T:   # what _TrackedCompensator reads of a tracker
    def __init__(self, planes):
        self.planes, self.limits = planes, (0.25, 4.0)


@pytest.mark.parametrize("plan_kind", ["no", "gain", "channel"])
@pytest.mark.parametrize("tracker_kind", ["gain", "channel"])
def test_scalar_effective_gains_equal_the_contract(plan_kind, tracker_kind):
    rng = np.random.default_rng(3)
    n, planes = 3, NT.planes_of(tracker_kind)
    r = rng.uniform(0.5, 2.0, (n, planes))
    plan = None
    gains = None
    if plan_kind != "no":
        plan = S.ExposureErrorCompensator(plan_kind, estimator=object())
        gains = [rng.uniform(0.7, 1.4, (3, 1) if plan_kind == "channel" else (1, 1)) for _ in range(n)]
        plan.set_gains(gains)
    comp = _TrackedCompensator(plan, _T(planes))
    comp.refresh(r)
    want = NT.effective_gains(plan_kind, gains, r, tracker_kind)
    assert comp.compensator_type == NT.effective_kind(plan_kind, tracker_kind)
    assert len(comp.gains) == n
    for g, w in zip(comp.gains, want):
        assert np.asarray(g).tobytes() == np.asarray(w, np.float64).tobytes()
    if plan is not None:
        assert plan.gains_version == 1 and all(np.array_equal(a, np.asarray(b).reshape(-1)) for a, b in zip(plan.gains, gains))
    with pytest.raises(S.StitchingError):
        comp.set_gains(want)


def test_block_effective_kinds_and_the_bound():
    assert NT.effective_kind("gain_blocks", "gain") == "gain_blocks" and NT.effective_kind("gain_blocks", "channel") == "channel_blocks"
    assert NT.effective_kind("channel_blocks", "gain") == "channel_blocks"
    m = np.full((2, 3), 1.5, np.float32)
    r = np.array([[1.25, 0.5, 2.0]])
    out = NT.effective_gains("gain_blocks", [m], r, "channel")[0]
    assert out.shape == (2, 3, 3) and out.dtype == np.float32 and np.array_equal(out[0, 0], np.float32(1.5) * r[0].astype(np.float32))
    plan = S.ExposureErrorCompensator("gain_blocks", estimator=object())
    # GAIN_MAP_BOUNDED is recomputed from max|P| * hi: a map bounded by itself (below 8e6) is not with the tracker's upper limit on top
    plan.set_gains([np.full((2, 2), 2.5e6, np.float32), np.full((2, 2), 1.5, np.float32), np.array([[1.0, np.inf]], np.float32)])
    comp = _TrackedCompensator(plan, _T(1))
    assert comp.compensator_type == "gain_blocks"
    assert comp._bounded_flags() == [0, S._lib.GAIN_MAP_BOUNDED, 0]


@pytest.mark.parametrize("bad", [dict(kind="blocks"), dict(rate=0.0), dict(rate=1.5), dict(stride=0), dict(stride=65), dict(stride=2.5),
                                 dict(limits=(1.5, 4.0)), dict(limits=(0.5, 0.9)), dict(limits=(0.5,)), dict(limits=(0.0, 2.0))])
def test_tracker_arguments_are_checked(bad):
    with pytest.raises(S.StitchingError):
        S.ExposureTracker(**bad)


def test_tracker_surface():
    t = S.ExposureTracker()
    assert (t.kind, t.rate, t.stride, t.limits) == ("gain", 0.25, 8, (0.25, 4.0)) and t.factors is None and t.last_stats is None
    assert "ExposureTracker" in S.__all__
    t.reset()
    assert S.ExposureTracker("channel", rate=1, stride=64).planes == 3
