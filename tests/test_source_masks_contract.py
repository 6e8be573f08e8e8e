"""Source validity masks on the CPU: the numpy contract (tests/numpy_source_masks.py) against the oracle's remap_nearest over the
oracle's maps on every constructed warp case and on the rounding family, the one-mistake variants told apart on named cases, and the
conservative shrink against its brute-force twin."""
import numpy as np
import pytest

from tests import constructed_source_masks as CM
from tests import constructed_warps as CW
from tests import numpy_source_masks as NS
from tests import numpy_warper as NW


def _maps(case):
    return NW.map_backward(case.warper_type, case.scale, case.K, case.R, case.rect)


@pytest.mark.parametrize("family", CW.FAMILIES + ["mask_rounding"])
def test_contract_equals_the_oracle(oracle, family):
    cases = [c for c in CM.ALL_CASES.values() if c.family == family]
    assert cases
    for case in cases:
        xm, ym = oracle.build_maps(case.warper_type, case.scale, case.K, case.R, case.rect)
        for pattern in CM.PATTERNS:
            m = CM.mask(pattern, case.size)
            want = oracle.remap_nearest(m, xm, ym)
            got = NS.warp_source_mask(case.warper_type, case.scale, case.K, case.R, m, case.rect)
            assert got.shape == want.shape == (case.rect[3], case.rect[2])
            assert np.array_equal(got, want), (case.name, pattern, int(np.count_nonzero(got != want)))


def test_patterns_are_what_they_claim():
    for size in sorted({c.size for c in CM.ALL_CASES.values()}):
        h, b = CM.mask("hash", size), CM.mask("binary", size)
        assert h.shape == b.shape == (size[1], size[0])
        assert h.min() >= 1 and h.max() <= 251
        assert set(np.unique(b)) <= {0, 255}
        if size[0] > 1:
            assert (h[:, 1:] != h[:, :-1]).all()
        if size[1] > 1:
            assert (h[1:, :] != h[:-1, :]).all()
    b = CM.mask("binary", (CW.SW, CW.SH))
    assert (b == 0).any() and (b == 255).any()
    # zeroed blocks: somewhere three adjacent zeros, which the checkerboard alone never has
    assert ((b[:, :-2] == 0) & (b[:, 1:-1] == 0) & (b[:, 2:] == 0)).any()
    h = CM.mask("hash", (9, 9))
    assert not np.array_equal(h, h.T)


def test_rounding_family_is_where_pattern_and_coordinate_differ():
    for case in CM.ROUNDING.values():
        xm, ym = _maps(case)
        v = xm if case.facts["axis"] == "x" else ym
        n = case.size[0] if case.facts["axis"] == "x" else case.size[1]
        k = np.floor(v.astype(np.float64))
        assert np.array_equal(v.astype(np.float64) - k, np.full(v.shape, case.facts["frac"]))   # exact: multiples of 1/64
        assert k.min() >= 1 and k.max() <= n - 3   # everything inside, the wavefronts are interior ones
        assert (np.unique(case.facts["waves"]) == [CW.INTERIOR]).all()
        s = NW._cv_round(v * np.float32(32))
        from_s, from_v = (s + 16) >> 5, NW._cv_round(v)
        if case.name.endswith("31_64"):
            assert np.array_equal(from_s, k + 1) and np.array_equal(from_v, k)
        elif case.name.endswith("33_64"):
            assert np.array_equal(from_s, k + 1) and np.array_equal(from_v, k + 1)
        else:
            assert np.array_equal(from_v, k + (k.astype(np.int64) & 1)) and set(np.unique(k.astype(np.int64) & 1)) == {0, 1}


# the named case every one-mistake variant must differ on (hash mask; the first five with the binary mask too)
TELLS = {
    "floor": ("mask_rounding-x-33_64", "mask_rounding-y-33_64"),
    "ties_half_up": ("mask_rounding-x-tie_1_2", "mask_rounding-y-tie_1_2"),
    "index_from_s": ("mask_rounding-x-31_64", "mask_rounding-y-31_64"),
    "interior_255": ("mask_rounding-x-33_64", "phases-q15-plane-x-interior_hi-phases"),
    "border_replicated": ("mask_ties-9x9", "edge_taps-q15-plane-331-x-low"),
    "xy_swapped": ("mask_rounding-x-33_64", "mask_ties-9x9"),
    "pitch_is_width": ("mask_rounding-x-33_64", "mask_rounding-y-33_64"),
}


@pytest.mark.parametrize("variant", NS.VARIANTS)
def test_every_wrong_variant_differs_on_a_named_case(variant):
    assert set(TELLS) == set(NS.VARIANTS)
    for name in TELLS[variant]:
        case = CM.ALL_CASES[name]
        xm, ym = _maps(case)
        patterns = ["hash"] if variant in ("xy_swapped", "pitch_is_width") else ["hash", "binary"]
        for pattern in patterns:
            if variant == "pitch_is_width":
                wide, off = CM.wide_mask(case.size)
                m = wide[:, off:off + case.size[0]]
                wrong = NS.remap_nearest_variant(m, xm, ym, variant, wide=wide, x_off=off)
            else:
                m = CM.mask(pattern, case.size)
                wrong = NS.remap_nearest_variant(m, xm, ym, variant)
            right = NW.remap_nearest_constant(m, xm, ym)
            assert np.array_equal(NS.remap_nearest_variant(m, xm, ym, "none"), right)   # the scaffold itself is the contract
            n = int(np.count_nonzero(wrong != right))
            print(f"{variant} on {name} ({pattern}): {n} differing bytes")
            assert n > 0, (variant, name, pattern)


SHRINKS = [((96, 72), (41, 31)), ((333, 251), (333, 251)), ((67, 5), (1, 1)), ((97, 61), (48, 30)), ((64, 48), (32, 24)), ((33, 7), (1, 7)),
           ((33, 7), (33, 1)), ((4000, 3), (365, 2))]


@pytest.mark.parametrize("src,dst", SHRINKS)
def test_shrink_formula_equals_the_brute_force(src, dst):
    rng = np.random.default_rng(src[0] * 7 + dst[0])
    for density in (0.02, 0.3):   # sparse holes: many footprints are whole; dense: few are
        m = np.where(rng.random((src[1], src[0])) < density, 0, rng.integers(1, 256, (src[1], src[0]))).astype(np.uint8)
        got, want = NS.shrink_mask(m, dst), NS.shrink_mask_brute(m, dst)
        assert got.shape == (dst[1], dst[0]) and set(np.unique(got)) <= {0, 255}
        assert np.array_equal(got, want)
        if src == dst:
            assert np.array_equal(got, np.where(m != 0, 255, 0))   # equal size binarises


def test_shrink_is_conservative_and_covers_the_source():
    src, dst = (96, 72), (41, 31)
    m = CM.binary_mask(*src)
    m[m == 0] = 0
    m[10:40, 20:70] = 200   # a solid block for whole footprints to fall into
    out = NS.shrink_mask(m, dst)
    assert (out == 255).any() and (out == 0).any()
    seen = np.zeros(m.shape, bool)
    for y in range(dst[1]):
        y0, y1 = NS.footprint(y, src[1], dst[1])
        for x in range(dst[0]):
            x0, x1 = NS.footprint(x, src[0], dst[0])
            assert 0 <= x0 < x1 <= src[0] and 0 <= y0 < y1 <= src[1]
            seen[y0:y1, x0:x1] = True
            if out[y, x] == 255:
                assert (m[y0:y1, x0:x1] != 0).all()
            else:
                assert (m[y0:y1, x0:x1] == 0).any()
    assert seen.all()   # the footprints leave no source pixel out: a zero anywhere zeroes some result pixel
    with pytest.raises(ValueError):
        NS.shrink_mask(m, (97, 72))
    with pytest.raises(ValueError):
        NS.shrink_mask(m, (0, 1))
