"""The contract of device frame ingest (tests/numpy_ingest.py) checked against itself: the distance of the integer conversion from the
float64 matrices over all 2^24 (Y, U, V) triples, hand-computed triples, nv12 == i420, odd sizes.  No GPU."""
import numpy as np
import pytest

from tests import numpy_ingest as N


@pytest.mark.parametrize("matrix,range_", N.VARIANTS)
def test_bound_holds_for_every_triple(matrix, range_):
    """|to_bgr - exact| <= 1/2 + delta and |to_bgr - round(exact)| <= floor(1 + delta) with delta derived from the float64 matrices
    (numpy_ingest's docstring), over all 2^24 triples."""
    delta = max(N.coefficient_error(matrix, range_))
    assert 0.0 < delta < 1.0  # "coefficient rounding and the final rounding together suggest 1-2 levels": here 1
    assert N.bound_exact(matrix, range_) == 0.5 + delta and N.bound_levels(matrix, range_) == 1
    u, v = np.arange(256)[None, :, None], np.arange(256)[None, None, :]
    worst_exact, worst_levels = 0.0, 0
    for y0 in range(0, 256, 32):
        y = np.arange(y0, y0 + 32)[:, None, None]
        got = N.yuv_to_bgr(y, u, v, matrix, range_).astype(np.float64)
        ref = N.exact_bgr(y, u, v, matrix, range_)
        worst_exact = max(worst_exact, float(np.abs(got - ref).max()))
        worst_levels = max(worst_levels, int(np.abs(got - np.floor(ref + 0.5)).max()))
    print(f"{matrix} {range_}: delta {delta:.4f}, worst |int - exact| {worst_exact:.4f} (bound {0.5 + delta:.4f}), "
          f"worst |int - round(exact)| {worst_levels} (bound {N.bound_levels(matrix, range_)})")
    assert worst_exact <= N.bound_exact(matrix, range_) + 1e-9
    assert worst_levels <= N.bound_levels(matrix, range_)


def test_docstring_states_the_derived_values():
    for matrix, range_ in N.VARIANTS:
        line = [ln for ln in N.__doc__.splitlines() if ln.strip().startswith(f"{matrix} {range_}")]
        assert len(line) == 1
        words = line[0].split()
        assert float(words[2]) == round(max(N.coefficient_error(matrix, range_)), 4)
        assert float(words[4]) == round(N.bound_exact(matrix, range_), 4) and int(words[5]) == N.bound_levels(matrix, range_)


def test_real_coefficients_round_to_the_stated_constants():
    """"The usual 8-bit-fraction roundings": every integer constant is the nearest integer to 256 times the real one."""
    for matrix, range_ in N.VARIANTS:
        assert tuple(int(np.floor(256.0 * m + 0.5)) for m in N.real_coefficients(matrix, range_)) == N.COEFFICIENTS[(matrix, range_)]
    assert N.coefficients() == (16,) + N.COEFFICIENTS[("bt709", "limited")]
    assert N.coefficients("bt601", "full")[0] == 0
    with pytest.raises(ValueError):
        N.coefficients("bt2020", "limited")


def _one(y, u, v, matrix, range_):
    return tuple(int(c) for c in N.to_bgr((np.full((1, 1), y, np.uint8), np.full((1, 1, 2), (u, v), np.uint8)), "nv12", matrix, range_)[0, 0])


# (Y, U, V) -> (B, G, R), by hand from the formulas of the contract: black, white, the primaries (the standard's own YUV values of pure
# red, green and blue: the 8-bit roundings on both sides leave them within a level of 0 / 255), then both clipping ends.  For
# instance bt601 limited red (81, 90, 240): C = 65 * 298 = 19370, D = -38, E = 112 ->
#   R = (19370 + 409 * 112 + 128) >> 8 = 65306 >> 8 = 255, G = (19370 + 3800 - 23296 + 128) >> 8 = 0, B = (19370 - 19608 + 128) >> 8 = -1 -> 0;
# (255, 255, 255): B = (71222 + 516 * 127 + 128) >> 8 = 534 -> 255, G = (71222 - 12700 - 26416 + 128) >> 8 = 125, R = 481 -> 255;
# (0, 0, 0): B = (-4768 - 66048 + 128) >> 8 = -277 -> 0 (arithmetic shift), G = (-4768 + 12800 + 26624 + 128) >> 8 = 135, R = -223 -> 0
HAND = {
    ("bt601", "limited"): [((16, 128, 128), (0, 0, 0)), ((235, 128, 128), (255, 255, 255)),
                           ((81, 90, 240), (0, 0, 255)), ((145, 54, 34), (1, 255, 0)), ((41, 240, 110), (255, 0, 0)),
                           ((255, 255, 255), (255, 125, 255)), ((0, 0, 0), (0, 135, 0))],
    ("bt709", "limited"): [((16, 128, 128), (0, 0, 0)), ((235, 128, 128), (255, 255, 255)),
                           ((63, 102, 240), (0, 1, 255)), ((173, 42, 26), (1, 255, 0)), ((32, 240, 118), (255, 0, 1)),
                           ((255, 255, 255), (255, 183, 255)), ((0, 0, 0), (0, 77, 0))],
    ("bt601", "full"): [((0, 128, 128), (0, 0, 0)), ((255, 128, 128), (255, 255, 255)),
                        ((76, 85, 255), (0, 0, 254)), ((150, 44, 21), (1, 255, 0)), ((29, 255, 107), (254, 0, 0)),
                        ((255, 255, 255), (255, 121, 255)), ((0, 0, 0), (0, 136, 0))],
    ("bt709", "full"): [((0, 128, 128), (0, 0, 0)), ((255, 128, 128), (255, 255, 255)),
                        ((54, 99, 255), (0, 0, 254)), ((182, 30, 12), (0, 255, 0)), ((18, 255, 116), (254, 0, 0)),
                        ((255, 255, 255), (255, 172, 255)), ((0, 0, 0), (0, 84, 0))],
}


@pytest.mark.parametrize("matrix,range_", N.VARIANTS)
def test_hand_computed_triples(matrix, range_):
    """black, white, the primaries, and clipping at both ends"""
    for (y, u, v), bgr in HAND[(matrix, range_)]:
        assert _one(y, u, v, matrix, range_) == bgr, (matrix, range_, (y, u, v))


def test_formula_spelled_out():
    """one triple through the formula as the issue writes it, by plain Python integers"""
    yoff, yk, rv, gu, gv, bu = N.coefficients("bt709", "limited")
    y, u, v = 100, 90, 200
    c, d, e = y - yoff, u - 128, v - 128
    clip8 = lambda t: max(0, min(255, t))  # noqa: E731
    want = (clip8((yk * c + bu * d + 128) >> 8), clip8((yk * c - gu * d - gv * e + 128) >> 8), clip8((yk * c + rv * e + 128) >> 8))
    assert _one(y, u, v, "bt709", "limited") == want == (17, 68, 227)


@pytest.mark.parametrize("h,w", [(1, 1), (2, 2), (3, 5), (6, 8), (7, 9)])
def test_nv12_equals_i420_and_odd_sizes_pick_the_floor_sample(h, w):
    rng = np.random.default_rng(h * 100 + w)
    ch, cw = N.chroma_shape(h, w)
    assert (ch, cw) == (-(-h // 2), -(-w // 2))
    y = rng.integers(0, 256, (h, w), dtype=np.uint8)
    u, v = rng.integers(0, 256, (ch, cw), dtype=np.uint8), rng.integers(0, 256, (ch, cw), dtype=np.uint8)
    for matrix, range_ in N.VARIANTS:
        a = N.to_bgr((y, np.stack([u, v], axis=-1)), "nv12", matrix, range_)
        b = N.to_bgr((y, u, v), "i420", matrix, range_)
        assert a.shape == (h, w, 3) and a.dtype == np.uint8 and np.array_equal(a, b)
        for yy in range(h):
            for xx in range(w):
                assert tuple(a[yy, xx]) == _one(y[yy, xx], u[yy >> 1, xx >> 1], v[yy >> 1, xx >> 1], matrix, range_)


def test_packed_formats():
    rng = np.random.default_rng(5)
    a3, a4 = rng.integers(0, 256, (3, 5, 3), dtype=np.uint8), rng.integers(0, 256, (3, 5, 4), dtype=np.uint8)
    assert np.array_equal(N.to_bgr(a3, "bgr"), a3) and np.array_equal(N.to_bgr(a3, "rgb"), a3[..., ::-1])
    assert np.array_equal(N.to_bgr(a4, "bgra"), a4[..., :3]) and np.array_equal(N.to_bgr(a4, "rgba"), a4[..., 2::-1])
    assert np.array_equal(N.to_bgr(a3[..., 0], "gray"), a3[..., 0])
    for a in (a3, a4, a4[..., :2], a3[..., 0], a3.astype(np.int16), a4.astype(np.float32)):
        out = N.to_bgr(a, None)
        assert out.dtype == a.dtype and np.array_equal(out, a) and out is not a
    for bad, fmt in ((a4, "bgr"), (a3, "rgba"), (a3, "gray"), (a3.astype(np.int16), "bgr"), (a3.astype(np.float64), None)):
        with pytest.raises(ValueError):
            N.to_bgr(bad, fmt)
    with pytest.raises(ValueError):
        N.to_bgr((a3[..., 0], a3[..., 0]), "nv12")  # the UV plane has the ceiling size and two channels
    with pytest.raises(ValueError):
        N.to_bgr((a3[..., 0],), "i420")
