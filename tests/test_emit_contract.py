"""The contract of device frame emit (tests/numpy_emit.py) checked against itself: the table against the rule that makes it, the
distance from the float64 matrix and the value ranges over all 2^24 (B, G, R) triples, the round trip through numpy_ingest, block
chroma, odd sizes, packed formats.  No GPU."""
import numpy as np
import pytest

from tests import numpy_emit as E
from tests import numpy_ingest as N


def test_the_table_equals_the_rule_and_rows_sum_as_stated():
    assert set(E.VARIANTS) == set(N.VARIANTS)
    for matrix, range_ in E.VARIANTS:
        ky, ku, kv = E.COEFFICIENTS[(matrix, range_)]
        assert E.derive_coefficients(matrix, range_) == (ky, ku, kv), (matrix, range_)
        assert sum(ky) == (65536 if range_ == "full" else 56284) and sum(ku) == 0 and sum(kv) == 0
        assert max(abs(k) for row in (ky, ku, kv) for k in row) < 1 << 16  # so a block's sum of products stays below 2^31
        assert all(0.0 < d <= 0.0051 for d in E.coefficient_error(matrix, range_))
    assert E.LUMA_ROW_SUM["limited"] == int(np.rint(65536.0 * 219.0 / 255.0))
    # the forward matrix is the inverse of the one ingest rounds: its real coefficients undo it
    for matrix, range_ in E.VARIANTS:
        ys, rv, gu, gv, bu = N.real_coefficients(matrix, range_)
        back = np.array([[ys, bu, 0.0], [ys, -gu, -gv], [ys, 0.0, rv]])  # rows B, G, R; columns Y - yoff, U - 128, V - 128
        assert np.allclose(back @ E.real_matrix(matrix, range_), np.eye(3), atol=1e-12)
    with pytest.raises(ValueError):
        E.coefficients("bt2020", "limited")


@pytest.mark.parametrize("matrix,range_", E.VARIANTS)
def test_every_triple(matrix, range_):
    """over all 2^24 uniform (B, G, R): |Y - exact| and the chroma of uniform blocks within 1/2 + delta, the value ranges, grey without
    colour, and the round trip through numpy_ingest.to_bgr within 2 levels"""
    limited = range_ == "limited"
    bound = E.bound_exact(matrix, range_)
    g, r = np.arange(256)[None, :, None], np.arange(256)[None, None, :]
    worst = np.zeros(3)
    lo, hi = np.full(3, 255), np.zeros(3, np.int64)
    trip = np.zeros(3, np.int64)
    for b0 in range(0, 256, 32):
        b = np.arange(b0, b0 + 32)[:, None, None]
        y = E.luma(b, g, r, matrix, range_)
        u, v = E.chroma(4 * b, 4 * g, 4 * r, matrix, range_)  # a uniform block's sums
        got = np.stack(np.broadcast_arrays(y, u, v), axis=-1)
        worst = np.maximum(worst, np.abs(got - E.exact_yuv(b, g, r, matrix, range_)).reshape(-1, 3).max(axis=0))
        lo, hi = np.minimum(lo, got.reshape(-1, 3).min(axis=0)), np.maximum(hi, got.reshape(-1, 3).max(axis=0))
        back = N.yuv_to_bgr(y, u, v, matrix, range_).astype(np.int64)
        want = np.stack(np.broadcast_arrays(b, g, r), axis=-1)
        trip = np.maximum(trip, np.abs(back - want).reshape(-1, 3).max(axis=0))
    print(f"{matrix} {range_}: worst |int - exact| (Y, U, V) {worst.round(4)} (bounds {np.round(bound, 4)}), ranges {lo} .. {hi}, "
          f"round trip (B, G, R) {trip}")
    assert all(worst[k] <= bound[k] + 1e-9 for k in range(3))
    assert worst.max() <= 0.5022 + 1e-4
    assert tuple(lo) == ((16, 16, 16) if limited else (0, 1, 1)) and tuple(hi) == ((235, 240, 240) if limited else (255, 255, 255))
    assert trip.max() <= 2
    grey = np.arange(256)
    u, v = E.chroma(4 * grey, 4 * grey, 4 * grey, matrix, range_)
    assert np.all(u == 128) and np.all(v == 128)
    assert int(E.luma(255, 255, 255, matrix, range_)) == (235 if limited else 255)
    assert int(E.luma(0, 0, 0, matrix, range_)) == (16 if limited else 0)


def test_only_full_range_chroma_clips():
    for matrix, range_ in E.VARIANTS:
        _, ku, kv = E.coefficients(matrix, range_)
        for k in (ku, kv):  # the extremes of a linear form lie at the corners of the cube
            corners = [((k[0] * sb + k[1] * sg + k[2] * sr + 131072) >> 18) + 128 for sb in (0, 1020) for sg in (0, 1020) for sr in (0, 1020)]
            assert (min(corners), max(corners)) == ((16, 240) if range_ == "limited" else (1, 256))
    assert tuple(int(c[0]) for c in E.chroma([1020], [0], [0], "bt709", "full")) == (255, 116)


@pytest.mark.parametrize("matrix,range_", E.VARIANTS)
def test_block_chroma_is_within_the_bound_of_the_float_average(matrix, range_):
    rng = np.random.default_rng(31)
    blocks = rng.integers(0, 256, (200000, 2, 2, 3), dtype=np.uint8)
    blocks[:1000, :, 1] = blocks[:1000, :, 0]  # some with equal columns, as an odd width makes them
    s = blocks.astype(np.int32).sum(axis=(1, 2))
    u, v = E.chroma(s[:, 0], s[:, 1], s[:, 2], matrix, range_)
    mean = blocks.astype(np.float64).mean(axis=(1, 2))
    ref = E.exact_yuv(mean[:, 0], mean[:, 1], mean[:, 2], matrix, range_)
    bound = E.bound_exact(matrix, range_)
    assert np.abs(u - ref[:, 1]).max() <= bound[1] + 1e-9 and np.abs(v - ref[:, 2]).max() <= bound[2] + 1e-9


def test_formula_spelled_out():
    """one pixel and one block through the formulas as the issue writes them, by plain Python integers"""
    (kyb, kyg, kyr), (kub, kug, kur), (kvb, kvg, kvr) = E.coefficients("bt709", "limited")
    clip8 = lambda t: max(0, min(255, t))  # noqa: E731
    block = np.array([[[10, 200, 30], [250, 0, 7]], [[99, 98, 97], [0, 255, 255]]], np.uint8)
    y, uv = E.from_bgr(block, "nv12")
    for yy in range(2):
        for xx in range(2):
            b, g, r = (int(c) for c in block[yy, xx])
            assert int(y[yy, xx]) == clip8(((kyb * b + kyg * g + kyr * r + 32768) >> 16) + 16)
    sb, sg, sr = (int(c) for c in block.astype(int).sum(axis=(0, 1)))
    assert (sb, sg, sr) == (359, 553, 389)
    assert int(uv[0, 0, 0]) == clip8(((kub * sb + kug * sg + kur * sr + 131072) >> 18) + 128)
    assert int(uv[0, 0, 1]) == clip8(((kvb * sb + kvg * sg + kvr * sr + 131072) >> 18) + 128)


@pytest.mark.parametrize("h,w", [(1, 1), (2, 2), (1, 9), (7, 1), (3, 5), (6, 8), (7, 9)])
def test_odd_sizes_replicate_the_edge(h, w):
    """the clamped sums equal an independent formulation: pad by edge replication to even sizes, then reshape and sum"""
    rng = np.random.default_rng(h * 100 + w)
    a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    ch, cw = N.chroma_shape(h, w)
    padded = np.pad(a, ((0, 2 * ch - h), (0, 2 * cw - w), (0, 0)), mode="edge").astype(np.int32)
    want = padded.reshape(ch, 2, cw, 2, 3).sum(axis=(1, 3))
    assert np.array_equal(E.block_sums(a), want)
    for matrix, range_ in E.VARIANTS:
        y, uv = E.from_bgr(a, "nv12", matrix, range_)
        y2, u, v = E.from_bgr(a, "i420", matrix, range_)
        assert y.shape == (h, w) and uv.shape == (ch, cw, 2) and u.shape == v.shape == (ch, cw)
        assert np.array_equal(y, y2) and np.array_equal(uv[..., 0], u) and np.array_equal(uv[..., 1], v)
        wu, wv = E.chroma(want[..., 0], want[..., 1], want[..., 2], matrix, range_)
        assert np.array_equal(u, wu) and np.array_equal(v, wv)
        assert N.to_bgr(E.from_bgr(a, "nv12", matrix, range_), "nv12", matrix, range_).shape == a.shape  # the shapes to_bgr takes
        assert N.to_bgr((y2, u, v), "i420", matrix, range_).shape == a.shape


def test_packed_formats():
    rng = np.random.default_rng(5)
    a3, m = rng.integers(0, 256, (3, 5, 3), dtype=np.uint8), rng.integers(0, 256, (3, 5), dtype=np.uint8)
    assert np.array_equal(E.from_bgr(a3, "bgr"), a3) and np.array_equal(E.from_bgr(a3, "rgb"), a3[..., ::-1])
    assert np.array_equal(E.from_bgr(m, "gray"), m)
    for fmt, colour in (("bgra", a3), ("rgba", a3[..., ::-1])):
        out = E.from_bgr(a3, fmt)
        assert out.shape == (3, 5, 4) and np.array_equal(out[..., :3], colour) and np.all(out[..., 3] == 255)
        out = E.from_bgr(a3, fmt, alpha=m)
        assert np.array_equal(out[..., :3], colour) and np.array_equal(out[..., 3], m)
        assert np.array_equal(N.to_bgr(out, fmt), a3)  # packed formats come back exactly
    a4 = rng.integers(0, 256, (3, 5, 4), dtype=np.uint8)
    for a in (a3, a4, a4[..., :2], m, a3.astype(np.int16), a4.astype(np.float32)):
        out = E.from_bgr(a, None)
        assert out.dtype == a.dtype and np.array_equal(out, a) and out is not a
    for bad, fmt in ((a4, "bgr"), (m, "rgba"), (a3, "gray"), (a3.astype(np.int16), "nv12"), (a3.astype(np.float64), None), (a3, "yuyv")):
        with pytest.raises(ValueError):
            E.from_bgr(bad, fmt)
    with pytest.raises(ValueError):
        E.from_bgr(a3, "bgr", alpha=m)
    with pytest.raises(ValueError):
        E.from_bgr(a3, "bgra", alpha=m[:2])
