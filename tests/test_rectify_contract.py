"""The contract of lens rectification on the host: tests/numpy_rectify.py against hand-written expectations, its derived quantisation
bound, `stitching_amd.LensMap` against it (nodes, error(), both fits, map extrapolation), and the sensitivity of these inputs to subtly
wrong variants.  No device and no library.

The lenses.  WIDE is a barrel lens in OpenCV's sign convention (k1 < 0), FISH a Kannala-Brandt one: both pull the rectified frame's
pixels TOWARDS the source's centre, so with fit="same" every pixel of theirs samples inside the source, and fit="inside" widens the
view (a focal factor below 1).  Wedges in the corners of fit="same" need the other sign: PINCUSHION (k1 > 0) pushes the rectified
corners outside the source, and fit="inside" narrows the view (a factor above 1) until they are gone.  The test that tells the two
fits apart therefore uses PINCUSHION for the wedges, and checks "inside" on all three."""
import numpy as np
import pytest

import stitching_amd as S
from tests import numpy_rectify as N

SRC = (96, 72)
K = np.array([[70.0, 0.0, 47.3], [0.0, 70.0, 35.6], [0.0, 0.0, 1.0]])
WIDE = (-0.25, 0.06, 0.001, -0.0008, -0.01)
RATIONAL = (-0.2, 0.05, 0.0005, 0.0007, 0.01, 0.02, -0.01, 0.003)
PINCUSHION = (0.25, 0.05, 0.0, 0.0)
FISH = (-0.03, 0.01, -0.004, 0.001)


def image(size, c=3, seed=3):
    w, h = size
    return np.random.default_rng(seed).integers(0, 256, (h, w) if c == 1 else (h, w, c), dtype=np.uint8)


def shift_maps(size, dx=0.0, dy=0.0):
    w, h = size
    x, y = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    return x + dx, y + dy


# ---- per pixel, against expectations written by hand --------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(37, 21), (16, 16), (33, 1), (1, 33)])
@pytest.mark.parametrize("c", [1, 3])
def test_identity_is_a_copy(size, c):
    src = image(size, c)
    lens = S.LensMap.from_maps(*shift_maps(size), size)
    assert np.array_equal(lens.nodes, N.maps_nodes(*shift_maps(size)))
    w, h = size
    want_mask = np.zeros((h, w), np.uint8)
    want_mask[:h - 1, :w - 1] = 255  # the taps (x + 1, y + 1) of the last column and row lie outside, with weight 0
    for border in N.BORDERS:
        out, mask = N.rectify(src, lens.nodes, size, border)
        assert np.array_equal(out, src), border
        assert np.array_equal(mask, want_mask), border


def test_half_pixel_shift():
    size = (21, 5)
    src = image(size, 1).astype(np.int32)
    nodes = N.maps_nodes(*shift_maps(size, dx=0.5))
    out, mask = N.rectify(src.astype(np.uint8), nodes, size, "constant")
    want = np.empty_like(src)
    want[:, :-1] = (src[:, :-1] + src[:, 1:] + 1) >> 1  # (512 a + 512 b + 512) >> 10
    want[:, -1] = (src[:, -1] + 0 + 1) >> 1              # the right tap lies outside: 0
    assert np.array_equal(out, want.astype(np.uint8))
    assert np.all(mask[:-1, :-1] == 255) and np.all(mask[:, -1] == 0) and np.all(mask[-1, :] == 0)
    rep, _ = N.rectify(src.astype(np.uint8), nodes, size, "replicate")
    want[:, -1] = src[:, -1]
    assert np.array_equal(rep, want.astype(np.uint8))


def test_negative_coordinates_floor():
    """x - 0.5 is q = -16 at x = 0: ix = -1, fx = 16 by the arithmetic shift (truncation would give ix = 0, fx = -16)"""
    size = (21, 5)
    src = image(size, 1).astype(np.int32)
    nodes = N.maps_nodes(*shift_maps(size, dx=-0.5))
    q = N.interpolate(nodes, size)
    assert np.all(q[:, 0, 0] == -16) and np.all(q[:, 0, 0] >> 5 == -1) and np.all(q[:, 0, 0] & 31 == 16)
    out, mask = N.rectify(src.astype(np.uint8), nodes, size, "constant")
    want = np.empty_like(src)
    want[:, 1:] = (src[:, :-1] + src[:, 1:] + 1) >> 1
    want[:, 0] = (0 + src[:, 0] + 1) >> 1
    assert np.array_equal(out, want.astype(np.uint8))
    assert np.all(mask[:, 0] == 0) and np.all(mask[:-1, 1:] == 255)
    rep, _ = N.rectify(src.astype(np.uint8), nodes, size, "replicate")
    want[:, 0] = src[:, 0]
    assert np.array_equal(rep, want.astype(np.uint8))


def test_wholly_outside():
    size = (20, 18)
    src = image(size, 3)
    for dx, dy, edge in ((-500.0, 0.0, src[:, :1]), (0.0, 900.0, src[-1:, :])):
        nodes = N.maps_nodes(*shift_maps(size, dx, dy))
        out, mask = N.rectify(src, nodes, size, "constant")
        assert not out.any() and not mask.any()
        rep, mask = N.rectify(src, nodes, size, "replicate")
        assert np.array_equal(rep, np.broadcast_to(edge, src.shape)) and not mask.any()


def test_coordinates_at_the_clip_limits():
    size = (17, 17)
    assert np.all(N.quantise(np.full((3, 3), -1e9), np.full((3, 3), 1e9)) == [N.Q6_MIN, N.Q6_MAX])
    with pytest.raises(ValueError, match="finite"):
        N.quantise(np.full((3, 3), np.nan), np.zeros((3, 3)))
    nodes = np.empty((3, 3, 2), np.int32)
    nodes[..., 0], nodes[..., 1] = N.Q6_MIN, N.Q6_MAX
    q = N.interpolate(nodes, size)  # S = 256 N: no overflow at the limits
    assert np.all(q[..., 0] == N.Q6_MIN // 2) and np.all(q[..., 1] == N.Q6_MAX // 2)
    src = image((9, 7), 1)
    rep, mask = N.rectify(src, nodes, size, "replicate")
    assert np.all(rep == src[-1, 0]) and not mask.any()


# ---- the grid ----------------------------------------------------------------------------------------------------------------------
LENSES = {
    "brown": (lambda **kw: S.LensMap.brown(K, WIDE, SRC, **kw), lambda nk, u, v: N.brown_source(K, WIDE, nk, u, v),
              lambda nk, d: N.brown_nodes(K, WIDE, nk, d)),
    "rational": (lambda **kw: S.LensMap.brown(K, RATIONAL, SRC, **kw), lambda nk, u, v: N.brown_source(K, RATIONAL, nk, u, v),
                 lambda nk, d: N.brown_nodes(K, RATIONAL, nk, d)),
    "fisheye": (lambda **kw: S.LensMap.fisheye(K, FISH, SRC, **kw), lambda nk, u, v: N.fisheye_source(K, FISH, nk, u, v),
                lambda nk, d: N.fisheye_nodes(K, FISH, nk, d)),
}


@pytest.mark.parametrize("name", list(LENSES))
@pytest.mark.parametrize("dst", [None, (70, 37)])
def test_nodes_bound_and_error(name, dst):
    make, source, make_nodes = LENSES[name]
    lens = make(dst_size=dst)
    w, h = size = lens.dst_size
    assert size == (dst or SRC) and lens.src_size == SRC
    assert lens.nodes.dtype == np.int32 and lens.nodes.shape == N.node_counts(w, h)[::-1] + (2,)
    assert np.array_equal(lens.nodes, make_nodes(lens.new_K, size))
    q = N.interpolate(lens.nodes, size)
    assert np.array_equal(lens.coordinates(), q)
    # the derived bound against the bilinear interpolation of the unrounded nodes
    sx, sy = source(lens.new_K, *N.node_pixels(w, h))
    b = N.float_bilinear(sx, sy, size)
    worst = np.abs(q / 32.0 - b).max()
    print(f"{name} {size}: |q/32 - B| max {worst:.6f} (bound {N.QUANTISATION_BOUND:.6f})")
    assert worst <= N.QUANTISATION_BOUND
    # error(): a dense recomputation against the exact model
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    ex, ey = source(lens.new_K, u, v)
    dense = np.hypot(q[..., 0] / 32.0 - ex, q[..., 1] / 32.0 - ey).max()
    print(f"{name} {size}: error() {lens.error():.6f}")
    assert lens.error() == pytest.approx(dense, abs=1e-9)
    assert lens.error() >= 0.0


def test_same_keeps_the_camera():
    lens = S.LensMap.brown(K, WIDE, SRC)
    assert np.array_equal(lens.new_K, K) and lens.dst_size == SRC
    nk = K * 1.5
    nk[2, 2] = 1.0
    assert np.array_equal(S.LensMap.brown(K, WIDE, SRC, new_K=nk).new_K, nk)


def mask_of(lens):
    return N.rectify(image(lens.src_size, 1), lens.nodes, lens.dst_size, "constant")[1]


@pytest.mark.parametrize("name,make,source,wider", [
    ("wide", lambda **kw: S.LensMap.brown(K, WIDE, SRC, **kw), lambda nk, u, v: N.brown_source(K, WIDE, nk, u, v), True),
    ("fisheye", lambda **kw: S.LensMap.fisheye(K, FISH, SRC, **kw), lambda nk, u, v: N.fisheye_source(K, FISH, nk, u, v), True),
    ("pincushion", lambda **kw: S.LensMap.brown(K, PINCUSHION, SRC, **kw), lambda nk, u, v: N.brown_source(K, PINCUSHION, nk, u, v), False),
    ("wide-resized", lambda **kw: S.LensMap.brown(K, WIDE, SRC, dst_size=(70, 37), **kw),
     lambda nk, u, v: N.brown_source(K, WIDE, nk, u, v), None),
])
def test_fit_inside_samples_inside_everywhere(name, make, source, wider):
    inside, same = make(fit="inside"), make(fit="same")
    assert np.all(mask_of(inside) == 255)
    factor = inside.new_K[0, 0] / same.new_K[0, 0]
    assert inside.new_K[1, 1] / same.new_K[1, 1] == pytest.approx(factor)
    assert np.array_equal(inside.new_K[:, 2], same.new_K[:, 2])
    if wider is not None:
        assert (factor < 1.0) == wider, factor
    # the widest such view: by the exact model, the border pixel nearest to an edge of the source lies the margin of one pixel inside it
    w, h = inside.dst_size
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    edge = np.ones((h, w), bool)
    edge[1:-1, 1:-1] = False
    sx, sy = source(inside.new_K, u[edge], v[edge])
    nearest = min(sx.min(), sy.min(), (SRC[0] - 1 - sx).min(), (SRC[1] - 1 - sy).min())
    print(f"{name}: focal factor {factor:.4f}, nearest border coordinate {nearest:.6f} px inside")
    assert 1.0 <= nearest < 1.0 + 1e-6


def test_fit_same_leaves_wedges_in_the_corners():
    """what tells the fits apart: the same lens, "same" has zeros in all four corners (and none in the middle), "inside" has none"""
    same = mask_of(S.LensMap.brown(K, PINCUSHION, SRC, fit="same"))
    h, w = same.shape
    assert same[0, 0] == 0 and same[0, w - 1] == 0 and same[h - 1, 0] == 0 and same[h - 1, w - 1] == 0
    assert np.all(same[h // 4:3 * h // 4, w // 4:3 * w // 4] == 255)
    assert np.all(mask_of(S.LensMap.brown(K, PINCUSHION, SRC, fit="inside")) == 255)
    assert np.all(mask_of(S.LensMap.brown(K, WIDE, SRC, fit="same")) == 255)  # a barrel lens samples inwards: see the module's docstring


@pytest.mark.parametrize("size", [(37, 21), (32, 16), (17, 2), (2, 17)])
def test_from_maps_extrapolates_a_linear_map_exactly(size):
    w, h = size
    x, y = shift_maps(size)
    mx, my = 0.75 * x - 0.125 * y + 3.5, 0.25 * x + 1.5 * y - 7.25  # exact in Q6 at every integer pixel
    lens = S.LensMap.from_maps(mx, my, (64, 64))
    nx, ny = N.node_counts(w, h)
    cx, cy = np.meshgrid(np.arange(nx) * 16.0, np.arange(ny) * 16.0)
    want = np.stack([0.75 * cx - 0.125 * cy + 3.5, 0.25 * cx + 1.5 * cy - 7.25], axis=-1) * 64.0
    assert (nx - 1) * 16 >= w and (ny - 1) * 16 >= h  # nodes past both edges
    assert np.array_equal(lens.nodes, want.astype(np.int32)) and np.array_equal(lens.nodes, N.maps_nodes(mx, my))
    assert lens.error() == 0.0 and lens.new_K is None and lens.dst_size == size and lens.src_size == (64, 64)


@pytest.mark.parametrize("size", [(1, 1), (1, 19), (19, 1)])
def test_single_columns_and_rows(size):
    w, h = size
    mx, my = shift_maps(size, 2.25, 3.5)
    lens = S.LensMap.from_maps(mx, my, (30, 30))
    assert lens.nodes.shape == N.node_counts(w, h)[::-1] + (2,)
    if w == 1:
        assert np.array_equal(lens.nodes[:, 0], lens.nodes[:, 1])  # the last column is repeated
    if h == 1:
        assert np.array_equal(lens.nodes[0], lens.nodes[1])
    src = image((30, 30), 3)
    out, mask = N.rectify(src, lens.nodes, size, "constant")
    x, y = (mx + 0.0).astype(int), (my + 0.0).astype(int)
    a, b, c, d = (src[y, x].astype(np.int32), src[y, x + 1].astype(np.int32), src[y + 1, x].astype(np.int32),
                  src[y + 1, x + 1].astype(np.int32))
    assert np.array_equal(out, ((24 * 16 * a + 8 * 16 * b + 24 * 16 * c + 8 * 16 * d + 512) >> 10).astype(np.uint8))
    assert np.all(mask == 255)
    brown = S.LensMap.brown(K, WIDE, SRC, dst_size=size)
    assert brown.nodes.shape == lens.nodes.shape and brown.error() >= 0.0


# ---- sensitivity: subtly wrong variants differ on these inputs ---------------------------------------------------------------------
def variant(src, nodes, dst_size, truncate=False, short_weights=False):
    """the contract for u8x1 and border "constant", with one thing wrong"""
    w, h = dst_size
    sh, sw = src.shape
    y, x = np.arange(h, dtype=np.int64)[:, None, None], np.arange(w, dtype=np.int64)[None, :, None]
    ax, ay, i, j = x & 15, y & 15, (x >> 4)[..., 0], (y >> 4)[..., 0]
    n = nodes.astype(np.int64)
    s = (16 - ay) * ((16 - ax) * n[j, i] + ax * n[j, i + 1]) + ay * ((16 - ax) * n[j + 1, i] + ax * n[j + 1, i + 1]) + 256
    if truncate:  # C's division and remainder instead of shift and mask
        q = np.trunc(s / 512.0).astype(np.int64)
        ii, ff = np.trunc(q / 32.0).astype(np.int64), np.fmod(q, 32)
    else:
        q = s >> 9
        ii, ff = q >> 5, q & 31
    fx, fy, ix, iy = ff[..., 0], ff[..., 1], ii[..., 0], ii[..., 1]
    acc = np.full((h, w), 512, np.int64)
    w00 = (32 - fx) * (32 - fy) - (1 if short_weights else 0)
    for dx, dy, wgt in ((0, 0, w00), (1, 0, fx * (32 - fy)), (0, 1, (32 - fx) * fy), (1, 1, fx * fy)):
        tx, ty = ix + dx, iy + dy
        inside = (tx >= 0) & (tx < sw) & (ty >= 0) & (ty < sh)
        acc += wgt * np.where(inside, src[np.clip(ty, 0, sh - 1), np.clip(tx, 0, sw - 1)].astype(np.int64), 0)
    return np.clip(acc >> 10, 0, 255).astype(np.uint8)


def test_subtly_wrong_variants_differ():
    size = (37, 21)
    src = image(size, 1)
    shifted = N.maps_nodes(*shift_maps(size, dx=-0.5, dy=-0.25))
    lens = S.LensMap.brown(K, WIDE, SRC)
    big = image(SRC, 1)
    # the variant function itself restates the contract
    assert np.array_equal(variant(src, shifted, size), N.rectify(src, shifted, size)[0])
    assert np.array_equal(variant(big, lens.nodes, SRC), N.rectify(big, lens.nodes, SRC)[0])
    # truncation instead of floor: the first column and row, where coordinates are negative
    trunc = variant(src, shifted, size, truncate=True)
    assert not np.array_equal(trunc, N.rectify(src, shifted, size)[0])
    assert np.array_equal(trunc[1:, 1:], N.rectify(src, shifted, size)[0][1:, 1:])
    # weights that sum to 1023: half a pixel to the right is (512 a + 512 b + 512) >> 10, a whole number before the shift wherever
    # a + b is odd, and one weight unit less of a > 0 then falls below it
    half = N.maps_nodes(*shift_maps(size, dx=0.5))
    short, right = variant(src, half, size, short_weights=True), N.rectify(src, half, size)[0]
    odd = ((src[:, :-1].astype(int) + src[:, 1:]) & 1 == 1) & (src[:, :-1] > 0)
    assert odd.any() and np.array_equal(short[:, :-1][odd], right[:, :-1][odd] - 1)
    # nodes taken at 16 i + 8 instead of 16 i
    w, h = SRC
    nx, ny = N.node_counts(w, h)
    u, v = np.meshgrid(np.arange(nx) * 16.0 + 8.0, np.arange(ny) * 16.0 + 8.0)
    off = N.quantise(*N.brown_source(K, WIDE, K, u, v))
    assert not np.array_equal(N.rectify(big, off, SRC)[0], N.rectify(big, lens.nodes, SRC)[0])
