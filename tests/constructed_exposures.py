"""Constructed inputs for the exposure compensators: the overlap statistics, the plan and the filter of the estimation
(csrc/stx_exposure.hip, exp_plan and filter_map of csrc/stx_exposure_host.cpp) and the gains multiplied into the images
(csrc/stx_gain.hip, csrc/stx_gain_host.cpp).  Every family is built to reach one path of those that warped synthetic frames, warped
masks and random fp32 gains never reach, and returns the facts that make it reach it.  Pure numpy, no GPU and no product code:
tests/test_constructed_exposures.py asserts the facts against the CPU contracts (tests/numpy_exposure.py, the oracle's gain_apply /
block_gain_apply / resize_linear_f32) and shows that each family tells the contract from a one-mistake variant of it;
tests/test_gpu_constructed_exposures.py runs the same inputs on the device.

Estimation families return a Scene: corners, images, masks, the block size and `facts`, a dict of what the construction promises,
stated from the construction alone.  Where offsets matter the pixels are position coded in the image's OWN coordinates (coded_image):
B = (x + salt) mod 251, G = (y + 2 salt) mod 241, R = (7 x + 13 y + salt) mod 256, so the integer sums over a rectangle follow from its
coordinates (coded_sums) and an off-by-one in either image's read offset changes them.  Apply families return images, gain maps and
facts; interp_gains restates cv::resize(INTER_LINEAR) for CV_32F operation by operation in fp32, so a builder can prove what gain
reaches a pixel.

Not covered: the fallback of stx_block_gain_apply_batch for interpolated rows above 64 MiB (gh x w floats per image) — an input of that
size is too large for a test.  A device view shares its parent's row pitch, which is a multiple of 64 bytes for every buffer of the
library's own, so an odd pitch cannot be built through the public surface: the views here start on odd columns (3, 6, 9 bytes past a
dword)."""
import numpy as np

# Constants of the kernels the families are shaped around.  tests/test_constructed_exposures.py reads each of them back from the
# sources: a moved constant fails that test instead of letting the families quietly miss their edges.
EXP_WG = 256                      # exposure_stats_kernel: lanes of a workgroup = pixels of a chunk; exposure_block_mul_kernel likewise
BLOCK_MUL_GRID = 64               # stx_launch_exposure_block_mul: at most 64 workgroups per image, a grid-stride loop above 64 * 256 pixels
GAIN_BATCH = 16                   # images per launch of gain_rows_kernel / block_gain4_kernel
PIXEL_GROUP = 4                   # pixels per lane of gain_apply_kernel and block_gain4_kernel (12 bytes = 3 dwords)
GAIN4_ROWS = 16                   # rows per workgroup of block_gain4_kernel (4 wavefronts x 4 rows)
GAIN_ROWS_WG = 256                # gain_rows_kernel: columns, or rows of the row table, per workgroup
EXP_SQRT_N = 3 * 255 * 255 + 1    # entries of the sqrt table: the last one is a white pixel's
BOUNDED_BELOW = 8.0e6             # exposure_error_compensator._gain_map: a map is "bounded" when every |g| is finite and below this
INT_EDGE = 2.0 ** 31 / 255.0      # 8421504.50196...: from here on 255 g leaves the int range.  fp32 has spacing 1 above 2^23, so the
INT_EDGE_F32 = np.float32(8421504.5)  # literal 8421504.5f is 8421504 (ties to even): 255 x 8421504 = 2^31 - 128, the largest fp32 below
#                                   2^31, rounds to itself and saturates to 255; 255 x 8421505 rounds to 2^31 in fp32 -> INT_MIN -> 0

JOB_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025)
LAYOUTS = ("row", "column", "square")
MASK_MODES = ("full", "first_chunk_off", "last_chunk_off")
KINDS = ("gain", "gain_blocks", "channel", "channel_blocks")


class Scene:
    def __init__(self, corners, imgs, masks, bl, facts):
        self.corners = [tuple(int(v) for v in c) for c in corners]
        self.imgs, self.masks, self.bl, self.facts = list(imgs), list(masks), int(bl), facts
        for a in self.imgs + self.masks:
            a.setflags(write=False)

    @property
    def sizes(self):
        return [(m.shape[1], m.shape[0]) for m in self.masks]


# ---------------------------------------------------------------------------------------------------------------------------------
# position-coded pixels
# ---------------------------------------------------------------------------------------------------------------------------------
def coded_channels(xs, ys, salt):
    xs, ys = np.asarray(xs, np.int64), np.asarray(ys, np.int64)
    return (xs + salt) % 251, (ys + 2 * salt) % 241, (7 * xs + 13 * ys + salt) % 256


def coded_image(w, h, salt):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack(coded_channels(xx, yy, salt), axis=2).astype(np.uint8)


def coded_sums(xs, ys, salt):
    """(B, G, R) sums of a coded image over the pixels (xs, ys) of its own coordinates: from the coordinates, not from an image"""
    return tuple(int(c.sum()) for c in coded_channels(xs, ys, salt))


def overlap_rect(corners, sizes, i, j):
    """(tx, ty, w, h) of the intersection of images i and j in panorama coordinates, or None"""
    (xi, yi), (xj, yj), (wi, hi), (wj, hj) = corners[i], corners[j], sizes[i], sizes[j]
    tx, ty, rx, ry = max(xi, xj), max(yi, yj), min(xi + wi, xj + wj), min(yi + hi, yj + hj)
    return (tx, ty, rx - tx, ry - ty) if tx < rx and ty < ry else None


def image_pair_facts(corners, masks, salts):
    """{(i, j): (c, (B, G, R) of i, (B, G, R) of j)} for every pair of coded images i <= j whose rectangles overlap, whole images as
    units: the count where both masks are 255 and the channel sums there, from coordinates"""
    sizes = [(m.shape[1], m.shape[0]) for m in masks]
    out = {}
    for i in range(len(masks)):
        for j in range(i, len(masks)):
            r = overlap_rect(corners, sizes, i, j)
            if r is None:
                continue
            tx, ty, w, h = r
            yy, xx = np.mgrid[ty:ty + h, tx:tx + w]
            (xi, yi), (xj, yj) = corners[i], corners[j]
            on = (masks[i][yy - yi, xx - xi] == 255) & (masks[j][yy - yj, xx - xj] == 255)
            out[(i, j)] = (int(on.sum()), coded_sums(xx[on] - xi, yy[on] - yi, salts[i]), coded_sums(xx[on] - xj, yy[on] - yj, salts[j]))
    return out


def _coded_scene(corners, sizes, bl, facts, masks=None, salts=None):
    salts = salts or [101 * k for k in range(len(sizes))]
    masks = masks or [np.full((h, w), 255, np.uint8) for w, h in sizes]
    imgs = [coded_image(w, h, s) for (w, h), s in zip(sizes, salts)]
    facts = dict(facts, salts=salts, pairs=image_pair_facts(corners, masks, salts))
    return Scene(corners, imgs, masks, bl, facts)


# ---------------------------------------------------------------------------------------------------------------------------------
# E1 job sizes
# ---------------------------------------------------------------------------------------------------------------------------------
def layout_of(n, layout):
    if layout == "row":
        return n, 1
    if layout == "column":
        return 1, n
    h = max(d for d in range(1, int(n ** 0.5) + 1) if n % d == 0)
    return n // h, h


def job_sizes(n, layout, mask_mode="full"):
    """two images whose overlap holds n pixels (w x h by `layout`): a at (0, 0), b at (2, 1).  mask_mode: "first_chunk_off": a's mask
    is 0 on the first 256 pixels of the overlap in the job's row-major order; "last_chunk_off": b's mask is 0 on the last, partial chunk
    (pixels 256 * ((n - 1) // 256) .. n - 1).  The block kinds run with bl = the largest side: one block per image."""
    w, h = layout_of(n, layout)
    sizes = [(w + 2, h + 1), (w + 1, h + 2)]
    corners = [(0, 0), (2, 1)]
    masks = [np.full((hh, ww), 255, np.uint8) for ww, hh in sizes]
    p = np.arange(n)
    off = p < EXP_WG if mask_mode == "first_chunk_off" else p >= EXP_WG * ((n - 1) // EXP_WG) if mask_mode == "last_chunk_off" else p < 0
    oy, ox = p[off] // w, p[off] % w
    if mask_mode == "first_chunk_off":
        masks[0][oy + 1, ox + 2] = 0
    else:
        masks[1][oy, ox] = 0
    facts = dict(n=n, w=w, h=h, c=n - int(off.sum()), offsets=((2, 1), (0, 0)), chunks=-(-n // EXP_WG), last_chunk=n - EXP_WG * ((n - 1) // EXP_WG))
    return _coded_scene(corners, sizes, max(w, h) + 2, facts, masks)


# ---------------------------------------------------------------------------------------------------------------------------------
# E2 placements
# ---------------------------------------------------------------------------------------------------------------------------------
PLACEMENTS = ("inside", "identical", "column", "row", "pixel", "touch_edge", "touch_corner", "negative")


def placements(which, bl=8):
    """a is 23 x 17 at (ax, ay).  facts: the overlap (w, h) or None, both images' read offsets into it.  Of two whole images one has
    the offset 0 on each axis (the overlap starts where the later one starts); the block kinds (bl = 8) add the blocks' own origins:
    "inside" (b 9 x 7 strictly inside a) pairs a's block at (8, 12) with b's at (5, 0): a is read at (9, 12), b at (5, 6)"""
    aw, ah = 23, 17
    ax, ay = (-1000, -37) if which == "negative" else (5, 3)
    bx, by, bw, bh = {"inside": (ax + 4, ay + 6, 9, 7), "identical": (ax, ay, aw, ah), "column": (ax + aw - 1, ay - 2, 11, 30),
                      "row": (ax - 3, ay + ah - 1, 40, 5), "pixel": (ax + aw - 1, ay + ah - 1, 6, 4), "touch_edge": (ax + aw, ay + 2, 9, 9),
                      "touch_corner": (ax + aw, ay + ah, 9, 9), "negative": (ax - 6, ay - 5, 19, 13)}[which]
    corners, sizes = [(ax, ay), (bx, by)], [(aw, ah), (bw, bh)]
    r = overlap_rect(corners, sizes, 0, 1)
    facts = dict(overlap=r and r[2:], offsets=r and ((r[0] - ax, r[1] - ay), (r[0] - bx, r[1] - by)), bl=bl)
    return _coded_scene(corners, sizes, bl, facts)


# ---------------------------------------------------------------------------------------------------------------------------------
# E3 block grids
# ---------------------------------------------------------------------------------------------------------------------------------
def axis_blocks(n, bl):
    """the blocks of one axis as BlocksCompensator::feed cuts it: ceil(n / bl) blocks of ceil(n / blocks) pixels, the last one shorter"""
    bp = -(-n // bl)
    bw = -(-n // bp)
    return [(k * bw, min(k * bw + bw, n)) for k in range(bp)], bw


def axis_pairs(n_a, off_a, n_b, off_b, bl):
    """(block of a, block of b) pairs of one axis whose intervals overlap"""
    a, _ = axis_blocks(n_a, bl)
    b, _ = axis_blocks(n_b, bl)
    return [(i, j) for i, (a0, a1) in enumerate(a) for j, (b0, b1) in enumerate(b) if max(a0 + off_a, b0 + off_b) < min(a1 + off_a, b1 + off_b)]


BLOCK_GRIDS = ("33_32", "50_8", "50_12", "bl1", "bl_large", "aligned", "off_by_one", "two_sizes")


def block_grids(which):
    """facts: per image (blocks per row, blocks per column, bw, bh); the number of unit pairs of different images (rectangles are
    products of intervals: pairs of the x axis times pairs of the y axis); how many blocks of b a block of a meets; cut_differs: cutting
    blocks of bl pixels would give other rectangles (an axis with several blocks whose size is not bl)"""
    corners, sizes, bl = {
        "33_32": ([(0, 0), (20, 7)], [(33, 20), (33, 20)], 32),        # bw = 17
        "50_8": ([(0, 0), (31, 3)], [(50, 9), (50, 9)], 8),            # 7 blocks of 8: the last 2 wide
        "50_12": ([(0, 0), (31, 3)], [(50, 13), (50, 13)], 12),        # 5 blocks of 10
        "bl1": ([(0, 0), (4, 2)], [(6, 5), (6, 5)], 1),                # every unit one pixel
        "bl_large": ([(0, 0), (11, 4)], [(20, 10), (20, 10)], 64),
        "aligned": ([(0, 0), (16, 8)], [(32, 24), (32, 24)], 8),       # the corner offset a multiple of both block sizes
        "off_by_one": ([(0, 0), (17, 9)], [(32, 24), (32, 24)], 8),
        "two_sizes": ([(0, 0), (13, 6)], [(33, 20), (50, 30)], 32),    # bw 17 and 25, bh 20 and 30
    }[which]
    px = axis_pairs(sizes[0][0], corners[0][0], sizes[1][0], corners[1][0], bl)
    py = axis_pairs(sizes[0][1], corners[0][1], sizes[1][1], corners[1][1], bl)
    grids = [(len(axis_blocks(w, bl)[0]), len(axis_blocks(h, bl)[0]), axis_blocks(w, bl)[1], axis_blocks(h, bl)[1]) for w, h in sizes]
    meets = {}
    for i, _ in px:
        for k, _ in py:
            meets[(i, k)] = sum(a == i for a, _ in px) * sum(a == k for a, _ in py)
    facts = dict(grids=grids, units=sum(g[0] * g[1] for g in grids), cross_pairs=len(px) * len(py), meets=meets, bl=bl,
                 cut_differs=any((g[0] > 1 and g[2] != bl) or (g[1] > 1 and g[3] != bl) for g in grids))
    return _coded_scene(corners, sizes, bl, facts)


# ---------------------------------------------------------------------------------------------------------------------------------
# E4 values
# ---------------------------------------------------------------------------------------------------------------------------------
VALUES = ("white", "black", "mask_levels", "disjoint_masks")
MASK_LEVELS = (0, 1, 127, 254, 255)


def values(which, bl=8):
    if which in ("white", "black"):
        v = 255 if which == "white" else 0
        corners, sizes = [(0, 0), (7, 5)], [(19, 14), (21, 12)]
        imgs = [np.full((h, w, 3), v, np.uint8) for w, h in sizes]
        masks = [np.full((h, w), 255, np.uint8) for w, h in sizes]
        r = overlap_rect(corners, sizes, 0, 1)
        return Scene(corners, imgs, masks, bl, dict(c=r[2] * r[3], table_index=3 * v * v, norm=float(np.sqrt(np.float64(3 * v * v)))))
    if which == "mask_levels":
        rng = np.random.default_rng(4)
        corners, sizes = [(0, 0), (6, 3)], [(40, 21), (37, 25)]
        masks = [rng.choice(np.array(MASK_LEVELS, np.uint8), size=(h, w)) for w, h in sizes]
        s = _coded_scene(corners, sizes, bl, dict(levels=MASK_LEVELS), masks)
        tx, ty, w, h = overlap_rect(corners, sizes, 0, 1)
        ma, mb = masks[0][ty:ty + h, tx:tx + w], masks[1][ty - 3:ty - 3 + h, tx - 6:tx - 6 + w]
        s.facts["c"] = int(((ma == 255) & (mb == 255)).sum())
        s.facts["c_if_254_counts"] = int(((ma >= 254) & (mb >= 254)).sum())
        s.facts["c_if_nonzero_counts"] = int(((ma > 0) & (mb > 0)).sum())
        return s
    # three images: a and b overlap in x 10 .. 19 where a's mask is 0; c lies under both and meets each where its mask is 255
    corners, sizes = [(0, 0), (10, 0), (0, 8)], [(20, 12), (20, 12), (30, 10)]
    masks = [np.full((h, w), 255, np.uint8) for w, h in sizes]
    masks[0][:, 10:] = 0
    return _coded_scene(corners, sizes, bl, dict(empty_pair=(0, 1), c={(0, 1): 0, (0, 2): 10 * 4, (1, 2): 20 * 4}), masks)


# ---------------------------------------------------------------------------------------------------------------------------------
# E5 tree order
# ---------------------------------------------------------------------------------------------------------------------------------
def tree_sum(vals):
    """the fp64 sum as exposure_stats_kernel's EXP_TREE mode makes it: lane t adds elements t, t + 256, ... in that order, then a
    halving tree in which lane t adds lane t + s, s = 128 .. 1"""
    v = np.ravel(np.asarray(vals, np.float64))
    lanes = np.zeros(EXP_WG, np.float64)
    if v.size:
        m = np.concatenate([v, np.zeros(-v.size % EXP_WG)]).reshape(-1, EXP_WG)
        lanes = np.add.accumulate(m, axis=0)[-1]  # sequential along the axis; a lane past the end adds 0.0, which changes no bit
    s = EXP_WG // 2
    while s:
        lanes = lanes[:s] + lanes[s:2 * s]
        s //= 2
    return float(lanes[0])


def tree_sum_contiguous(vals):
    """the variant: lane t sums a contiguous run of ceil(n / 256) elements, then the same tree"""
    v = np.ravel(np.asarray(vals, np.float64))
    k = max(1, -(-v.size // EXP_WG))
    m = np.concatenate([v, np.zeros(k * EXP_WG - v.size)]).reshape(EXP_WG, k)
    lanes = np.add.accumulate(m, axis=1)[:, -1]
    s = EXP_WG // 2
    while s:
        lanes = lanes[:s] + lanes[s:2 * s]
        s //= 2
    return float(lanes[0])


def norm_jobs(scene):
    """per pair of images i <= j whose rectangles overlap (whole images as units) the fp64 norms sqrt(b^2 + g^2 + r^2) of both in the
    job's row-major order, 0.0 where either mask is not 255: what the "gain" kind sums"""
    out = {}
    nrm = [np.sqrt((im.astype(np.int64) ** 2).sum(axis=2).astype(np.float64)) for im in scene.imgs]
    for i in range(len(scene.imgs)):
        for j in range(i, len(scene.imgs)):
            r = overlap_rect(scene.corners, scene.sizes, i, j)
            if r is None:
                continue
            tx, ty, w, h = r
            sl = [(slice(ty - scene.corners[k][1], ty - scene.corners[k][1] + h), slice(tx - scene.corners[k][0], tx - scene.corners[k][0] + w))
                  for k in (i, j)]
            m = (scene.masks[i][sl[0]] == 255) & (scene.masks[j][sl[1]] == 255)
            out[(i, j)] = (int(m.sum()), np.where(m, nrm[i][sl[0]], 0.0), np.where(m, nrm[j][sl[1]], 0.0))
    return out


def tree_large():
    """one overlap of 340 x 300 = 102 000 pixels, the upper end the kernel documents; seeded bytes (their norms are irrational, so
    the order of the sum shows in its last bits)"""
    rng = np.random.default_rng(340)
    w, h = 340, 300
    imgs = [rng.integers(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(2)]
    masks = [np.full((h, w), 255, np.uint8) for _ in range(2)]
    masks[0][rng.random((h, w)) < 0.1] = 0
    return Scene([(3, 5), (3, 5)], imgs, masks, 32, dict(n=w * h))


# ---------------------------------------------------------------------------------------------------------------------------------
# E6 between feeds, E7 filter shapes
# ---------------------------------------------------------------------------------------------------------------------------------
def _texture(rng, w, h):
    return rng.integers(40, 128, (h, w, 3)).astype(np.uint8)


BETWEEN_FEEDS = ("exposures", "small_and_large", "tails")


def between_feeds(which):
    """the same texture at exposures 0.5 and 2 (gains far from 1 after the first feed); rows of 250 outside a's mask (products that
    saturate between feeds).  "small_and_large": 16 x 16 = 256 pixels beside 130 x 130 = 16 900 > 64 * 256, bl = 32 gives blocks of 26.
    "tails": widths 20 .. 23 (w % 4 = 0 .. 3) for the whole-image kinds' 4-pixel kernel"""
    rng = np.random.default_rng(6)
    if which == "tails":
        corners, sizes, bl = [(0, 0), (5, 2), (11, 4), (16, 1)], [(20, 9), (21, 9), (22, 9), (23, 9)], 8
    elif which == "small_and_large":
        corners, sizes, bl = [(40, 50), (0, 0)], [(16, 16), (130, 130)], 32
    else:
        corners, sizes, bl = [(0, 0), (9, 4)], [(50, 36), (50, 36)], 12
    x0, y0 = min(c[0] for c in corners), min(c[1] for c in corners)
    x1, y1 = max(c[0] + s[0] for c, s in zip(corners, sizes)), max(c[1] + s[1] for c, s in zip(corners, sizes))
    tex = _texture(rng, x1 - x0, y1 - y0)
    imgs, masks = [], []
    for k, ((cx, cy), (w, h)) in enumerate(zip(corners, sizes)):
        t = tex[cy - y0:cy - y0 + h, cx - x0:cx - x0 + w].astype(np.float64)
        img = np.clip(np.rint(t * (0.5 if k % 2 == 0 else 2.0)), 0, 255).astype(np.uint8)
        mask = np.full((h, w), 255, np.uint8)
        if k % 2 == 0:  # the dark image: bright rows its mask switches off — multiplied between feeds all the same
            img[:2] = 250
            mask[:2] = 0
        imgs.append(img)
        masks.append(mask)
    grids = [(axis_blocks(w, bl)[1], axis_blocks(h, bl)[1]) for w, h in sizes]
    return Scene(corners, imgs, masks, bl, dict(pixels=[w * h for w, h in sizes], block_sizes=grids, grid_stride_above=BLOCK_MUL_GRID * EXP_WG))


FILTER_GRIDS = ((1, 1), (1, 5), (5, 1), (2, 2), (2, 5))  # (rows, columns) of the block grid


def filter_shapes(grid, bl=8):
    """two images of grid x bl - (2, 3) pixels at (3, 2) from each other, b twice as bright with a ramp across, so the block gains differ
    and the filter has something to smooth; a 1-long axis stays, an axis of 2 reflects onto the other element"""
    rows, cols = grid
    w, h = bl * cols - 3, bl * rows - 2
    rng = np.random.default_rng(7 + 10 * rows + cols)
    tex = _texture(rng, w + 3, h + 2).astype(np.float64)
    ramp = 1.0 + np.arange(w + 3)[None, :, None] / (w + 3.0) + np.arange(h + 2)[:, None, None] / (2.0 * (h + 2))
    a = tex[:h, :w].astype(np.uint8)
    b = np.clip(np.rint(tex * ramp), 0, 255).astype(np.uint8)[2:, 3:]
    masks = [np.full((h, w), 255, np.uint8) for _ in range(2)]
    return Scene([(0, 0), (3, 2)], [a, b], masks, bl, dict(grid=(rows, cols), size=(w, h)))


# ---------------------------------------------------------------------------------------------------------------------------------
# apply: cv::resize(INTER_LINEAR) for CV_32F and cv::multiply's rounding, restated in fp32
# ---------------------------------------------------------------------------------------------------------------------------------
def linear_coeffs(src_n, dst_n, clamp, d0=0, n=None):
    """(source index, fraction) of destination pixels d0 .. d0 + n - 1: f = (float)((d + 0.5) * scale - 0.5), s = floor(f), f -= s;
    clamp (the horizontal pass): s < 0 -> (0, 0), s >= src_n - 1 -> (src_n - 1, 0)"""
    n = dst_n if n is None else n
    scale = 1.0 / (float(dst_n) / float(src_n))
    f = ((np.arange(d0, d0 + n, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    if clamp:
        lo, hi = s < 0, s >= src_n - 1
        s[lo], f[lo] = 0, 0
        s[hi], f[hi] = src_n - 1, 0
    return s, f


def interp_gains(gmap, w, h, sub=None):
    """the gain of every pixel of a w x h image under gain map `gmap` (gh x gw or gh x gw x 3), fp32 operation by operation as
    cv::resize(INTER_LINEAR) makes it; sub = (full_w, full_h, x0, y0): the image is that rectangle of the full image the map lies over.
    A map of the image's size is taken as it is.  -> (h, w, channels of the map)"""
    g = np.asarray(gmap, np.float32)
    g = g[:, :, None] if g.ndim == 2 else g
    gh, gw = g.shape[:2]
    fw, fh, x0, y0 = sub or (w, h, 0, 0)
    if (gw, gh) == (fw, fh):
        return g[y0:y0 + h, x0:x0 + w]
    one = np.float32(1)
    sx, a1 = linear_coeffs(gw, fw, True, x0, w)
    sy, b1 = linear_coeffs(gh, fh, False, y0, h)
    a0, b0 = (one - a1).astype(np.float32), (one - b1).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        sx1 = np.minimum(sx + 1, gw - 1)
        two = (sx < gw - 1)[None, :, None]
        hrow = np.where(two, g[:, sx] * a0[None, :, None] + g[:, sx1] * a1[None, :, None], g[:, sx]).astype(np.float32)
        r0, r1 = np.clip(sy, 0, gh - 1), np.clip(sy + 1, 0, gh - 1)
        return (hrow[r0] * b0[:, None, None] + hrow[r1] * b1[:, None, None]).astype(np.float32)


INT_MIN = -2147483648.0


def half_even(v):
    return np.rint(v)


def half_away(v):
    return np.sign(v) * np.floor(np.abs(v) + 0.5)


def half_up(v):
    return np.floor(v + 0.5)


def products(img, gains):
    """the fp32 products cv::multiply makes: byte x gain (gains (h, w, 1 | 3) or a scalar / BGR triple)"""
    g = np.asarray(gains, np.float32)
    g = np.broadcast_to(g.reshape(1, 1, -1), (1, 1, g.size)) if g.ndim <= 1 else g
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(img, np.uint8).astype(np.float32) * g).astype(np.float32)


def saturate(v, rounding=half_even):
    """saturate_cast<uchar>(cvRound(v)): `rounding` in fp64 (exact for fp32 inputs), INT_MIN outside the int range and for NaN"""
    v = np.asarray(v, np.float64)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(v) & (v >= INT_MIN) & (v < -INT_MIN)
        r = np.where(ok, rounding(np.where(ok, v, 0.0)), INT_MIN)
    return np.clip(r, 0, 255).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------------------------
# A1 ties
# ---------------------------------------------------------------------------------------------------------------------------------
TIE_GAINS = (0.5, 0.75, 1.0, 1.25, 1.5, 2.5, 3.0)
TIE_SCALARS = (0.5, 1.5, 2.5)
TIE_WIDTHS = (20, 21, 22, 23)


def tie_ramp(w, h=13):
    """every byte value in every channel (h * w >= 256 pixels, channel c holds value (p + 85 c) mod 256 at pixel p).  Under a gain
    k + 0.5 every odd byte is a tie"""
    p = np.arange(h * w)[:, None] + 85 * np.arange(3)[None, :]
    img = (p % 256).astype(np.uint8).reshape(h, w, 3)
    return img, dict(odd_bytes=int((img % 2 == 1).sum()), all_values=all(np.unique(img[..., c]).size == 256 for c in range(3)))


TIE_SEEDS = {1: 6, 3: 0}  # of seeds 0 .. 11 the first whose interpolated gains admit both 254.5 and 255.5 (b = 128 under 509 / 256, b = 146 under 1.75)


def ties(channels=1, seed=None, size=(64, 32), map_size=(8, 4)):
    """image = gain map x 8: every interpolation coefficient is a multiple of 1/16 and every interpolated gain a dyadic fraction, exact
    in fp32.  Every byte is chosen so that byte x gain is k + 0.5 where a byte exists that makes it so — by turns a tie that rounds
    down to even, one that rounds up to even and one at 254.5 or above (saturating), else any tie, else a seeded byte; 254.5 and 255.5
    wherever a pixel admits them.
    -> image, gain map, facts (the tie counts; the builder asserts the least the families need)"""
    rng = np.random.default_rng(TIE_SEEDS[channels] if seed is None else seed)
    (w, h), (gw, gh) = size, map_size
    shape = (gh, gw) if channels == 1 else (gh, gw, 3)
    gmap = rng.choice(np.array(TIE_GAINS, np.float32), size=shape)
    g = interp_gains(gmap, w, h).astype(np.float64)
    g = np.broadcast_to(g, (h, w, 3))
    assert np.array_equal(g * 1024, np.rint(g * 1024))  # dyadic: the fp32 gains are what the exact interpolation gives
    b = np.arange(256, dtype=np.float64)
    prod = g[..., None] * b  # (h, w, 3, 256), exact
    tie = prod - np.floor(prod) == 0.5
    down = tie & (np.floor(prod) % 2 == 0) & (prod < 254)  # k even: rounds down
    up = tie & (np.floor(prod) % 2 == 1) & (prod < 254)   # k odd: rounds up
    sat = tie & (prod >= 254.5)
    turn = (np.arange(h * w * 3).reshape(h, w, 3) + rng.integers(0, 3)) % 3
    img = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    pick = rng.random((h, w, 3, 256))
    edge = (prod == 254.5) | (prod == 255.5)
    for cls_k, cls in ((3, tie), (0, down), (1, up), (2, sat), (3, edge)):  # later classes overwrite "any tie" where it is their turn
        has = cls.any(axis=3) & ((turn == cls_k) | (cls_k == 3))
        choice = np.argmax(np.where(cls, pick, -1.0), axis=3)
        img[has] = choice[has].astype(np.uint8)
    p = np.take_along_axis(prod, img[..., None].astype(np.int64), axis=3)[..., 0]
    is_tie = p - np.floor(p) == 0.5
    facts = dict(admits_tie=float(tie.any(axis=3).mean()), ties=int(is_tie.sum()),
                 ties_down=int((is_tie & (np.floor(p) % 2 == 0) & (p < 254)).sum()), ties_up=int((is_tie & (np.floor(p) % 2 == 1) & (p < 254)).sum()),
                 ties_saturating=int((is_tie & (p > 255)).sum()), has_254_5=bool((p == 254.5).any()), has_255_5=bool((p == 255.5).any()))
    return img, gmap, facts


def assert_tie_facts(f):
    assert f["ties_down"] >= 500 and f["ties_up"] >= 500 and f["ties_saturating"] >= 100 and f["has_254_5"] and f["has_255_5"], f


# ---------------------------------------------------------------------------------------------------------------------------------
# A2 the int-range edge
# ---------------------------------------------------------------------------------------------------------------------------------
EDGE_BLOCK = 5  # odd: the centre pixel of a block samples the map at an integer position, where the interpolation returns the gain
EDGE_MAPS = ("edge", "at_bound", "below_bound", "inf", "nan")
F32_BELOW_2_31 = float(np.nextafter(np.float32(2.0 ** 31), np.float32(0)))


def edge_specials(which):
    f = np.float32
    return {"edge": [INT_EDGE_F32, np.nextafter(INT_EDGE_F32, f(0)), np.nextafter(INT_EDGE_F32, f(np.inf))],
            "at_bound": [f(BOUNDED_BELOW)],
            "below_bound": [np.nextafter(f(BOUNDED_BELOW), f(0)), f(-0.0), f(-3.0), f(1e-40)],
            "inf": [f(np.inf), f(-0.0)],
            "nan": [f(np.nan)]}[which]


def int_edge(which, channels=1):
    """a 5 x 3 gain map (1.0 with the special gains of `which` on its even columns of rows 0 and 2, so every neighbour of a special
    gain is finite) over a 25 x 15 image: the centre pixel of a special gain's block holds the bytes (255, 254, 0) and gets the gain
    itself — proved here through interp_gains.  With 3 channels the specials rotate through the channels.
    -> image, map, facts: bounded (what exposure_error_compensator will flag), products at or above 2^31, products on the largest fp32
    below it, 0 x inf"""
    sp = edge_specials(which)
    gw, gh = 5, 3
    gmap = np.ones((gh, gw, channels), np.float32)
    slots = [(r, c) for r in (0, 2) for c in (0, 2, 4)]
    rng = np.random.default_rng(len(which))
    img = rng.integers(0, 256, (gh * EDGE_BLOCK, gw * EDGE_BLOCK, 3)).astype(np.uint8)
    centres = []
    for k, (r, c) in enumerate(slots[:len(sp)]):
        for ch in range(channels):
            gmap[r, c, ch] = sp[(k + ch) % len(sp)]
        cy, cx = r * EDGE_BLOCK + EDGE_BLOCK // 2, c * EDGE_BLOCK + EDGE_BLOCK // 2
        img[cy, cx] = (255, 254, 0)
        centres.append((cy, cx, r, c))
    g = interp_gains(gmap, img.shape[1], img.shape[0])
    for cy, cx, r, c in centres:  # the interpolation returns the gain unchanged (-0.0 may come back as +0.0: the same products)
        assert np.array_equal(g[cy, cx], gmap[r, c], equal_nan=True), (which, g[cy, cx], gmap[r, c])
    p = products(img, g).astype(np.float64)
    gm = gmap[..., 0] if channels == 1 else gmap
    with np.errstate(invalid="ignore"):
        facts = dict(bounded=bool(np.isfinite(gm).all() and np.abs(gm).max() < BOUNDED_BELOW), at_or_above_2_31=int((p >= 2.0 ** 31).sum()),
                     largest_below_2_31=int((p == F32_BELOW_2_31).sum()), nan_products=int(np.isnan(p).sum()),
                     zero_times_inf=bool(which == "inf" and any(np.isnan(p[cy, cx]).any() for cy, cx, _, _ in centres)))
    return img, gm.copy(), facts


# ---------------------------------------------------------------------------------------------------------------------------------
# A3 geometry
# ---------------------------------------------------------------------------------------------------------------------------------
# (w, h, gw, gh): taller than 256 rows and at most 256 wide; widths around the 4-pixel group and the 256 columns of a workgroup; heights
# around its 16 rows; maps of one block, one row, one column, and larger than the image
GEOMETRY = ((5, 700, 1, 22), (3, 300, 2, 10)) + tuple((w, 7, max(1, -(-w // 32)), 2) for w in (1, 2, 3, 4, 5, 255, 256, 257)) + \
    tuple((9, h, 2, max(1, -(-h // 8))) for h in (1, 15, 16, 17, 33)) + ((13, 9, 1, 1), (13, 9, 6, 1), (13, 9, 1, 4), (13, 9, 40, 3))
SUB_FULL = (37, 29, 5, 4)  # the full image and its map; the rectangles (x0, y0, w, h): odd corner, the far corner, one pixel
SUB_RECTS = ((3, 5, 11, 9), (31, 25, 6, 4), (17, 13, 1, 1), (0, 0, 37, 29))


def geometry(w, h, gw, gh, channels=1, seed=0):
    rng = np.random.default_rng(1000 * w + h + seed)
    img = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    gmap = (0.5 + rng.random((gh, gw) if channels == 1 else (gh, gw, 3))).astype(np.float32)
    return img, gmap


def stale_row_table(img, gmap):
    """the variant for tall images: the row table is written for the first ceil(w / 256) * 256 rows only (a grid sized from the width);
    the rows past it read an all-zero entry — source row 0, fraction 0: H[0] * 1 + H[1] * 0, the first map row interpolated across"""
    h, w = img.shape[:2]
    g = interp_gains(gmap, w, h).copy()
    covered = -(-w // GAIN_ROWS_WG) * GAIN_ROWS_WG
    if h > covered:
        g[covered:] = interp_gains(np.asarray(gmap, np.float32)[:1], w, 1)[0]
    return saturate(products(img, g))


def unbounded_in_second_launch(n=18, which=17):
    """n images of 9 x 5 with 2 x 2 maps; image `which` alone holds a gain of 3e7: with 16 images per launch the first launch is FAST,
    the second is not"""
    assert GAIN_BATCH <= which < n <= 2 * GAIN_BATCH
    imgs, maps = zip(*(geometry(9, 5, 2, 2, seed=k) for k in range(n)))
    maps = [m.copy() for m in maps]
    maps[which][1, 1] = np.float32(3e7)
    return list(imgs), maps, dict(bounded=[k != which for k in range(n)])
