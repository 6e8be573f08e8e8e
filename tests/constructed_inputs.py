"""Constructed inputs for the three device search stages (csrc/stx_color_seams.hip, stx_seams.hip, stx_crop.hip): every family is built
to reach one structural path of a kernel that warped masks and i.i.d. noise never reach, and returns the facts that make it reach it.
Pure numpy, no GPU and no product code: tests/test_constructed_inputs.py asserts the facts against the numpy contracts
(numpy_color_seams, numpy_seams, numpy_lir) and shows that each family tells the contract from a plausibly wrong variant;
tests/test_gpu_constructed_inputs.py runs the same inputs on the device.

Seam families return (corners, imgs, masks, facts); mask families return (mask, facts).  `facts` is a dict of what the construction
promises, stated from the construction alone (never from a contract's output)."""
import numpy as np

from tests.numpy_color_seams import MAX_COST, MAX_SEAM_LENGTH  # noqa: F401  (3 * 255^2 and 16384: the contract's own)
from tests.numpy_seams import GAP                              # the voronoi finder's gap around a roi

# Constants of the kernels the families are shaped around.  tests/test_constructed_inputs.py reads each of them back from the .hip
# sources: if a kernel's constant moves, that test fails instead of the families quietly missing their paths.
ROW_STEP = 256               # SEAM_STEP: pixels per wavefront step of seam_rows_kernel (64 lanes * SEAM_PX)
COL_BATCH = 8                # SEAM_BATCH: rows per batch of seam_cols_kernel
LIR_LANES = 256              # CROP_WG: lanes of crop_rows_kernel, a lane owns ceil(W / 256) bars
LIR_LDS_MAX_W = 4864         # CROP_LDS_MAX_W: rows up to this width keep their pointers in LDS, wider ones in a global scratch slice
LIR_ROWS_GRID = 2048         # CROP_ROWS_GRID: workgroups of crop_rows_kernel, more rows than this take the grid-stride loop
BACK = 64                    # CS_BACK: rows per walk-back step of color_seam_dp_kernel; its window is 2 * BACK - 1 columns wide
SEAM_LANES = 256             # CS_WG: lanes of color_seam_dp_kernel, K columns per lane

ZIGZAG_L = (64, 65, 66, 128, 129, 130, 200, 333)
ZIGZAG_W = (2, 3, 64, 65, 70, 257, 600)
RAGGED_RW = (235, 236, 237, 491, 492, 493, 600)   # + 2 * GAP: windows of 255, 256, 257, 511, 512, 513 and 620 pixels
RAGGED_RH = (1, 4, 5, 7, 8, 9, 12, 30)
RAGGED_DENSITY = (0.1, 0.5, 0.9)
PROFILES = ("ascending", "descending", "tent", "valley", "comb", "sawtooth")
HISTOGRAM_W = (257, 700, 4864, 4865, 5200)
HISTOGRAM_H = 40


# ---------------------------------------------------------------------------------------------------------------------------------
# colour seams
# ---------------------------------------------------------------------------------------------------------------------------------
def _side_by_side(W, L, transpose):
    """two images whose overlap is W across and L along a vertical seam (or the same stacked: a horizontal one); the first in the list
    is the FIRST image of the pair.  -> corners, sizes (w, h), roi (x, y, w, h)"""
    sizes, corners, roi = [(W + 3, L), (W + 2, L)], [(0, 0), (3, 0)], (3, 0, W, L)
    if transpose:
        sizes, corners, roi = [(h, w) for w, h in sizes], [(y, x) for x, y in corners], (0, 3, L, W)
    return corners, sizes, roi


def _paint(img, corner, roi, transpose, rt_values):
    """img[roi] = rt_values ((L, W, 3): r along the seam, t across it)"""
    x, y, w, h = roi
    v = rt_values.transpose(1, 0, 2) if transpose else rt_values
    img[y - corner[1]:y - corner[1] + h, x - corner[0]:x - corner[0] + w] = v


def zigzag_valley(L, W, anchor_high=False):
    """t(r): one column per row between 0 and W - 1, anchored on a border at r = L - 1, where the walk back starts: the first 64-row
    window then sees the seam run monotonically from the border for min(63, W - 1) columns"""
    k = (L - 1) - np.arange(L)
    if W == 1:
        return np.zeros(L, np.int64)
    p = 2 * (W - 1)
    t = np.minimum(k % p, p - k % p)
    return (W - 1 - t) if anchor_high else t


def window_drifts(s):
    """per walk-back window (r_hi = L - 1, L - 1 - 64, ...): (r_hi, rows n the step walks, the farthest |s(r_hi - q) - s(r_hi)| over
    q <= min(63, r_hi), the farthest window column at which a choice is READ: q < n)"""
    s = np.asarray(s, np.int64)
    out, r_hi = [], len(s) - 1
    while r_hi > 0:
        n = min(BACK, r_hi)
        q = np.arange(min(BACK - 1, r_hi) + 1)
        d = np.abs(s[r_hi - q] - s[r_hi])
        out.append((r_hi, n, int(d.max()), int(d[:n].max())))
        r_hi -= n
    return out


def zigzag_pair(L, W, transpose=False, first_is_j=False, v=255):
    """Image i is black, image j the constant (v, v, v) except along the valley t(r), where it is black too: c = 0 on the valley and
    3 v^2 off it, so the only path of cost 0, and the contract's seam, is the valley.  Both masks are full.  The valley is anchored at
    t = W - 1 when first_is_j, else at t = 0, so that over the family the walk starts on either border."""
    corners, sizes, roi = _side_by_side(W, L, transpose)
    t = zigzag_valley(L, W, anchor_high=first_is_j)
    imgs = [np.zeros((h, w, 3), np.uint8) for w, h in sizes]
    bright = np.full((L, W, 3), v, np.uint8)
    bright[np.arange(L), t] = 0
    imgs[1][:] = 77  # outside the roi: never read
    _paint(imgs[1], corners[1], roi, transpose, bright)
    masks = [np.full((h, w), 255, np.uint8) for w, h in sizes]
    if first_is_j:  # the same pair listed the other way round: the FIRST image (smaller centre) is now j
        corners, imgs, masks = corners[::-1], imgs[::-1], masks[::-1]
    drifts = window_drifts(t)
    facts = {"valley": t.astype(np.int32), "roi": roi, "vertical": not transpose, "first_is_i": not first_is_j,
             "drift": max(d[2] for d in drifts), "reach": max(d[3] for d in drifts), "windows": drifts,
             "touches": (bool((t == 0).any()), bool((t == W - 1).any())), "L": L, "W": W}
    return corners, imgs, masks, facts


def zigzag_cover():
    """(L, W, transpose, first_is_j): every L with every W (so every L at W = 70 and every W at L = 200), orientation and order
    spread so that each value of every factor meets each value of every other factor (tests/test_constructed_inputs.py checks it)"""
    return [(L, W, (a + b) % 2 == 1, (a // 2 + b) % 2 == 1) for a, L in enumerate(ZIGZAG_L) for b, W in enumerate(ZIGZAG_W)]


def three_squares(lo, hi):
    """the largest c in [lo, hi] that is a^2 + b^2 + d^2 with 0 <= a, b, d <= 255.  -> (c, (a, b, d))"""
    sq = np.arange(256, dtype=np.int64) ** 2
    two = (sq[:, None] + sq[None, :])
    for c in range(hi, lo - 1, -1):
        rest = c - two
        ok = (rest >= 0) & (rest <= 255 * 255)
        root = np.rint(np.sqrt(np.where(ok, rest, 0))).astype(np.int64)
        hit = ok & (root * root == rest)
        if hit.any():
            a, b = (int(i) for i in np.argwhere(hit)[0])
            return c, (a, b, int(root[a, b]))
    raise ValueError((lo, hi))


def saturated_pair(W, jog=0):
    """L = 16384 rows, W columns of constant cost: black against white (195 075 a row, 3 196 108 800 in all) everywhere but one cheap
    column tc of cost c a row, c chosen so that the cheap column's sum stays just below 2^31 while its neighbours' accumulators pass it.

    jog = 0: every column constant.  A(L-1, tc) = L c < 2^31 <= A(L-1, tc +- 1) = (L - 1) c + 195 075: the final arg-min compares
             accumulators on both sides of 2^31; the seam is the cheap column.
    jog = -1 / +1: the cheap column's last cell is white too and its neighbour (L-1, tc + jog) costs 0.  Then already A(L-2, tc +- 1) =
             (L - 2) c + 195 075 >= 2^31 > A(L-2, tc) = (L - 1) c, and the seam's last step chooses between them: `right < best`
             (jog -1) or `left < best` (jog +1) compares across 2^31 ON the seam.  The seam is tc up to row L - 2 and tc + jog at L - 1.
    The closed forms hold because every other path pays at least one white cell more (asserted in the CPU test from the sums)."""
    L = MAX_SEAM_LENGTH
    tc = {3: 2, 5: 3}[W] if jog <= 0 else {3: 0, 5: 1}[W]
    assert 0 <= tc + jog < W
    if jog == 0:
        c, colour = three_squares(0, (2 ** 31 - 1) // L)
    else:
        c, colour = three_squares(0, (2 ** 31 - 1) // (L - 1))
    corners, sizes, roi = _side_by_side(W, L, False)
    imgs = [np.zeros((h, w, 3), np.uint8) for w, h in sizes]
    rt = np.full((L, W, 3), 255, np.uint8)
    rt[:, tc] = colour
    seam = np.full(L, tc, np.int32)
    if jog:
        rt[L - 1, tc] = 255
        rt[L - 1, tc + jog] = 0
        seam[L - 1] = tc + jog
    _paint(imgs[1], corners[1], roi, False, rt)
    masks = [np.full((h, w), 255, np.uint8) for w, h in sizes]
    rows_paid = L if jog == 0 else L - 1
    facts = {"roi": roi, "cheap": tc, "c": c, "seam": seam, "L": L, "W": W,
             "seam_sum": rows_paid * c,                                   # A(L-1) at the seam's end
             "neighbour_sum": (rows_paid - 1) * c + MAX_COST,             # the accumulator next to it in the row the comparison reads
             "neighbour_row": L - 1 if jog == 0 else L - 2}
    return corners, imgs, masks, facts


def fork_pair(transpose=False):
    """A 5-wide, 6-long overlap of cost 0 except: the last row is bright but for t = 2, and the cell above it, (L-2, 2), is bright.  At
    (L-1, 2) straight costs 3 v^2 and both diagonals 0: the tie t - 1 against t + 1 lies ON the seam.  The contract takes t - 1 and
    then goes straight: s = 1, 1, 1, 1, 1, 2."""
    L, W = 6, 5
    corners, sizes, roi = _side_by_side(W, L, transpose)
    imgs = [np.zeros((h, w, 3), np.uint8) for w, h in sizes]
    rt = np.zeros((L, W, 3), np.uint8)
    rt[L - 1] = 255
    rt[L - 1, 2] = 0
    rt[L - 2, 2] = 255
    _paint(imgs[1], corners[1], roi, transpose, rt)
    masks = [np.full((h, w), 255, np.uint8) for w, h in sizes]
    return corners, imgs, masks, {"roi": roi, "seam": np.array([1, 1, 1, 1, 1, 2], np.int32), "L": L, "W": W}


def mixed_level(seed=0):
    """Seven images, five pairs, three levels.  Level 0 holds three pairs that share no image: (0, 1) with W = 600, L = 5, (2, 3) with
    W = 3, L = 300 — one launch of the 4-columns-per-lane kernel serves both — and the horizontal (4, 5) with L = 40, W = 20.  Image 6
    lies over the roi of (4, 5): (4, 6) is level 1 and (5, 6) level 2.  Mask 2 is empty on rows 100 .. 179 (`both` empty: the cost
    is 0 across those rows), and mask 6 is empty wherever image 4 lies, so `both` of (4, 6) is empty altogether while its roi is not."""
    rng = np.random.default_rng(seed)
    corners = [(0, 0), (3, 0), (2000, 0), (2003, 0), (3000, 0), (3000, 3), (3010, 10)]
    sizes = [(603, 5), (602, 5), (6, 300), (5, 300), (40, 23), (40, 22), (50, 14)]
    imgs = [(rng.integers(0, 4, (h, w, 3)) * 85).astype(np.uint8) for w, h in sizes]
    masks = [((rng.random((h, w)) < 0.9) * rng.choice([255, 254, 1], (h, w))).astype(np.uint8) for w, h in sizes]
    masks[2][100:180] = 0
    masks[6][:13] = 0          # image 4 ends at y = 23: rows 10 .. 22 of the panorama
    masks[6][13] = 255
    facts = {"pairs": [(0, 1, 3, 0, 600, 5), (2, 3, 2003, 0, 3, 300), (4, 5, 3000, 3, 40, 20), (4, 6, 3010, 10, 30, 13),
                       (5, 6, 3010, 10, 30, 14)],                          # i, j and the roi, in run()'s order
             "levels": [0, 0, 0, 1, 2], "nlevels": 3,
             "LW": [(5, 600), (300, 3), (40, 20), (13, 30), (14, 30)],    # (L, W) of each pair
             "vertical": [True, True, False, True, True], "empty_both": 3, "zero_cost_rows": (1, slice(100, 180))}
    return corners, imgs, masks, facts


# ---------------------------------------------------------------------------------------------------------------------------------
# voronoi
# ---------------------------------------------------------------------------------------------------------------------------------
def ragged_pair(rw, rh, density, seed):
    """Two noise masks (0, 255, 254, 1) over a roi of rw x rh.  Image 0 reaches past the roi on the left and above, image 1 on the right
    and below, each by 1 .. 15 pixels: inside the 10-pixel gap lie pixels of one image only, sources of that image's distance.  From
    four roi rows on, one roi row is blank in both images (noise alone never leaves a row of 235 pixels without a source)."""
    rng = np.random.default_rng([seed, rw, rh, int(density * 100)])
    a, b, c, d = (int(v) for v in rng.integers(1, 16, 4))
    sizes = [(rw + a, rh + b), (rw + c, rh + d)]
    corners = [(-7, 5), (-7 + a, 5 + b)]
    masks = [((rng.random((h, w)) < density) * rng.choice([255, 254, 1], (h, w))).astype(np.uint8) for w, h in sizes]
    blank = None
    if rh >= 4:  # one roi row is empty in both images over their whole width: a window row with no source at all
        blank = rh // 2
        masks[0][b + blank] = 0
        masks[1][blank] = 0
    imgs = [np.zeros((h, w, 3), np.uint8) for w, h in sizes]
    facts = {"roi": (-7 + a, 5 + b, rw, rh), "window": (rw + 2 * GAP, rh + 2 * GAP), "margins": (a, b, c, d),
             "blank_row": None if blank is None else GAP + blank}  # as a window row
    return corners, imgs, masks, facts


def far_source_pair(rw=700, rh=12):
    """Full masks but for single pixels, over a roi of rw x rh (a window of 720 columns: three steps of 256).  A zero in one mask is a
    unique pixel of the other: the only sources.  Window rows (roi row + GAP) and what they hold:
      row 2   mask 1 lacks column 1: image 0's only source of the row lies on the far left, up to 698 columns from the roi's pixels —
              the left-to-right carry l1 crosses two steps
      row 4   mask 1 lacks column rw - 2: the same from the right (n1)
      row 6   mask 0 lacks column 1, row 7 mask 0 lacks column rw - 2: image 1's sources (l2, n2)
      row 9   image 0's only source lies in the gap: image 0 reaches 12 columns past the roi on the left, its mask there is 0 but for
              one pixel at window column 2
      every other row has no source at all (the gap above and below lies outside both images)."""
    corners, sizes = [(0, 0), (12, 0)], [(rw + 12, rh), (rw, rh)]
    masks = [np.full((h, w), 255, np.uint8) for w, h in sizes]
    masks[0][:, :12] = 0
    masks[0][9, 4] = 254                      # window column 4 - (12 - GAP) = 2
    masks[1][2, 1] = 0
    masks[1][4, rw - 2] = 0
    masks[0][6, 12 + 1] = 0
    masks[0][7, 12 + rw - 2] = 0
    imgs = [np.zeros((h, w, 3), np.uint8) for w, h in sizes]
    facts = {"roi": (12, 0, rw, rh),
             # window row -> (image whose source it is, window column of the row's only source)
             "sources": {GAP + 2: (1, GAP + 1), GAP + 4: (1, GAP + rw - 2), GAP + 6: (2, GAP + 1), GAP + 7: (2, GAP + rw - 2),
                         GAP + 9: (1, 2)},
             "window": (rw + 2 * GAP, rh + 2 * GAP)}
    return corners, imgs, masks, facts


def tie_pair(rw=301, rh=21, seed=3):
    """Two images on the same rectangle with mirror-symmetric masks: mask 1 is mask 0 flipped left to right, each full but for a few
    single pixels.  unique2 is the mirror image of unique1, so dist1(x, y) = dist2(rw - 1 - x, y): on the middle column dist1 == dist2
    on every row, and the decision there is the tie's (mask i is zeroed)."""
    assert rw % 2 == 1
    rng = np.random.default_rng(seed)
    m = np.full((rh, rw), 255, np.uint8)
    ys, xs = rng.integers(0, rh, 9), rng.integers(0, rw // 2 - 1, 9)  # holes left of the middle only: never on their own mirror image
    m[ys, xs] = 0
    masks = [m, m[:, ::-1].copy()]
    imgs = [np.zeros((rh, rw, 3), np.uint8)] * 2
    return [(0, 0), (0, 0)], imgs, masks, {"roi": (0, 0, rw, rh), "tie_column": rw // 2}


# ---------------------------------------------------------------------------------------------------------------------------------
# largest interior rectangle: histograms
# ---------------------------------------------------------------------------------------------------------------------------------
def profile(name, W, H=HISTOGRAM_H):
    """h(x) in 1 .. H"""
    x = np.arange(W, dtype=np.int64)
    up = 1 + x * H // W
    if name == "ascending":
        return up
    if name == "descending":
        return up[::-1].copy()
    if name == "tent":
        return np.minimum(1 + 2 * x * H // W, 1 + 2 * (W - 1 - x) * H // W).clip(1, H)
    if name == "valley":
        return (H + 1 - np.minimum(1 + 2 * x * H // W, 1 + 2 * (W - 1 - x) * H // W)).clip(1, H)
    if name == "comb":
        return np.where(x % 2 == 0, H, 1)
    if name == "sawtooth":
        return 1 + (x % 37) * (H - 1) // 36
    raise KeyError(name)


def histogram_mask(name, W, H=HISTOGRAM_H, anchor="bottom"):
    """mask[y, x] = y >= H - h(x) (bars standing on the last row); anchor "top": the same upside down, mask[y, x] = y < h(x).
    The row stage sees v(y, x), the run of true cells downward: standing bars give rows of two values (0 and H - y, in runs as long as
    the profile's steps), hanging bars give the profile itself, h(x) - y: a staircase of many values in every row."""
    h = profile(name, W, H)
    y = np.arange(H)[:, None]
    m = (y >= H - h[None, :]) if anchor == "bottom" else (y < h[None, :])
    return (m * 255).astype(np.uint8), {"profile": h, "chunk": -(-W // LIR_LANES), "in_lds": W <= LIR_LDS_MAX_W}


def notched_mask(H=2100, W=4865):
    """A full mask with one zero pixel every 97 rows: more rows than the row stage has workgroups (its grid-stride loop) and wider than
    its LDS holds (the global scratch slice), at once.  Every notch is a hole of its own: none lies on the border."""
    m = np.full((H, W), 255, np.uint8)
    ys = np.arange(48, H - 1, 97)
    xs = 1 + (ys * 613) % (W - 2)
    m[ys, xs] = 0
    return m, {"notches": len(ys), "chunk": -(-W // LIR_LANES), "in_lds": W <= LIR_LDS_MAX_W, "grid_stride": H > LIR_ROWS_GRID}


def down_runs(mask):
    """v(y, x): the run of true cells from (x, y) downward (crop_cols_kernel)"""
    g = np.asarray(mask) != 0
    v = np.zeros(g.shape, np.int64)
    run = np.zeros(g.shape[1], np.int64)
    for y in range(g.shape[0] - 1, -1, -1):
        run = np.where(g[y], run + 1, 0)
        v[y] = run
    return v


def nearest_smaller(v):
    """For every bar of every row of v (H, W): the column of the nearest strictly smaller bar on the left (-1: none) and on the right
    (W: none).  The pointer walk of the kernel, all bars at once: a pointer whose bar is not smaller jumps to that bar's pointer."""
    v = np.ascontiguousarray(v, np.int64)
    H, W = v.shape
    flat = v.ravel()
    cell = np.arange(H * W, dtype=np.int64)
    out = []
    for step, stop in ((-1, -1), (1, W)):
        ptr = cell % W + step                      # column pointed at, per cell
        act = cell
        while act.size:                            # only the walks still under way
            cur, base = ptr[act], act - act % W
            go = cur != stop
            go[go] = flat[base[go] + cur[go]] >= flat[act[go]]
            act, cur, base = act[go], cur[go], base[go]
            ptr[act] = ptr[base + cur]
        out.append(ptr.reshape(H, W))
    return out[0], out[1]


def farthest_smaller(mask, rows=None, real=False):
    """The largest distance from a nonzero bar to its nearest strictly smaller bar, over the rows `rows` of v (all by default) — the
    rows as the kernel sees them: v is taken from the WHOLE mask first.  Where a bar has no smaller bar on a side its walk ends at the
    row's end (column -1 or W), having crossed every chunk on the way: that distance counts too, unless real=True, which counts
    walks that end at an actual bar only."""
    v = down_runs(mask)
    if rows is not None:
        v = v[rows]
    W = v.shape[1]
    lf, rt = nearest_smaller(v)
    x = np.arange(W)[None, :]
    on = v > 0
    left, right = on & ((lf >= 0) | (not real)), on & ((rt < W) | (not real))
    return int(max(np.where(left, x - lf, 0).max(), np.where(right, rt - x, 0).max()))


# ---------------------------------------------------------------------------------------------------------------------------------
# largest interior rectangle: contours
# ---------------------------------------------------------------------------------------------------------------------------------
def spiral_mask(n=401, closed=False):
    """A one-pixel-wide square spiral of foreground with one pixel of background between its arms, walked inward from (0, 0).  Open: one
    component, and the background corridor reaches the border at (1, 0): (1, 0).  closed: that entrance is filled, the corridor becomes
    one hole: (1, 1).  Vertical arms are runs of one pixel: label chains as long as the spiral."""
    m = np.zeros((n, n), np.uint8)
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = 255
    length = 1

    def free(yy, xx, ddy, ddx):
        ny, nx = yy + ddy, xx + ddx
        if not (0 <= ny < n and 0 <= nx < n) or m[ny, nx]:
            return False
        ay, ax = ny + ddy, nx + ddx
        return not (0 <= ay < n and 0 <= ax < n) or not m[ay, ax]

    while True:
        if not free(y, x, dy, dx):
            dy, dx = dx, -dy  # turn right
            if not free(y, x, dy, dx):
                break
        y, x = y + dy, x + dx
        m[y, x] = 255
        length += 1
    if closed:
        m[1, 0] = 255
    return m, {"length": length, "counts": (1, 1) if closed else (1, 0)}


def serpentine_mask(n=400):
    """Every other row is foreground, joined to the next one alternately at the right and the left end: one component; every background
    row reaches the border at its open end: (1, 0)."""
    m = np.zeros((n, n), np.uint8)
    m[0::2] = 255
    for k, y in enumerate(range(1, n - 1, 2)):
        m[y, n - 1 if k % 2 == 0 else 0] = 255
    return m, {"length": int(np.count_nonzero(m)), "counts": (1, 0)}


def rings_mask(k, n):
    """k concentric one-pixel square rings, one pixel of background between them, in an n x n mask (n >= 4 k - 3).  k components; the
    background between two rings is a hole each, and so is the inside of the innermost ring when it has one (its side n - 4 (k - 1)
    is at least 3)."""
    assert n >= 4 * k - 3
    m = np.zeros((n, n), np.uint8)
    for r in range(k):
        a, b = 2 * r, n - 1 - 2 * r
        m[a, a:b + 1] = m[b, a:b + 1] = 255
        m[a:b + 1, a] = m[a:b + 1, b] = 255
    inner = n - 4 * (k - 1)
    return m, {"counts": (k, k if inner >= 3 else k - 1)}


def diagonal_mask(n=300, complement=False):
    """Single foreground pixels on the diagonal: one component under the 8-neighbourhood, and both background triangles reach the
    border: (1, 0).  complement: a filled square whose diagonal pixels (1, 1) .. (n - 2, n - 2) are background — they touch each other
    only diagonally, and the background is 4-connected: n - 2 holes."""
    i = np.arange(n)
    if not complement:
        m = np.zeros((n, n), np.uint8)
        m[i, i] = 255
        return m, {"counts": (1, 0)}
    m = np.full((n, n), 255, np.uint8)
    m[i[1:-1], i[1:-1]] = 0
    return m, {"counts": (1, n - 2)}
