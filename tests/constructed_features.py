"""Constructed inputs for FeatureEstimator (csrc/stx_features.hip, csrc/stx_features_host.cpp): every family is built to reach one path
of the kernels or of the 64-bit key that seeded noise, three grey values, a dot and a checker of at most 200 x 150 never reach, and
returns the facts that make it reach it.  Pure numpy, no GPU and no product code: tests/test_constructed_features.py asserts the facts
against the contract tests/numpy_features.py and shows that each family tells the contract from a one-mistake variant of it;
tests/test_gpu_constructed_features.py runs the same inputs on the device.

Every builder returns (image or list of images, facts); the constructed images are u8 BGR with B = G = R, whose grey is that value.
`facts` is a dict of what the construction promises, stated from the construction alone (never from the contract's output)."""
import numpy as np

# Constants of the kernels the families are shaped around.  tests/test_constructed_features.py reads each of them back from
# stx_internal.h: if the tiles are re-cut, that test fails instead of the families quietly missing their borders.
BORDER = 16          # STX_FEAT_BORDER: keypoints lie in [16, w - 17] x [16, h - 17]; score tiles start at (16, 16)
SCORE_TW = 32        # STX_FEAT_SCORE_TW
SCORE_TH = 8         # STX_FEAT_SCORE_TH
BLUR_TW = 64         # STX_FEAT_BLUR_TW
R_BIAS = 1 << 33     # STX_FEAT_R_BIAS: the key holds R_BIAS - R above y << 15 | x
REACH = 20           # two keypoints this far apart on an axis share no pixel of a 9 x 9 patch and a radius-15 disc (15 + 4 < 20)

# Family 1.  A 9 x 9 patch of 0 / 255: centre 255, the 16 ring pixels 0, the other cells found by a greedy search (flip a cell, keep the
# flip if the centre stays a candidate at threshold 20 and R grows) from a checker of 2 x 2 cells.  Only the result is kept.
PATCH = 255 * np.array([[0, 0, 1, 1, 0, 0, 1, 1, 0],
                        [0, 1, 1, 0, 0, 0, 1, 1, 0],
                        [1, 1, 0, 0, 1, 1, 0, 0, 1],
                        [0, 0, 1, 1, 0, 0, 1, 0, 0],
                        [0, 0, 1, 1, 1, 0, 1, 0, 0],
                        [1, 0, 0, 0, 1, 1, 0, 0, 1],
                        [1, 1, 0, 0, 1, 1, 0, 1, 1],
                        [0, 1, 1, 0, 0, 0, 1, 1, 0],
                        [0, 0, 1, 1, 0, 0, 1, 0, 0]], np.uint8)
PATCH_R = 2151674779  # of the centre: between 2^31 and 2^32

TILED_SIZES = ((420, 300), (420, 40), (40, 420))
TILED_PITCH = (31, 23)  # coprime to SCORE_TW and to SCORE_TH: the copies' columns run through the residues 0, 31, 30, ... of 32, the rows 0, 7, 6, ... of 8
SELECTION_THRESHOLD = 5
SCALES = ((1.05, 16), (1.5, 8), (2.0, 8))  # (scale, nlevels)
# 24 images: the first and the last have no level, image 5 is listed again as image 17
BATCH_SIZES = ((32, 40), (33, 33), (33, 50), (50, 33), (48, 48), (64, 64), (65, 40), (40, 65), (97, 71), (71, 97), (80, 60), (100, 100),
               (34, 120), (120, 34), (63, 63), (66, 35), (35, 66), None, (90, 70), (57, 43), (43, 57), (128, 96), (39, 39), (40, 32))
BATCH_TWICE = (5, 17)
TOO_SMALL_SIZES = ((32, 32), (20, 100), (100, 20), (32, 33), (1, 1))


def bgr(g):
    return np.ascontiguousarray(np.repeat(np.asarray(g, np.uint8)[:, :, None], 3, axis=2))


def _stamp(g, x, y, patch=PATCH):
    """patch with its centre on (x, y)"""
    r = patch.shape[0] // 2
    g[y - r:y + r + 1, x - r:x + r + 1] = patch


def high_response(w=41, h=41):
    """Family 1: the patch alone on black, its centre in the middle of the image."""
    g = np.zeros((h, w), np.uint8)
    x, y = w // 2, h // 2
    _stamp(g, x, y)
    return bgr(g), {"keypoint": (x, y), "R": PATCH_R}


# Family 2.  Profiles of the rows -4 .. +4 around a keypoint row whose value is 200 (the keypoint pixel itself is 221): every other row is
# darker than 200 by more than the threshold of 20, rows -1 and +1 are far apart
NEGATIVE_PROFILES = ((100, 100, 100, 0, 200, 170, 100, 100, 100), (60, 60, 60, 150, 200, 10, 60, 60, 60))
NEGATIVE_ROWS = (20, 32)
NEGATIVE_COLUMNS = (40, 23)
POSITIVE_DOT = (30, 44)  # (x, y): 255 on a band of black rows


def negative_response():
    """Family 2: 64 x 64, every row constant but for three pixels.  Two keypoints sit on a row of 200 as one pixel of 221 between darker
    rows: Ix is 0 but beside that pixel, so a = 2 * 21^2, b = 0 and c is large, and R = (25 a c - (a + c)^2) >> 16 is negative.  A dot on
    black rows is the ordinary corner with R > 0."""
    g = np.zeros((64, 64), np.uint8)
    for profile, y0, x0 in zip(NEGATIVE_PROFILES, NEGATIVE_ROWS, NEGATIVE_COLUMNS):
        for d, v in zip(range(-4, 5), profile):
            g[y0 + d, :] = v
        g[y0 - 6:y0 - 4, :] = profile[0]  # the rows between two profiles are constant too
        g[y0 + 5:y0 + 7, :] = profile[-1]
        g[y0, x0] = 221
    g[39:, :] = 0
    g[POSITIVE_DOT[1], POSITIVE_DOT[0]] = 255
    negatives = [(x, y) for x, y in zip(NEGATIVE_COLUMNS, NEGATIVE_ROWS)]
    return bgr(g), {"negatives": negatives, "positive": POSITIVE_DOT, "threshold": 20}


def _lattice(n, pitch):
    """keypoint coordinates on one axis: from BORDER in steps of pitch, and the last legal one, n - 17, at least REACH from the others"""
    last = n - 1 - BORDER
    return [v for v in range(BORDER, last - REACH + 1, pitch)] + [last]


def tiled(w=420, h=300):
    """Family 3: the family-1 patch repeated on black, so far apart that no copy sees another: every keypoint has the same R, bin and
    descriptor, and only y and x tell their keys apart.  A side of 40 holds one row (column) of copies, on its last legal row."""
    px, py = TILED_PITCH
    assert px >= REACH and py >= REACH
    xs, ys = _lattice(w, px), _lattice(h, py)
    g = np.zeros((h, w), np.uint8)
    for y in ys:
        for x in xs:
            _stamp(g, x, y)
    return bgr(g), {"xs": xs, "ys": ys, "keypoints": [(x, y) for y in ys for x in xs], "R": PATCH_R}


PLATEAU_SIZE = (120, 56)
PLATEAU_PAIRS = (((BORDER + SCORE_TW - 1, 18), (BORDER + SCORE_TW, 18)),          # across the first and the second border between
                 ((BORDER + 2 * SCORE_TW - 1, 36), (BORDER + 2 * SCORE_TW, 36)),  # score tiles of a row
                 ((20, BORDER + SCORE_TH - 1), (20, BORDER + SCORE_TH)),          # and, transposed, between tiles of a column
                 ((64, BORDER + 2 * SCORE_TH - 1), (64, BORDER + 2 * SCORE_TH)))
PLATEAU_DOT = (100, 20)


def plateau():
    """Family 4: a bright pixel joined to its mirror image: two adjacent pixels of 255 on black have the same score, 255, above all their
    other neighbours', so neither is strictly above its 8 neighbours and neither is a candidate.  Each pair straddles a border between
    two score tiles: the equal neighbour's score is one that the tile computes in its halo.  A single dot is the keypoint that remains."""
    w, h = PLATEAU_SIZE
    g = np.zeros((h, w), np.uint8)
    for a, b in PLATEAU_PAIRS:
        g[a[1], a[0]] = g[b[1], b[0]] = 255
    g[PLATEAU_DOT[1], PLATEAU_DOT[0]] = 255
    return bgr(g), {"pairs": PLATEAU_PAIRS, "dot": PLATEAU_DOT}


# Family 5.  Pixels (u, v, value) beside a dot, a set that (u, v) -> (v, u) maps onto itself, outside every ring that the dot's suppression reads
TIE_BLOB = ((6, 6, 255), (5, 8, 200), (8, 5, 200), (7, 9, 90), (9, 7, 90))
TIE_KINDS = ("diagonal+", "diagonal-", "antidiagonal+", "antidiagonal-", "both")
TIE_BINS = {"diagonal+": (4, 5), "diagonal-": (22, 23), "antidiagonal+": (31, 32), "antidiagonal-": (13, 14), "both": tuple(range(36))}
TIE_SIZE = (161, 41)


def orientation_ties():
    """Family 5: five dots (centre 255, ring 0) in one row, 30 apart, each with its disc symmetric under a mirror.  (u, v) -> (v, u) gives
    m10 = m01 and the maximum of m (CX[b] + CY[b]) at 45 or 225 degrees, between two bins; (u, v) -> (-v, -u) gives m10 = -m01 and
    315 or 135 degrees; both mirrors give m10 = m01 = 0, where all 36 bins tie.  CX[b] == CY[(9 - b) % 36] makes the ties exact."""
    w, h = TIE_SIZE
    g = np.zeros((h, w), np.uint8)
    keypoints = {}
    for k, kind in enumerate(TIE_KINDS):
        x, y = 20 + 30 * k, 20
        g[y, x] = 255
        for u, v, value in TIE_BLOB:
            for su, sv in {"diagonal+": ((1, 1),), "diagonal-": ((-1, -1),), "antidiagonal+": ((1, -1),), "antidiagonal-": ((-1, 1),),
                           "both": ((1, 1), (-1, -1))}[kind]:
                g[y + sv * v, x + su * u] = value
        keypoints[kind] = (x, y)
    return bgr(g), {"keypoints": keypoints, "bins": TIE_BINS}


def smoothed_noise(w, h, seed):
    """seeded noise, each pixel averaged with its right, lower and lower-right neighbours (wrapping): corners everywhere"""
    a = np.random.RandomState(7000 + seed).randint(0, 256, (h, w, 3)).astype(np.uint16)
    return ((a + np.roll(a, -1, 0) + np.roll(a, -1, 1) + np.roll(a, (-1, -1), (0, 1)) + 2) // 4).astype(np.uint8)


def selection_level():
    """Families 6 and 8: one 200 x 150 level of smoothed noise; at threshold 5 it has more than 600 candidates (asserted on the CPU)."""
    return smoothed_noise(200, 150, 0), {"threshold": SELECTION_THRESHOLD, "at_least": 600}


def selection_sizes(count):
    """nfeatures around the 256-key chunks of the survivor and ranking loops, and on both sides of `count > keep`"""
    return (255, 256, 257, 511, 512, 513, count - 1, count, count + 1)


def mask_pixel(x, y, level_size, size):
    """(row, column) of the mask pixel that decides about candidate (x, y) of a level of level_size = (w_l, h_l) in an image of size (w0, h0)"""
    (wl, hl), (w0, h0) = level_size, size
    return ((2 * y + 1) * h0) // (2 * hl), ((2 * x + 1) * w0) // (2 * wl)


def pick_mask_keypoints(ref, size=(420, 300)):
    """Family 7: from the contract's result `ref` of the tiled image over 3 levels -> the indices of one keypoint of level 2 and of one of
    level 0 with x >= 256, each the only keypoint that its mask pixel decides about"""
    pixels = [mask_pixel(x, y, ref["level_sizes"][l], size) for l, x, y in zip(ref["level"].tolist(), ref["x"].tolist(), ref["y"].tolist())]
    alone = [pixels.count(p) == 1 for p in pixels]
    return [next(k for k in range(len(pixels)) if alone[k] and ref["level"][k] == level and ref["x"][k] >= least) for level, least in ((2, 0), (0, 256))]


def single_pixel_masks(size, pixel, one_at):
    """Family 7: (a mask that is 0 but for `pixel`, its complement: 255 but for `pixel`, with the value 1 at `one_at`)"""
    w0, h0 = size
    only, rest = np.zeros((h0, w0), np.uint8), np.full((h0, w0), 255, np.uint8)
    only[pixel] = 255
    rest[pixel] = 0
    rest[one_at] = 1
    return only, rest


def batch():
    """Family 8: 24 images of mixed sizes; the first and the last have no level, one is listed twice (the same array)."""
    imgs = [None if s is None else smoothed_noise(s[0], s[1], 10 + i) for i, s in enumerate(BATCH_SIZES)]
    imgs[BATCH_TWICE[1]] = imgs[BATCH_TWICE[0]]
    return imgs, {"no_level": (0, len(imgs) - 1), "twice": BATCH_TWICE}


def too_small_batch():
    return [smoothed_noise(w, h, 50 + i) for i, (w, h) in enumerate(TOO_SMALL_SIZES)], {"levels": 0}
