"""Constructed inputs for the feather and the "no" blender (csrc/stx_blend.hip: the three column kernels and the row kernel of the
distance transform, feather_gather_kernel, no_gather_kernel): every family is built to reach one path of those kernels that warped ring
images of a few hundred columns never reach, and returns the facts that make it reach it.  Pure numpy, no GPU and no product code:
tests/test_constructed_blends.py asserts the facts against both CPU references (oracle.Blender's handle and tests/numpy_blenders.py) and
shows that each family tells the contract from a one-mistake variant of it; tests/test_gpu_constructed_blends.py runs the same scenes
on the device.

Every builder returns a Scene: the blender kind, its sharpness, the feeds (image, mask, corner) in feed order and `facts`, a dict of
what the construction promises, stated from the construction alone (never from a reference's output).

The distance probe.  The device keeps its distances to itself, and S.Blender's sharpness (1 / blend_width) saturates the weight a few
dozen pixels from the mask's edge.  A probe pair makes every distance visible in the int16 panorama: image A, int16 constant 32767
under the mask in question, fed first; image B, int16 zeros under an all-255 mask of the same size and corner; sharpness 2^-14.  A's
weight is d / 16384 <= 1/2, B's 8192 / 16384 = 1/2, and the result trunc(trunc(32767 * wA) / (wA + 1/2 + 1e-5)) — probe_value(d) — is
strictly increasing in d over 0 .. 8192 (asserted by the CPU test), so equal int16 panoramas are equal distances everywhere.  B is
also the "no zero anywhere" case of the column pass."""
import numpy as np

# Constants of the kernels the families are shaped around.  tests/test_constructed_blends.py reads each of them back from the sources:
# a moved constant fails that test instead of letting the families quietly miss their edges.
CHUNK_ROWS = 64       # STX_DT_RC: rows per chunk of the column pass; the zero rows of a chunk are one 64-bit set ...
HALF_ROWS = 32        # ... handled as two 32-bit halves by dt_col_fill_batch_kernel ...
BITSET_ROWS = 8       # ... and gathered 8 rows at a time by dt_col_summary_batch_kernel
COL_GROUP = 4         # columns per lane in the column pass and in the gathers
ROW_GROUP = 8         # DT_RW: pixels per lane in the row pass
ROW_STEP = 512        # 64 lanes x DT_RW: pixels per wavefront step of the row pass, carry from step to step
CAP = 8192            # STX_FEATHER_DIST_CAP
LDS_BYTES = 65536     # STX_FEATHER_LDS_BYTES: 2 bytes per column and row of a workgroup of the row pass
LDS_WIDTHS = (8192, 16384, 32768)  # the widest image with 4, 2 and 1 rows per workgroup; the last is the widest image at all
SPAN_COLS = 256       # a wavefront of the gathers: 64 lanes x COL_GROUP columns ...
SPAN_ROWS = 4         # ... and a workgroup four rows of them

NO, FEATHER = 0, 1    # STX_BLEND_NO, STX_BLEND_FEATHER (the oracle's handle uses the same numbers)
PROBE_SHARPNESS = 2.0 ** -14
PROBE_VALUE = 32767


def rows_per_block(w):
    """rows of a workgroup of dt_rows_batch_kernel for a batch whose widest image has w columns; 0: refused"""
    lds = (w + ROW_STEP - 1) // ROW_STEP * ROW_STEP * 2
    return 4 if lds * 4 <= LDS_BYTES else 2 if lds * 2 <= LDS_BYTES else 1 if lds <= LDS_BYTES else 0


class Scene:
    def __init__(self, kind, sharpness, feeds, facts):
        self.kind, self.sharpness, self.feeds, self.facts = kind, float(sharpness), list(feeds), facts
        x0 = min(c[0] for _, _, c in self.feeds)
        y0 = min(c[1] for _, _, c in self.feeds)
        x1 = max(c[0] + m.shape[1] for _, m, c in self.feeds)
        y1 = max(c[1] + m.shape[0] for _, m, c in self.feeds)
        self.roi = (x0, y0, x1 - x0, y1 - y0)


# ---------------------------------------------------------------------------------------------------------------------------------
# the probe
# ---------------------------------------------------------------------------------------------------------------------------------
def probe_value(d, sharpness=PROBE_SHARPNESS, value=PROBE_VALUE):
    """the int16 panorama under a probe pair where A's distance is d: FeatherBlender's arithmetic, every step rounded to fp32"""
    f = np.float32
    d = np.asarray(d)
    wa = np.minimum((d.astype(f) * f(sharpness)).astype(f), f(1))
    wb = np.minimum(f(CAP) * f(sharpness), f(1))
    acc = np.trunc((f(value) * wa).astype(f)).astype(f)  # B adds (short)(0 * wB) = 0
    den = ((wa + wb).astype(f) + f(1e-5)).astype(f)
    return np.trunc((acc / den).astype(f)).astype(np.int64)


PROBE_TABLE = probe_value(np.arange(CAP + 1))


def probe_decode(pano16):
    """distances from the int16 panorama of probe pairs; -1 where a value is none of probe_value(0 .. CAP)"""
    v = np.asarray(pano16)[..., 0].astype(np.int64)
    i = np.minimum(np.searchsorted(PROBE_TABLE, v), CAP)
    return np.where(PROBE_TABLE[i] == v, i, -1)


def l1_from_zeros(shape, zeros):
    """the L1 distance to the nearest of `zeros` ((row, column) pairs), saturated at CAP; CAP everywhere without one.  Brute force
    over the zeros: for constructions that know their few zeros"""
    h, w = shape
    d = np.full((h, w), CAP, np.int64)
    yy, xx = np.arange(h)[:, None], np.arange(w)[None, :]
    for zy, zx in zeros:
        np.minimum(d, np.abs(yy - zy) + np.abs(xx - zx), out=d)
    return d


def mask_of(shape, zeros):
    m = np.full(shape, 255, np.uint8)
    for zy, zx in zeros:
        m[zy, zx] = 0
    return m


def probe_feeds(mask, corner=(0, 0)):
    h, w = mask.shape
    return [(np.full((h, w, 3), PROBE_VALUE, np.int16), mask, corner), (np.zeros((h, w, 3), np.int16), np.full((h, w), 255, np.uint8), corner)]


def probe_scene(masks, corners=None, zeros=None, **facts):
    """probe pairs of `masks` at `corners` (disjoint) in one blender.  facts["dist"]: per mask the distances the construction
    promises (from its zeros), or None where the mask does not know them"""
    corners = corners or [(0, 0)] * len(masks)
    feeds = [f for m, c in zip(masks, corners) for f in probe_feeds(m, c)]
    dist = [None if z is None else l1_from_zeros(m.shape, z) for m, z in zip(masks, zeros or [None] * len(masks))]
    return Scene(FEATHER, PROBE_SHARPNESS, feeds, dict(facts, dist=dist, corners=corners, probe=True))


# ---------------------------------------------------------------------------------------------------------------------------------
# Family 1.  Chunk edges: 9 columns (two whole column groups and a ninth column), every column with its own single zero row out of
# CHUNK_EDGE_ROWS, rotated over the columns so that the four columns of a lane's group differ
# ---------------------------------------------------------------------------------------------------------------------------------
CHUNK_EDGE_W = 9
CHUNK_EDGE_H = (1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200)
CHUNK_EDGE_ROWS = (0, 31, 32, 63, 64, "last", None)


def chunk_edges(h, rot):
    zeros = []
    for j in range(CHUNK_EDGE_W):
        r = CHUNK_EDGE_ROWS[(j + rot) % len(CHUNK_EDGE_ROWS)]
        r = h - 1 if r == "last" else r
        if r is not None and r < h:
            zeros.append((r, j))
    return probe_scene([mask_of((h, CHUNK_EDGE_W), zeros)], zeros=[zeros], zero_rows={j: r for r, j in zeros})


# ---------------------------------------------------------------------------------------------------------------------------------
# Family 2.  Far links: five chunks and a remainder; zero rows only in chunk 0, only in the last chunk, or in both with the chunks
# 1 .. 3 (and 4) empty between them: dt_col_link_batch_kernel carries first / last zero rows across empty chunks
# ---------------------------------------------------------------------------------------------------------------------------------
FAR_LINK_W, FAR_LINK_H = 6, 323
FAR_LINK_WHERE = ("first", "last", "both")


def far_links(where):
    zeros = []
    for j in range(FAR_LINK_W):
        if where in ("first", "both"):
            zeros.append(((11 * j + 5) % CHUNK_ROWS, j))  # rows 5, 16, 27, 38, 49, 60 of chunk 0
        if where in ("last", "both"):
            zeros.append((5 * CHUNK_ROWS + j % 3, j))  # rows 320 .. 322: the remainder chunk
    chunks = sorted({zy // CHUNK_ROWS for zy, _ in zeros})
    return probe_scene([mask_of((FAR_LINK_H, FAR_LINK_W), zeros)], zeros=[zeros], chunks_with_zeros=chunks,
                       empty_chunks=[c for c in range((FAR_LINK_H + CHUNK_ROWS - 1) // CHUNK_ROWS) if c not in chunks])


# ---------------------------------------------------------------------------------------------------------------------------------
# Family 3.  The cap in the column pass.  8261 rows, 6 columns.  "both" is column 0 with a zero in row 0 and column 1 with one in the
# last row: every pixel is then within 4134 steps of a zero and the cap is reached only inside the column pass (columns 2 .. 5 hold
# "no zero").  "top" and "bottom" have one of the two zeros each: there the result itself passes 8191, 8192 and "would be 8193"
# ---------------------------------------------------------------------------------------------------------------------------------
COLUMN_CAP_W, COLUMN_CAP_H = 6, 8261
COLUMN_CAP_WHERE = ("top", "bottom", "both")


def column_cap(where):
    zeros = ([(0, 0)] if where in ("top", "both") else []) + ([(COLUMN_CAP_H - 1, 1)] if where in ("bottom", "both") else [])
    facts = {}
    if where == "top":  # column 0: d = row
        facts["at"] = {(CAP - 1, 0): CAP - 1, (CAP, 0): CAP, (CAP + 1, 0): CAP, (CAP - 1, 1): CAP, (COLUMN_CAP_H - 1, 5): CAP}
        facts["would_be"] = {(CAP + 1, 0): CAP + 1}
    elif where == "bottom":  # column 1: d = 8260 - row
        last = COLUMN_CAP_H - 1
        facts["at"] = {(last - CAP + 1, 1): CAP - 1, (last - CAP, 1): CAP, (last - CAP - 1, 1): CAP, (0, 1): CAP}
        facts["would_be"] = {(last - CAP - 1, 1): CAP + 1}
    else:
        facts["at"] = {(4130, 0): 4130, (4131, 0): 4130, (CAP, 0): COLUMN_CAP_H - 1 - CAP + 1}
    return probe_scene([mask_of((COLUMN_CAP_H, COLUMN_CAP_W), zeros)], zeros=[zeros], **facts)


# ---------------------------------------------------------------------------------------------------------------------------------
# Family 4.  Row steps: three rows (the fourth wavefront of a four-row workgroup is dead), every row with its own single zero column
# out of ROW_STEP_COLS, rotated over the rows; at 1540 columns also a lone zero in column 0 (the forward carry crosses three step
# edges) and a lone one in the last column (the backward carry)
# ---------------------------------------------------------------------------------------------------------------------------------
ROW_STEP_H = 3
ROW_STEP_W = (1, 7, 8, 9, 15, 16, 17, 511, 512, 513, 1023, 1024, 1025, 1540)
ROW_STEP_COLS = (0, 7, 8, 511, 512, "last", None)
LONE_W = 1540
LONE_WHERE = ("first", "last")


def row_steps(w, rot):
    zeros = []
    for i in range(ROW_STEP_H):
        c = ROW_STEP_COLS[(i + rot) % len(ROW_STEP_COLS)]
        c = w - 1 if c == "last" else c
        if c is not None and c < w:
            zeros.append((i, c))
    return probe_scene([mask_of((ROW_STEP_H, w), zeros)], zeros=[zeros], zero_cols={i: c for i, c in zeros})


def lone_zero(where):
    zeros = [(1, 0 if where == "first" else LONE_W - 1)]
    far = LONE_W - 1 if where == "first" else 0
    return probe_scene([mask_of((ROW_STEP_H, LONE_W), zeros)], zeros=[zeros], at={(1, far): LONE_W - 1, (0, far): LONE_W},
                       step_edges_crossed=(LONE_W - 1) // ROW_STEP)


# ---------------------------------------------------------------------------------------------------------------------------------
# Family 5.  LDS row counts and the cap in the row pass: five rows; the widths on both sides of the two thresholds and the widest
# ---------------------------------------------------------------------------------------------------------------------------------
LDS_H = 5
LDS_W = (8192, 8193, 16384, 16385, 32768)


def lds_rows(w):
    zeros = [(0, 0), (1, w - 1), (2, w // 2)]
    return probe_scene([mask_of((LDS_H, w), zeros)], zeros=[zeros], rows_per_block=rows_per_block(w),
                       workgroups=-(-LDS_H // rows_per_block(w)))


# ---------------------------------------------------------------------------------------------------------------------------------
# Family 6.  Unequal batch: one blender, probe pairs of very different shape at disjoint corners — one grid, sized by the largest
# ---------------------------------------------------------------------------------------------------------------------------------
UNEQUAL = (((700, 3), (0, 0)), ((3, 700), (0, 10)), ((1, 1), (10, 10)), ((520, 130), (20, 20)))  # ((width, height), corner)


def unequal_masks():
    rng = np.random.default_rng(6)
    out = []
    for (w, h), corner in UNEQUAL:
        n = 0 if w * h == 1 else 5
        zeros = sorted({(int(rng.integers(h)), int(rng.integers(w))) for _ in range(n)})
        out.append((mask_of((h, w), zeros), zeros, corner))
    return out


def unequal_batch():
    ms = unequal_masks()
    return probe_scene([m for m, _, _ in ms], [c for _, _, c in ms], [z for _, z, _ in ms], widest=700, tallest=700)


# ---------------------------------------------------------------------------------------------------------------------------------
# Family 7.  Views and padding: masks the device test feeds as views at x offsets 1, 2, 3 modulo 4 into larger buffers that hold 0, or
# 255, around them.  The column pass reads whole dwords, so it computes on those surroundings; nothing of them may reach the image
# ---------------------------------------------------------------------------------------------------------------------------------
VIEW_SHAPE = (130, 1030)
VIEW_DENSITY = ("sparse", "half")
VIEW_OFFSETS = (1, 2, 3)
VIEW_SURROUND = (0, 255)


def view_mask(density):
    rng = np.random.default_rng({"sparse": 71, "half": 72}[density])
    h, w = VIEW_SHAPE
    m = np.where(rng.random(VIEW_SHAPE) < {"sparse": 1e-3, "half": 0.5}[density], 0, 255).astype(np.uint8)
    m[0, :4] = m[h - 1, w - 4:] = m[1, 0] = m[h - 2, w - 1] = 255  # two corners whose distance is certainly not 1
    zeros = [tuple(p) for p in np.argwhere(m == 0)]
    # border pixels that are not 0 and have no 0 beside them inside the image: their distance is 2 or more — 1 only for a transform
    # that takes what lies outside the image for zeros
    nz = np.pad(m != 0, 1, constant_values=True)
    inner = nz[1:-1, 1:-1] & nz[:-2, 1:-1] & nz[2:, 1:-1] & nz[1:-1, :-2] & nz[1:-1, 2:]
    edge = np.zeros(VIEW_SHAPE, bool)
    edge[0], edge[-1], edge[:, 0], edge[:, -1] = True, True, True, True
    return m, zeros, np.argwhere(inner & edge)


def views(density):
    m, zeros, far_edge = view_mask(density)
    return probe_scene([m], zeros=[zeros if len(zeros) <= 1000 else None], edge_at_least_2=far_edge, n_zeros=len(zeros))


# ---------------------------------------------------------------------------------------------------------------------------------
# Family 8.  Placement: a backdrop as wide as the panorama and one-row images 1 .. 8 wide at the offsets around a wavefront's first
# and last column, each on a row of its own.  Panoramas 257 .. 260 wide end on every length of the tail store
# ---------------------------------------------------------------------------------------------------------------------------------
PLACE_PANO_W = (520, 257, 258, 259, 260)
PLACE_SMALL_W = (1, 2, 3, 4, 5, 8)
PLACE_X = (0, 1, 2, 3, 253, 254, 255, 256, 257)


def _values(rng, shape, dtype):
    if dtype == np.uint8:
        return rng.integers(1, 256, shape + (3,)).astype(np.uint8)
    return rng.integers(-32768, 32768, shape + (3,)).astype(np.int16)


def placement(kind, dtype, pano_w):
    """feeds[0] is the backdrop; facts["small"]: the indices of the small images (fed after it, each on its own row)"""
    rng = np.random.default_rng(800 + pano_w)
    spots = [(w, x) for w in PLACE_SMALL_W for x in PLACE_X if x + w <= pano_w]
    feeds = [(_values(rng, (len(spots), pano_w), dtype), np.full((len(spots), pano_w), 255, np.uint8), (0, 0))]
    for row, (w, x) in enumerate(spots):
        feeds.append((_values(rng, (1, w), dtype), np.full((1, w), 255, np.uint8), (x, row)))
    # full masks: every feather weight is min(8192 * sharpness, 1) = 1
    return Scene(kind, 0.5, feeds, {"small": list(range(1, len(feeds))), "spots": spots, "tail": pano_w % COL_GROUP})


# ---------------------------------------------------------------------------------------------------------------------------------
# Family 9.  The ones path: a feather whose weight reaches 1 at distance 2.  Span 0 of image A lies wholly where every weight is 1;
# in span 1 a single zero mask pixel in column 357 = 1 (mod 4) keeps the weights below 1 inside ONE lane's group in each of three rows
# ---------------------------------------------------------------------------------------------------------------------------------
ONES_ZERO = (4, 357)


def ones_path():
    rng = np.random.default_rng(9)
    h, w = 8, 2 * SPAN_COLS
    ma = mask_of((h, w), [ONES_ZERO])
    feeds = [(_values(rng, (h, w), np.uint8), ma, (0, 0)), (_values(rng, (h, w), np.uint8), np.full((h, w), 255, np.uint8), (2, 2))]
    zy, zx = ONES_ZERO
    below_one = sorted([(zy, zx), (zy, zx - 1), (zy, zx + 1), (zy - 1, zx), (zy + 1, zx)])
    return Scene(FEATHER, 0.5, feeds, {"below_one": below_one, "lane_group": zx // COL_GROUP, "span": zx // SPAN_COLS})


# ---------------------------------------------------------------------------------------------------------------------------------
# Family 10.  Accumulator wrap: FeatherBlender adds (short)(px * w) into int16 with two's complement wrap-around
# ---------------------------------------------------------------------------------------------------------------------------------
WRAP_KINDS = ("ones", "border", "s16")
WRAP_N = 140


def accumulator_wrap(which):
    if which == "s16":  # 32767 + 32767 wraps to -2; / 2.00001 -> 0 ((short)(-0.99..))
        feeds = [(np.full((8, 8, 3), 32767, np.int16), np.full((8, 8), 255, np.uint8), (0, 0))] * 2
        return Scene(FEATHER, 0.5, feeds, {"sum": 2 * 32767, "wrapped": -2, "value": 0})
    m = np.full((8, 8), 255, np.uint8)
    if which == "border":  # distances 1 .. 3 inside a zero frame: the weights 0.32 d stay below 1, every lane is on the float path
        m[0] = m[-1] = m[:, 0] = m[:, -1] = 0
    feeds = [(np.full((8, 8, 3), 255, np.uint8), m, (0, 0))] * WRAP_N
    if which == "ones":  # 140 * 255 = 35700 wraps to -29836; / 140.00001 -> -213; convertScaleAbs -> 213
        return Scene(FEATHER, 0.5, feeds, {"sum": WRAP_N * 255, "wrapped": WRAP_N * 255 - 65536, "value": -213, "u8": 213})
    # (short)(255 * 0.32 d) = 81, 163, 244: 140 of the last are 34160 and wrap, 140 of the others do not
    return Scene(FEATHER, 0.32, feeds, {"sums": {1: WRAP_N * 81, 2: WRAP_N * 163, 3: WRAP_N * 244}, "wraps_at": 3})


# ---------------------------------------------------------------------------------------------------------------------------------
# Family 11.  Weight sum order: three overlapping images with weights k / 10; fp32 sums of those depend on the order of the addends
# ---------------------------------------------------------------------------------------------------------------------------------
def weight_sum_order():
    rng = np.random.default_rng(11)
    feeds = []
    for k, corner in enumerate(((0, 0), (5, 3), (9, 7))):
        h, w = 40, 300
        m = np.full((h, w), 255, np.uint8)
        m[rng.integers(h, size=40), rng.integers(w, size=40)] = 0
        feeds.append((_values(rng, (h, w), np.int16), m, corner))
    return Scene(FEATHER, 0.1, feeds, {"weights": [k / 10 for k in range(11)]})


# ---------------------------------------------------------------------------------------------------------------------------------
# Family 12.  The "no" gather: the last fed image whose mask is set wins, the panorama's mask is the OR of all masks
# ---------------------------------------------------------------------------------------------------------------------------------
NO_STACK_HOLE = (5, 100)


def no_stack(grey, dtype):
    """binary: five images on one rectangle; the last covers span 0 but for one pixel, the hole (the early exit is one lane short of
    firing there), and all of span 1 (it fires).  Under the hole images 3 and 2 are 0 and image 1 is 255: the walk has to go on down
    to image 1 for that one lane, and an exit that fires a lane early leaves value 0 and mask 0 there.  grey: images 0 .. 2 carry
    masks of the constants 1, 2 and 4 instead; under the hole image 3 is 0, so image 2 gives the value and the mask is 7"""
    rng = np.random.default_rng(120 + grey)
    h, w = 8, 2 * SPAN_COLS
    feeds = []
    for k in range(5):
        if k == 4:
            m = mask_of((h, w), [NO_STACK_HOLE])
        elif grey and k < 3:
            m = np.full((h, w), 1 << k, np.uint8)
        else:
            m = np.where(rng.random((h, w)) < 0.5, 255, 0).astype(np.uint8)
        feeds.append((_values(rng, (h, w), dtype), m, (0, 0)))
    if grey:  # the last image leaves columns 300 .. 399 to the stack below it
        feeds[4][1][:, 300:400] = 0
        feeds[3][1][:, 350:400] = 0
    for k in (2, 3):
        if not (grey and k == 2):
            feeds[k][1][NO_STACK_HOLE] = 0
    if not grey:
        feeds[1][1][NO_STACK_HOLE] = 255
    facts = {"hole": NO_STACK_HOLE, "winner_elsewhere": 4, "winner_hole": 2 if grey else 1, "mask_hole": 7 if grey else 255}
    if grey:
        facts.update(or_of_greys=7, grey_only=(slice(None), slice(350, 400)), winner_grey_only=2)
    return Scene(NO, 0.0, feeds, facts)
