"""Constructed masks and sizes for the resize kernels (stitching_amd/csrc/stx_resize.hip, stx_resize_host.cpp): pure numpy, no product
code.  Every family returns cases with `facts` stated from the construction alone; tests/test_constructed_resizes.py holds them against
the contract (tests/numpy_resize.py) without a GPU, tests/test_gpu_constructed_resizes.py runs them on the device.

A seam-mask case is a dict:
  name    for messages
  lows    the low-resolution seam masks (numpy, u8)
  finals  one Final per image: a parent image and the view of it that is handed over as the final warped mask
  sub     None, or one (full_w, full_h, x0, y0) per image: the view is that rectangle of a full mask
  batch   True: one SeamFinder.resize_all call; False: one SeamFinder.resize call (one image)
  facts   what the construction guarantees

`expected_path(case)` restates the host's choice of kernels from the construction alone: a parent is an image of the library's own
(rows of BUF_PITCH-byte multiples holding whole 8-pixel groups, first byte aligned to the pitch unit), so a view at column x of it
starts x bytes (mod 8) off alignment.  The constants below are the sources' own; the CPU test reads them back from the sources.
"""
import functools
import math
from fractions import Fraction

import numpy as np

from tests import numpy_resize as NR

SEAM1_COLS, SEAM1_ROWS = 8, 8            # pixels and rows per lane of the one-launch LDS kernel
TILE_W, TILE_H = 64 * SEAM1_COLS, 4 * SEAM1_ROWS  # its 512 x 32 destination tile
SEAM_BATCH = 16                          # images per launch of either batch loop
SEAM_ROWS = 16                           # destination rows per lane of the 4-pixel kernels
RESIZE_TW, RESIZE_TH = 64, 4             # destination tile of the image-resize kernels
LDS_BUDGET = 40 << 10                    # bytes of window the one-launch kernel may ask for
BUF_PITCH = 64                           # row pitch unit of the library's own images
PATHS = ("lds", "tables_batch", "single_4px", "single_1px", "per_image_fallback", "aligned_copy_then_lds")
COUNTERS = ("lds", "tables_batch", "single_4px", "single_1px")  # the order of stx_debug_seam_resize_paths


def buf_pitch(w, c=1):
    return -(-(-(-w // 8) * 8 * c) // BUF_PITCH) * BUF_PITCH


class Final:
    """the view parent[y:y + h, x:x + w] of a device image `parent`"""

    def __init__(self, parent, x=0, y=0, w=None, h=None):
        self.parent = np.ascontiguousarray(parent, np.uint8)
        self.x, self.y = int(x), int(y)
        self.w = self.parent.shape[1] - self.x if w is None else int(w)
        self.h = self.parent.shape[0] - self.y if h is None else int(h)
        assert self.w > 0 and self.h > 0 and self.x + self.w <= self.parent.shape[1] and self.y + self.h <= self.parent.shape[0]

    @property
    def array(self):
        return self.parent[self.y:self.y + self.h, self.x:self.x + self.w]

    @property
    def whole(self):
        return (self.x, self.y) == (0, 0) and self.array.shape == self.parent.shape

    def aligned(self, k):
        """pointer and pitch multiples of k, and the row readable up to the next multiple of k columns"""
        pitch = buf_pitch(self.parent.shape[1])
        return self.x % k == 0 and pitch % k == 0 and -(-self.w // k) * k <= pitch


def framed(inner, x, y, right=3, below=2):
    """-> Final: `inner` at (x, y) of a parent whose other bytes are all 0xff (a read past the view shows up in the result)"""
    h, w = inner.shape
    parent = np.full((y + h + below, x + w + right), 0xff, np.uint8)
    parent[y:y + h, x:x + w] = inner
    return Final(parent, x, y, w, h)


def case(name, lows, finals, sub=None, batch=True, **facts):
    finals = [f if isinstance(f, Final) else Final(f) for f in finals]
    assert len(lows) == len(finals) and (batch or (len(lows) == 1 and sub is None))
    return {"name": name, "lows": [np.array(a, np.uint8, order="C") for a in lows], "finals": finals,
            "sub": None if sub is None else [tuple(int(v) for v in q) for q in sub], "batch": batch, "facts": facts}


def single(c, i):
    """image i of a case without sub as a SeamFinder.resize call"""
    assert c["sub"] is None
    return case(f"{c['name']}[{i}]", [c["lows"][i]], [c["finals"][i]], batch=False)


def full_size(c, i):
    f = c["finals"][i]
    return (f.w, f.h) if c["sub"] is None else c["sub"][i][:2]


# ---------------------------------------------------------------------------------------------------------------------------------
# the host's choice
# ---------------------------------------------------------------------------------------------------------------------------------
def window_bound(src_n, full_n, tile):
    """source columns (rows) the host reserves under a tile: min(src, ceil(tile * scale) + 3)"""
    scale = 1.0 / (float(full_n) / float(src_n))
    return min(src_n, int(math.ceil(tile * scale)) + 3)


def lds_bytes(c):
    """the one-launch kernel's dynamic LDS for the whole call: window + halo, and its dilation"""
    pitch = rows = 0
    for i, low in enumerate(c["lows"]):
        fw, fh = full_size(c, i)
        pitch = max(pitch, window_bound(low.shape[1], fw, TILE_W) + 2)
        rows = max(rows, window_bound(low.shape[0], fh, TILE_H))
    pitch = (pitch + 3) // 4 * 4
    return pitch * (rows + 2) + pitch * rows


def _single_path(c):
    f, = c["finals"]
    if f.aligned(8) and lds_bytes(c) <= LDS_BUDGET:
        return "lds"
    return "single_4px" if f.aligned(4) else "single_1px"


def expected_path(c):
    if not c["batch"]:
        return _single_path(c)
    fast = all(f.aligned(4) for f in c["finals"])
    if not fast and c["sub"] is None:
        return "per_image_fallback"
    fits = lds_bytes(c) <= LDS_BUDGET
    if not fast:  # the unaligned rectangles are copied into images of the library's own: those are 8-aligned
        return "aligned_copy_then_lds" if fits and all(f.aligned(8) for f in c["finals"] if f.aligned(4)) else "tables_batch"
    return "lds" if fits and all(f.aligned(8) for f in c["finals"]) else "tables_batch"


def image_paths(c):
    """-> per image, the kernel (one of COUNTERS) its pixels are made by"""
    p = expected_path(c)
    if p == "per_image_fallback":
        return [_single_path(single(c, i)) for i in range(len(c["lows"]))]
    return [{"aligned_copy_then_lds": "lds"}.get(p, p)] * len(c["lows"])


def expected_counts(c):
    """-> what stx_debug_seam_resize_paths moves by over the call"""
    paths = image_paths(c)
    return [paths.count(k) for k in COUNTERS]


def tile_window(src_n, full_n, first, count):
    """source columns (rows) the kernel stages for the destination indices first .. first + count - 1: from the first one's offset to
    one past the last one's, clamped to the source"""
    a, b = NR.coeff(first, src_n, full_n)[0], NR.coeff(first + count - 1, src_n, full_n)[0]
    return min(b + 1, src_n - 1) - a + 1


# ---------------------------------------------------------------------------------------------------------------------------------
# paint
# ---------------------------------------------------------------------------------------------------------------------------------
def low_mask(rng, h, w, grey=False):
    """blobs of 255 on 0 at about a quarter of the area (so the dilation leaves 0, 255 and edges), optionally a few other values"""
    m = np.where(rng.random((h, w)) < 0.25, 255, 0).astype(np.uint8)
    if grey:
        k = rng.random((h, w)) < 0.1
        m[k] = rng.integers(1, 255, int(k.sum()), dtype=np.uint8)
    return m


def final_mask(rng, h, w):
    """mostly 255, zeros and arbitrary bytes elsewhere: the AND is bitwise"""
    m = np.full((h, w), 255, np.uint8)
    k = rng.random((h, w)) < 0.3
    m[k] = rng.integers(0, 256, int(k.sum()), dtype=np.uint8)
    return m


# ---------------------------------------------------------------------------------------------------------------------------------
# view_offsets
# ---------------------------------------------------------------------------------------------------------------------------------
VIEW_X0 = {"lds": (0, 8), "single_4px": (4, 12), "single_1px": (1, 2, 3, 5, 7)}
VIEW_WIDTHS = (12, 13, 15, 21) + tuple(range(1, 10))  # 4k, 4k + 1, 4k + 3, 8k + 5, 1 .. 9
VIEW_HEIGHTS = (5, 17, 33, 66)  # below / across the 8 and 16 rows of a lane, the 32 and 64 rows of a workgroup


def _view_pair(rng, x0, w, k):
    h = VIEW_HEIGHTS[k % len(VIEW_HEIGHTS)]
    low = low_mask(rng, 2 + k % 3, 1 + (w + 4) // 5, grey=k % 2 == 1)
    return low, framed(final_mask(rng, h, w), x0, 1 + k % 2)


def view_offsets():
    rng = np.random.default_rng(101)
    out = []
    for path, offsets in VIEW_X0.items():
        for x0 in offsets:
            pairs = [_view_pair(rng, x0, w, k) for k, w in enumerate(VIEW_WIDTHS)]
            for (low, f), w in zip(pairs, VIEW_WIDTHS):
                out.append(case(f"view x0={x0} w={w}", [low], [f], batch=False, path=path, x0=x0, width=w))
            lows, finals = [p[0] for p in pairs], [p[1] for p in pairs]
            out.append(case(f"views x0={x0} batch", lows, finals, x0=x0,
                            path={"lds": "lds", "single_4px": "tables_batch", "single_1px": "per_image_fallback"}[path]))
            # the same views as rectangles of larger final masks
            sub = [(f.w + 8 + 4 * (k % 3), f.h + 5, 4 * (k % 3), k % 4) for k, f in enumerate(finals)]
            out.append(case(f"views x0={x0} batch sub", lows, finals, sub=sub, x0=x0,
                            path={"lds": "lds", "single_4px": "tables_batch", "single_1px": "aligned_copy_then_lds"}[path]))
    # one odd-offset view among aligned masks: the whole call is demoted (without sub), or that one image is copied (with sub)
    lows = [low_mask(rng, 3 + k, 4 + k) for k in range(5)]
    finals = [Final(final_mask(rng, 20 + 7 * k, 30 + 9 * k)) for k in range(5)]
    finals[3] = framed(finals[3].parent, 5, 2)
    out.append(case("one odd view among aligned", lows, finals, path="per_image_fallback",
                    image_paths=["lds", "lds", "lds", "single_1px", "lds"]))
    sub = [(f.w + 12, f.h + 3, 8, 2) for f in finals]
    out.append(case("one odd view among aligned, sub", lows, finals, sub=sub, path="aligned_copy_then_lds"))
    # ... and one 4-aligned view next to the odd one: after the copy the call still cannot take the LDS kernel
    finals = list(finals)
    finals[1] = framed(finals[1].parent, 4, 0)
    out.append(case("odd and 4-aligned views, sub", lows, finals, sub=sub, path="tables_batch"))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# lds_budget
# ---------------------------------------------------------------------------------------------------------------------------------
def budget_edge(sw=700, sh=40):
    """-> (dw_fits, dw_over): the narrowest destination of a sw x sh mask (height kept) whose window still fits the budget, and the next
    narrower one, by lds_bytes' own arithmetic"""
    probe = lambda dw: lds_bytes(case("probe", [np.zeros((sh, sw), np.uint8)], [np.zeros((sh, dw), np.uint8)], batch=False))  # noqa: E731
    dw = sw
    assert probe(dw) <= LDS_BUDGET
    while probe(dw - 1) <= LDS_BUDGET:
        dw -= 1
    return dw, dw - 1


def lds_budget():
    rng = np.random.default_rng(102)
    out = []

    def one(sw, sh, dw, dh, **kw):
        c = case(f"budget {sw}x{sh}->{dw}x{dh}", [low_mask(rng, sh, sw)], [final_mask(rng, dh, dw)], batch=False, **kw)
        c["facts"]["lds_bytes"] = lds_bytes(c)
        return c

    out.append(one(700, 50, 350, 25, path="single_4px", factor=0.5))   # (52 + 50) rows of 704 bytes
    out.append(one(520, 40, 520, 40, path="lds", factor=1.0))           # (37 + 35) rows of 520 bytes
    fits, over = budget_edge()
    out.append(one(700, 40, fits, 40, path="lds", edge="fits"))
    out.append(one(700, 40, over, 40, path="single_4px", edge="over"))
    # one downscaled image among enlargements: the budget is computed from the whole batch
    lows = [low_mask(rng, 4, 6), low_mask(rng, 50, 700), low_mask(rng, 5, 3)]
    finals = [final_mask(rng, 40, 90), final_mask(rng, 25, 350), final_mask(rng, 33, 70)]
    c = case("budget: one downscale in a batch", lows, finals, path="tables_batch")
    c["facts"]["lds_bytes"] = lds_bytes(c)
    out.append(c)
    c = case("budget: over the edge in a batch", [low_mask(rng, 40, 700), low_mask(rng, 3, 3)], [final_mask(rng, 40, over), final_mask(rng, 9, 9)],
             path="tables_batch")
    c["facts"]["lds_bytes"] = lds_bytes(c)
    out.append(c)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# window_reach
# ---------------------------------------------------------------------------------------------------------------------------------
def reach(src_n, full_n, tile, step):
    """-> (largest window over all tile starts that are multiples of `step`, the start it is found at, the host's bound)"""
    best, at = 0, 0
    for s in range(0, full_n, step):
        n = tile_window(src_n, full_n, s, min(tile, full_n - s))
        if n > best:
            best, at = n, s
    return best, at, window_bound(src_n, full_n, tile)


def find_reach(tile, step, src_range, factor=2.766, clamped=True):
    """the first src -> dst (dst about factor * src) whose largest window equals the host's bound; clamped: the bound is the whole
    source (the min with the source size holds), else the ceil(tile * scale) + 3 side"""
    for src in src_range:
        for dst in range(int(src * factor) - 2, int(src * factor) + 3):
            got, at, bound = reach(src, dst, tile, step)
            if got == bound and (bound == src) == clamped and dst > tile / 4:
                return src, dst, at
    raise AssertionError("no such size")


def window_reach():
    rng = np.random.default_rng(103)
    out = []
    for sw, dw in ((60, 165), (60, 166), (60, 167), (61, 166), (59, 166)):  # 60 -> 166: a tile's window is all 60 columns, the bound is 60
        got, at, bound = reach(sw, dw, TILE_W, 4)
        out.append(case(f"reach cols {sw}->{dw}", [low_mask(rng, 3, sw)], [final_mask(rng, 20, dw)], batch=False, path="lds",
                        window=got, bound=bound, axis="x"))
    sh, dh, _ = find_reach(TILE_H, 1, range(8, 40))
    for a, b in ((sh, dh - 1), (sh, dh), (sh, dh + 1)):
        got, at, bound = reach(a, b, TILE_H, 1)
        out.append(case(f"reach rows {a}->{b}", [low_mask(rng, a, 5)], [final_mask(rng, b, 37)], batch=False, path="lds",
                        window=got, bound=bound, axis="y"))
    # several tiles, where the bound is the ceil(tile * scale) + 3 side: the widest windows leave one column / row spare
    for sw, dw, axis in ((7, 1544, "x"), (5, 166, "y")):
        tile, step = (TILE_W, 4) if axis == "x" else (TILE_H, 1)
        got, at, bound = reach(sw, dw, tile, step)
        low, fin = low_mask(rng, 3, sw), final_mask(rng, 9, dw)
        out.append(case(f"reach {axis} {sw}->{dw} tiles", [low if axis == "x" else low.T.copy()], [fin if axis == "x" else fin.T.copy()], batch=False,
                        path="lds", window=got, bound=bound, axis=axis))
    # rectangles whose first column / row lies at every phase of the source grid: 60 -> 166 is 2.77 destination columns per source one
    lows, finals, sub = [], [], []
    for k, x0 in enumerate(range(0, 48, 4)):
        y0 = k  # rows: 11 -> 30, 2.7 destination rows per source row
        w, h = min(166 - x0, 50 + 3 * k), min(30 - y0, 7 + k)
        lows.append(low_mask(rng, 11, 60))
        finals.append(final_mask(rng, h, w))
        sub.append((166, 30, x0, y0))
    phases = {(NR.coeff(q[2], 60, 166)[1], NR.coeff(q[3], 11, 30)[1]) for q in sub}
    out.append(case("reach: rectangles at every phase", lows, finals, sub=sub, path="lds", phases=len(phases)))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# batch_chunks
# ---------------------------------------------------------------------------------------------------------------------------------
CHUNK_COUNTS = (SEAM_BATCH, SEAM_BATCH + 1, 2 * SEAM_BATCH + 1)


def batch_chunks():
    rng = np.random.default_rng(104)
    out = []
    for n in CHUNK_COUNTS:
        for x0, path in ((0, "lds"), (4, "tables_batch")):
            lows, finals = [], []
            for i in range(n):
                w, h = 9 + (7 * i) % 23, 5 + (5 * i) % 13  # smaller than one tile
                if i == SEAM_BATCH + 0 and n > SEAM_BATCH:  # the largest image leads the second chunk: several tiles of either kernel
                    w, h = 1100, 70
                elif i == 2:  # several tiles in the first chunk too, of other sizes
                    w, h = 530, 40
                low = low_mask(rng, 2 + i % 4, 2 + (3 * i) % 5, grey=i % 5 == 0)
                if w > TILE_W:  # the multi-tile images: a low mask that keeps a 0 and a 255 after dilation, unlike image i - 16's
                    low = low_mask(rng, 5 + i % 3, 8 + i % 5)
                    low[0, 0], low[-3:, -3:] = 255, 0
                lows.append(low)
                finals.append(framed(final_mask(rng, h, w), x0, 0))
            largest = int(np.argmax([f.w * f.h for f in finals]))
            out.append(case(f"chunks n={n} x0={x0}", lows, finals, path=path, n=n, largest=largest,
                            chunks=-(-n // SEAM_BATCH)))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# sub_tables
# ---------------------------------------------------------------------------------------------------------------------------------
def sub_tables():
    rng = np.random.default_rng(105)
    lows, finals, sub = [], [], []
    fw, fh = 131, 47
    for x0 in (0, 4, 52):
        for y0 in (0, 1, fh - 1):
            w = min(fw - x0, (13, 22, 79)[len(lows) % 3])  # no multiple of 4
            h = min(fh - y0, 1 + 6 * (len(lows) % 4))
            lows.append(low_mask(rng, 7, 11, grey=True))
            finals.append(framed(final_mask(rng, h, w), 4, 1))
            sub.append((fw, fh, x0, y0))
    # a rectangle that ends on the full mask's last column and row
    lows.append(low_mask(rng, 7, 11))
    finals.append(framed(final_mask(rng, 20, fw - 100), 4, 0))
    sub.append((fw, fh, 100, fh - 20))
    out = [case("sub on tables: views at x0 = 4", lows, finals, sub=sub, path="tables_batch", ends_on_corner=len(lows) - 1)]
    # the same rectangles in whole buffers, pushed to the tables by a batch over the LDS budget
    lows2 = lows + [low_mask(rng, 50, 700)]
    finals2 = [Final(f.array) for f in finals] + [Final(final_mask(rng, 20, 200))]
    sub2 = sub + [(350, 25, 100, 3)]
    c = case("sub on tables: over the budget", lows2, finals2, sub=sub2, path="tables_batch")
    c["facts"]["lds_bytes"] = lds_bytes(c)
    out.append(c)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# borders
# ---------------------------------------------------------------------------------------------------------------------------------
def borders():
    rng = np.random.default_rng(106)
    out = []
    ones = lambda h, w: np.full((h, w), 255, np.uint8)  # noqa: E731
    for sh, sw, dh, dw in ((1, 7, 9, 50), (7, 1, 50, 9), (1, 1, 6, 11), (2, 2, 13, 21), (5, 6, 1, 1), (1, 1, 1, 1)):
        out.append(case(f"border {sw}x{sh}->{dw}x{dh}", [low_mask(rng, sh, sw, grey=True) | (128 if sh * sw == 1 else 0)], [ones(dh, dw)],
                        batch=False, path="lds"))
    # a lone 255 in every corner and on every edge of a 9 x 12 low mask; 9 x 12 -> 45 x 1100: three tiles across, windows cut the mask
    sh, sw = 9, 12
    for y, x in ((0, 0), (0, sw - 1), (sh - 1, 0), (sh - 1, sw - 1), (0, 5), (sh - 1, 5), (4, 0), (4, sw - 1), (4, 5)):
        low = np.zeros((sh, sw), np.uint8)
        low[y, x] = 255
        out.append(case(f"lone 255 at {y},{x}", [low], [ones(45, 1100)], batch=False, path="lds",
                        dilated=(slice(max(y - 1, 0), y + 2), slice(max(x - 1, 0), x + 2))))
    low = ones(sh, sw)
    low[4, 5] = 0
    out.append(case("lone 0", [low], [ones(45, 1100)], batch=False, path="lds", all_255=True))  # dilation fills a lone 0
    low[3:6, 4:7] = 0
    out.append(case("lone 0 after dilation", [low], [ones(45, 1100)], batch=False, path="lds"))
    # other values in both masks
    low = np.full((4, 5), 0x5a, np.uint8)
    low[1, 1] = 0x3c
    fin = np.full((31, 44), 0xa5, np.uint8)
    fin[:, ::3] = 0x0f
    out.append(case("0x5a AND 0xa5", [low], [fin], batch=False, path="lds", values={0x5a & 0xa5, 0x5a & 0x0f}))
    for x0, path in ((4, "single_4px"), (3, "single_1px")):
        out.append(case(f"0x5a AND 0xa5 at x0={x0}", [low], [framed(fin, x0, 1)], batch=False, path=path, values={0x5a & 0xa5, 0x5a & 0x0f}))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# ties and knife edges
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fused_coeff(v, src_n, dst_n):
    """numpy_resize.coeff with scale * (v + 0.5) - 0.5 rounded ONCE (a fused multiply-subtract), by exact fractions"""
    scale = 1.0 / (float(dst_n) / float(src_n))
    fval = float(Fraction(scale) * Fraction(float(v) + 0.5) - Fraction(1, 2))
    ival = math.floor(fval)
    if ival >= 0 and src_n > 1:
        if ival < src_n - 1:
            return ival, int(round((fval - float(ival)) * 256.0)), True
        return src_n - 1, 0, False
    return 0, 0, False


def half_up_coeff(v, src_n, dst_n):
    """numpy_resize.coeff with the fraction * 256 rounded half up"""
    o, c1, inner = NR.coeff(v, src_n, dst_n)
    if inner:
        scale = 1.0 / (float(dst_n) / float(src_n))
        fval = scale * (float(v) + 0.5) - 0.5
        c1 = int(math.floor((fval - float(o)) * 256.0 + 0.5))
    return o, c1, inner


def tie_columns(src_n, dst_n):
    """interior destination indices whose fraction * 256 is exactly k + 1/2 in the contract's doubles"""
    scale = 1.0 / (float(dst_n) / float(src_n))
    v = np.arange(dst_n, dtype=np.float64)
    f = scale * (v + 0.5) - 0.5
    i = np.floor(f)
    t = (f - i) * 256.0
    inner = (i >= 0) & (i < src_n - 1)
    return np.flatnonzero(inner & (t - np.floor(t) == 0.5))


def knife_columns(src_n, dst_n):
    """destination indices where fraction * 256 lies within 1e-9 of k + 1/2 and the fused evaluation gives another weight"""
    scale = 1.0 / (float(dst_n) / float(src_n))
    v = np.arange(dst_n, dtype=np.float64)
    f = scale * (v + 0.5) - 0.5
    t = (f - np.floor(f)) * 256.0
    near = np.flatnonzero(np.abs(t - np.floor(t) - 0.5) < 1e-9)
    return [int(k) for k in near if fused_coeff(int(k), src_n, dst_n) != NR.coeff(int(k), src_n, dst_n)]


TIES = ((2, 512), (3, 768), (4, 1024))
KNIVES = ((3, 1280, 222), (3, 3328, 565), (2, 1536, 388))  # (src, dst, a column where a fused multiply-subtract changes the weight)


def more_knives(limit=3):
    """a few more, by search: sources of 4 .. 9 samples, destinations of 128 k"""
    found = []
    for src in range(4, 10):
        for dst in range(128, 4097, 128):
            cols = [k for k in knife_columns(src, dst) if NR.coeff(k, src, dst)[0] + 2 <= src - 1]
            if cols and dst % src:
                found.append((src, dst, cols[0]))
                break
        if len(found) == limit:
            break
    return found


def edge_line(src_n, o, dilated):
    """a line of src_n samples that is 0 up to sample o and 255 from o + 1 on — after dilation, if `dilated` (needs o + 2 < src_n)"""
    line = np.zeros(src_n, np.uint8)
    line[o + (2 if dilated else 1):] = 255
    return line


def coefficient_cases(kind):
    """-> (src, dst, column, axis) for the ties or the knife edges: across ("x") and, transposed, down ("y")"""
    sizes = [(s, d, int(tie_columns(s, d)[0])) for s, d in TIES] if kind == "ties" else list(KNIVES) + more_knives()
    return [(s, d, c, axis) for s, d, c in sizes for axis in ("x", "y")]


def coefficient_image(src_n, dst_n, col, axis, channels=1):
    """-> (source image, (dw, dh)): the edge line across 3 rows (or down 3 columns): the named column lies between a 0 and a 255"""
    o = NR.coeff(col, src_n, dst_n)[0]
    img = np.repeat(edge_line(src_n, o, False)[None, :], 3, axis=0)
    img = img if axis == "x" else img.T.copy()
    if channels == 3:
        img = np.stack([img, 255 - img, img // 2], axis=2)
    return np.ascontiguousarray(img), ((dst_n, 5) if axis == "x" else (5, dst_n))


def coefficient_masks(kind):
    """seam-mask cases on every path a call can take for them: whole buffers (lds), views at 4 (single_4px) and 3 (single_1px), and
    batches (lds, tables_batch).  Two-sample sources are constant after dilation: they run, but only sources of three samples or more
    show their column (facts: visible)."""
    out = []
    for src_n, dst_n, col, axis in coefficient_cases(kind):
        o = NR.coeff(col, src_n, dst_n)[0]
        visible = o + 2 <= src_n - 1
        line = edge_line(src_n, o, True) if visible else edge_line(src_n, o, False)
        low = np.repeat(line[None, :], 4, axis=0)
        fin = np.full((9, dst_n), 255, np.uint8)
        if axis == "y":
            low, fin = low.T.copy(), fin.T.copy()
        facts = {"column": col, "axis": axis, "visible": visible, "src": src_n, "dst": dst_n}
        for x0, path in ((0, "lds"), (4, "single_4px"), (3, "single_1px")):
            out.append(case(f"{kind} {src_n}->{dst_n} {axis} x0={x0}", [low], [framed(fin, x0, 1) if x0 else Final(fin)], batch=False, path=path, **facts))
        for x0, path in ((0, "lds"), (4, "tables_batch")):
            out.append(case(f"{kind} {src_n}->{dst_n} {axis} batch x0={x0}", [low, low[::-1, ::-1].copy()],
                            [framed(fin, x0, 0) if x0 else Final(fin), Final(fin)], path=path, **facts))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# image resize: the batch kernel's flat tile list
# ---------------------------------------------------------------------------------------------------------------------------------
def image_batches():
    """-> list of (name, sources, sizes, facts): sources are (parent, x, y, w, h) views of 1- and 3-channel images"""
    rng = np.random.default_rng(107)

    def src(h, w, c, view=False):
        shape = (h + 3, w + 5) if view else (h, w)
        a = rng.integers(0, 256, shape + ((3,) if c == 3 else ()), dtype=np.uint8)
        return (a, 3, 2, w, h) if view else (a, 0, 0, w, h)

    out = []
    sizes = [(dw, dh) for dw in (RESIZE_TW, RESIZE_TW + 1, 2 * RESIZE_TW) for dh in (RESIZE_TH, RESIZE_TH + 1)]
    out.append(("tile edges", [src(3 + k, 5 + 2 * k, 1 + 2 * (k % 2)) for k in range(len(sizes))], sizes, {"tiles": [(-(-w // RESIZE_TW)) * (-(-h // RESIZE_TH)) for w, h in sizes]}))
    for n in (1, 2, 3, 17, 40):
        srcs, sz = [], []
        for i in range(n):
            srcs.append(src(2 + i % 5, 3 + i % 7, 1 + 2 * (i % 2), view=i % 3 == 2))
            sz.append((1, 1) if i % 3 == 1 else (70 + 13 * (i % 4), 5 + i % 6))  # a 1 x 1 destination between two multi-tile ones
        out.append((f"{n} images", srcs, sz, {"n": n}))
    return out


def source_array(s):
    a, x, y, w, h = s
    return a[y:y + h, x:x + w]


SEAM_FAMILIES = {"view_offsets": view_offsets, "lds_budget": lds_budget, "window_reach": window_reach, "batch_chunks": batch_chunks,
                 "sub_tables": sub_tables, "borders": borders, "ties": lambda: coefficient_masks("ties"),
                 "knife_edges": lambda: coefficient_masks("knife_edges")}


def want(c, seam_resize=NR.seam_resize):
    """the contract's results of a case"""
    return [seam_resize(low, f.array, None if c["sub"] is None else c["sub"][i]) for i, (low, f) in enumerate(zip(c["lows"], c["finals"]))]
