"""Constructed cameras and rectangles for the warp (csrc/stx_warp.hip: warp_fast_kernel and, for what it refuses, warp_kernel): every
family is built to put the samples of chosen wavefronts on one sampling path of the tuned kernel, or on the threshold between two, and
returns the facts that make it do so.  Pure numpy, no GPU and no product code: tests/test_constructed_warps.py asserts the facts
against the maps of tests/numpy_warper.py and against the oracle, and shows that the families tell the contract from one-mistake
variants of it; tests/test_gpu_constructed_warps.py runs the same cases on the device.

A case is (warper_type, scale, K, R, source, rect, facts) — it iterates as these seven — plus its name, family and remap model.
`facts` is stated from the construction alone: for the plane cases from exact arithmetic on the camera's entries, never from a map.

The plane construction.  With the plane warper, scale = 1, R = I and K = [[ax, bx, ox], [ay, by, oy], [0, 0, 1]] a destination pixel
(col, row) maps to x = ax col + bx row + ox, y = ay col + by row + oy with z = 1.  Every entry is a multiple of 2^-12 pixel small
enough for the fp32 sums to be exact, so the construction knows s = cvRound(32 v) of every sample as an integer (`Axis.s`).
"""
import math

import numpy as np

# Constants of the kernel the families are shaped around.  tests/test_constructed_warps.py reads each of them back from the source.
LANES = 64            # WARP_FW: columns of a wavefront of the tuned kernel, one lane each ...
ROWS = 4              # ... WARP_TH rows (x WARP_IT = 1 blocks of them) one below the other in every lane
BATCH = 8             # WARP_BATCH: images of one launch
RND_U0 = 0x4B400000   # bit pattern of 1.5 * 2^23: fl(32 v + 1.5 * 2^23) has the pattern RND_U0 + cvRound(32 v) for |32 v| < 2^22
PERIODIC_LIMIT = 1 << 21   # |s| below it: the periodic path
ROUND_LIMIT = 1 << 22      # |32 v| from here on the pattern is no longer RND_U0 + cvRound(32 v)
S16_MIN, S16_MAX = -32768, 32767   # remap's saturate_cast<short> of the pixel part s >> 5
Z_MIN_BITS, Z_MAX_BITS = 0x21800000, 0x5D800000   # 2^-60, 2^60: |z| inside shares one reciprocal between x / z and y / z
NUM_MAX = 2.0 ** 60   # numerators up to here may take the shared reciprocal
NUM_BOUND = 2.0 ** 59   # the host's bound on the numerators (num_ok)
TUNED_MAX = 32767     # sources of 2 .. 32767 columns and rows take the tuned kernel (fast_ok)

INTERIOR, MIRROR, PERIODIC, GENERIC, OTHER = 0, 1, 2, 3, 4   # OTHER: the fp32 remap models' one class beside INTERIOR
CLASS_NAMES = ("interior", "mirror", "periodic", "generic", "other")
Z_ONE, EASY, FDIV = 0, 1, 2
DIV_NAMES = ("z_one", "easy", "fdiv")

RECT_W, RECT_H = 3 * LANES, 2 * ROWS   # three wavefront columns, two row blocks
AFFINE_SHIFT = (16, 8)   # the translation of the affine cases' H
SW, SH = 331, 9


def interior_hi(n):
    """the largest s whose four taps are inside a source of n pixels: s >> 5 <= n - 2"""
    return 32 * (n - 1) - 1


def interior_lo(model="q15"):
    """the fp32 models sample at floor(v), which is s >> 5 or one less: their interior starts one pixel further in"""
    return 0 if model == "q15" else 32


def zone(n):
    """(lowest, highest) s at most one mirror image away from a source of n pixels and inside int16"""
    return max(-32 * n, S16_MIN * 32), min(64 * n - 33, S16_MAX * 32 + 31)


def mask_hi32(n):
    """the nearest-neighbour sample is inside for -16 <= 32 v < this (fp32): cvRound(v) <= n - 1, the tie n - 1/2 goes to even"""
    v = np.float32(n - 0.5)
    return np.float32(32) * (v if (n - 1) & 1 else np.nextafter(v, np.float32(3e38)))


# ---------------------------------------------------------------------------------------------------------------------------------
# classification
# ---------------------------------------------------------------------------------------------------------------------------------
def pattern(v):
    """bit pattern of fl(32 v + 1.5 * 2^23), one rounding (the kernel's fused multiply-add)"""
    with np.errstate(invalid="ignore", over="ignore"):
        t = (np.asarray(v, np.float32).astype(np.float64) * 32.0 + 12582912.0).astype(np.float32)
    return t.view(np.uint32).astype(np.int64)


def _grid(px, reduce):
    """per-pixel values of a rectangle -> [block row][wavefront column][lane], the rows of a lane reduced; lanes beyond the width hold
    the last column, rows beyond the height the last row (they take part in the ballots)"""
    h, w = px.shape
    nby, nbx = -(-h // ROWS), -(-w // LANES)
    rows, cols = np.minimum(np.arange(nby * ROWS), h - 1), np.minimum(np.arange(nbx * LANES), w - 1)
    return reduce(px[rows][:, cols].reshape(nby, ROWS, nbx, LANES), axis=1)


def _classes(in_int, in_zone, in_per, model):
    if model != "q15":
        return np.where(in_int, INTERIOR, OTHER)
    return np.where(in_int, INTERIOR, np.where(in_zone, MIRROR, np.where(in_per, PERIODIC, GENERIC)))


def _waves(px):
    lanes = _grid(px, np.max)
    return lanes.max(axis=2), lanes, px


def classify(xmap, ymap, sw, sh, model="q15"):
    """The path the kernel's tests select, from the maps: (class of every 64 x 4 wavefront [block row][wavefront column], class of every
    lane [block row][wavefront column][lane], class of every pixel).  A wavefront has the highest class among its lanes, a lane the
    highest among its rows.  The tests are the kernel's: unsigned ranges of the patterns."""
    ux, uy = pattern(xmap), pattern(ymap)
    lo = RND_U0 + interior_lo(model)
    in_int = (ux >= lo) & (ux <= RND_U0 + interior_hi(sw)) & (uy >= lo) & (uy <= RND_U0 + interior_hi(sh))
    (xl, xh), (yl, yh) = zone(sw), zone(sh)
    in_zone = (ux >= RND_U0 + xl) & (ux <= RND_U0 + xh) & (uy >= RND_U0 + yl) & (uy <= RND_U0 + yh)
    in_per = (np.minimum(ux, uy) >= RND_U0 - PERIODIC_LIMIT) & (np.maximum(ux, uy) < RND_U0 + PERIODIC_LIMIT)
    return _waves(_classes(in_int, in_zone, in_per, model))


def classify_s(sx, sy, sw, sh, model="q15"):
    """classify() from the integers s = cvRound(32 v) a construction knows (any magnitude), without a float"""
    def rng(s, lo, hi):
        return (s >= lo) & (s <= hi)
    in_int = rng(sx, interior_lo(model), interior_hi(sw)) & rng(sy, interior_lo(model), interior_hi(sh))
    in_zone = rng(sx, *zone(sw)) & rng(sy, *zone(sh))
    in_per = rng(sx, -PERIODIC_LIMIT, PERIODIC_LIMIT - 1) & rng(sy, -PERIODIC_LIMIT, PERIODIC_LIMIT - 1)
    return _waves(_classes(in_int, in_zone, in_per, model))


def _bits(a):
    return np.asarray(a, np.float32).view(np.int32).astype(np.int64)


def host_flags(kind, scale, k_rinv, t, rect):
    """(num_ok, z_one) as the host setup proves them from the camera and the rectangle (fill_warpk)"""
    kr = np.asarray(k_rinv, np.float32).astype(np.float64).reshape(9)
    t = np.zeros(3) if t is None else np.asarray(t, np.float32).astype(np.float64)
    x0, y0, w, h = rect
    sc = abs(float(np.float32(scale)))
    ok = bool(np.isfinite(sc) and sc > 1e-30 and np.isfinite(kr).all() and np.isfinite(t).all())
    umax, vmax = max(abs(x0), abs(x0 + w)) / max(sc, 1e-30), max(abs(y0), abs(y0 + h)) / max(sc, 1e-30)
    bx = by = bz = 1.0001
    if kind == "spherical":
        ok = ok and umax < 5e5 and vmax < 5e5
    elif kind == "cylindrical":
        ok, by = ok and umax < 5e5, vmax * 1.0001
    else:
        bx, by, bz = (umax + abs(t[0])) * 1.0001, (vmax + abs(t[1])) * 1.0001, (1.0 + abs(t[2])) * 1.0001
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(2):
            ok = ok and bool(abs(kr[3 * r]) * bx + abs(kr[3 * r + 1]) * by + abs(kr[3 * r + 2]) * bz <= NUM_BOUND)
    c8 = np.float32(k_rinv[2][2]) * (np.float32(1) - np.float32(t[2]))
    z_one = ok and kind in ("plane", "affine") and kr[6] == 0 and kr[7] == 0 and c8 == np.float32(1)
    return bool(ok), bool(z_one)


def classify_division(kind, X, Y, Z, num_ok, z_one):
    """The division sequence in front of the sampling, from the numerators and the denominator of every pixel: (wavefronts
    [block row][wavefront column][3] holding at least one lane of z_one / easy / fdiv, class of every lane).  A lane decides for
    its four rows together; z_one holds for a whole image."""
    if z_one:
        lanes = _grid(np.zeros(np.shape(Z), np.int64), np.max)
    else:
        zb = _bits(Z) & 0x7FFFFFFF if kind in ("plane", "affine") else _bits(Z)
        easy = (_grid(zb, np.min) >= Z_MIN_BITS) & (_grid(zb, np.max) <= Z_MAX_BITS)
        if not num_ok:
            easy &= _grid(np.fmax(np.abs(X), np.abs(Y)), np.fmax.reduce) <= np.float32(NUM_MAX)
        lanes = np.where(easy, EASY, FDIV)
    return np.stack([(lanes == c).any(axis=2) for c in (Z_ONE, EASY, FDIV)], axis=2), lanes


# ---------------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------------
_sources = {}


def source(sw, sh):
    """uniform random bytes: neighbouring pixels differ, so a tap taken one pixel off shows"""
    if (sw, sh) not in _sources:
        a = np.random.default_rng(1000 * sw + sh).integers(0, 256, (sh, sw, 3), dtype=np.uint8)
        a.setflags(write=False)
        _sources[(sw, sh)] = a
    return _sources[(sw, sh)]


class Case:
    def __init__(self, name, family, warper_type, scale, K, R, size, rect, facts, model="q15"):
        self.name, self.family, self.warper_type, self.scale, self.model = name, family, warper_type, float(scale), model
        self.K, self.R = np.ascontiguousarray(K, np.float32), np.ascontiguousarray(R, np.float32)
        self.size, self.rect, self.facts = tuple(size), tuple(int(v) for v in rect), facts

    @property
    def source(self):
        return source(*self.size)

    def __iter__(self):
        return iter((self.warper_type, self.scale, self.K, self.R, self.source, self.rect, self.facts))

    def with_(self, name, family=None, **kw):
        c = Case(name, family or self.family, self.warper_type, self.scale, self.K, self.R, self.size, self.rect, dict(self.facts), self.model)
        for k, v in kw.items():
            setattr(c, k, v)
        return c


class Axis:
    """v = a col + b row + o, in pixels, every term a multiple of 2^-12"""

    def __init__(self, a, b, o):
        self.a, self.b, self.o = float(a), float(b), float(o)
        assert all(v * 4096 == int(v * 4096) for v in (self.a, self.b, self.o)), (a, b, o)

    def v(self, rect):
        x0, y0, w, h = rect
        return self.a * np.arange(x0, x0 + w, dtype=np.float64)[None, :] + self.b * np.arange(y0, y0 + h, dtype=np.float64)[:, None] + self.o

    def s(self, rect):
        """cvRound(32 v), exact (float64 holds these sums exactly; rint rounds half to even)"""
        return np.rint(32.0 * self.v(rect)).astype(np.int64)


def still(n, along_cols, at=None):
    """the axis a family is not about: inside the interior of n pixels (of the fp32 models' too), moving by a few 1/32"""
    at = (1.25 if n > 3 else 1.0 / 32 + (0 if n == 2 else 1)) if at is None else at
    return Axis(2.0 ** -10, 2.0 ** -11, at) if along_cols else Axis(0, 2.0 ** -10, at)   # (both terms: K stays regular)


def plane_case(name, family, size, ax, ay, rect=(0, 0, RECT_W, RECT_H), model="q15", warper_type="plane", **facts):
    """the plane (or affine, H = I) camera of two axes; facts: what the integers say"""
    K = [[ax.a, ax.b, ax.o], [ay.a, ay.b, ay.o], [0, 0, 1]]
    sx, sy = ax.s(rect), ay.s(rect)
    waves, lanes, px = classify_s(sx, sy, size[0], size[1], model)
    facts = dict(facts, sx=sx, sy=sy, waves=waves, lanes=lanes, pixels=px, division={"z_one"})
    R = np.eye(3)
    if warper_type == "affine":
        # AffineWarper takes the 3 x 3 affine H in R's place and hands the plane warper T = -(h02, h12, 0): u' - t0 = col + h02.  The
        # translation is taken out of the rectangle again, so the samples are the plane case's and the column table holds a t0
        R = np.array([[1, 0, AFFINE_SHIFT[0]], [0, 1, AFFINE_SHIFT[1]], [0, 0, 1]], np.float64)
        rect = (rect[0] - AFFINE_SHIFT[0], rect[1] - AFFINE_SHIFT[1], rect[2], rect[3])
    return Case(name, family, warper_type, 1.0, K, R, size, rect, facts, model)


def _major(size, axis):
    """(n of the axis a family is about, the source with that axis along `axis`): the y families transpose source and camera"""
    return size[0], (tuple(size) if axis == "x" else (size[1], size[0]))


def _axes(axis, major, n_minor):
    """the family's axis moves along the lanes in both constructions; the other one rests"""
    return (major, still(n_minor, False)) if axis == "x" else (still(n_minor, True), major)


def limits(n, model="q15"):
    """name -> (side the far values lie on, s on the limit, s one past it) for an axis of n pixels"""
    zl, zh = zone(n)
    L = {"interior_lo": (-1, interior_lo(model), interior_lo(model) - 1), "interior_hi": (+1, interior_hi(n), interior_hi(n) + 1)}
    if model != "q15":
        return L
    L.update({"zone_lo": (-1, zl, zl - 1), "zone_hi": (+1, zh, zh + 1),
              "periodic_hi": (+1, PERIODIC_LIMIT - 1, PERIODIC_LIMIT), "periodic_lo": (-1, -PERIODIC_LIMIT, -PERIODIC_LIMIT - 1),
              "pixel_hi": (+1, S16_MAX * 32 + 31, (S16_MAX + 1) * 32), "pixel_lo": (-1, S16_MIN * 32, S16_MIN * 32 - 1),
              "round_hi": (+1, ROUND_LIMIT - 1, ROUND_LIMIT), "round_lo": (-1, -ROUND_LIMIT, -ROUND_LIMIT - 1)})
    return L


# where the one sample sits: (name, rectangle width, its column, its row).  A plane map is monotonic along both axes of a rectangle,
# so the one sample beyond a limit is a corner of the rectangle: lane 0 or lane 63 of a corner wavefront, in row 0 of the first block
# or row 3 of the last, or — "lane 31" — the last column of a rectangle that ends in the middle of a wavefront, whose lanes 32 .. 63
# then compute on that column too.
PLACES = (("lane0_row0", RECT_W, 0, 0), ("lane63_row3", RECT_W, RECT_W - 1, RECT_H - 1), ("lane31_row0", RECT_W - 32, RECT_W - 33, 0),
          ("lane0_row3", RECT_W, 0, RECT_H - 1))


def one_sample(name, family, size, axis, side, s_target, place, model="q15", warper_type="plane", height=RECT_H, width=None):
    """step 1 pixel per column and per row, the sample of `place` at s_target and every other sample further to the near side"""
    n, size = _major(size, axis)
    _, w, tc, tr = place
    if width is not None:
        w, tc = width, (width - 1 if tc else 0)
    tr = height - 1 if tr else 0
    a = side * (1 if tc else -1)
    b = side * (1 if tr else -1)
    major = Axis(a, b, s_target / 32.0 - a * tc - b * tr)
    ax, ay = _axes(axis, major, size[1] if axis == "x" else size[0])
    return plane_case(name, family, size, ax, ay, (0, 0, w, height), model, warper_type, axis=axis, target=(tc, tr), s_target=s_target)


def family_thresholds(model="q15", warper_type="plane", family="thresholds", size=(SW, SH), names=None, places=PLACES):
    """1. every limit of the chain, one sample on it and one sample 1/32 past it, the sample alone in its wavefront"""
    out = []
    for axis in "xy":
        for lim, (side, on, past) in limits(size[0], model).items():
            if names and lim not in names:
                continue
            for place in places:
                for what, s in (("on", on), ("past", past)):
                    out.append(one_sample(f"{family}-{model}-{warper_type}-{size[0]}-{axis}-{lim}-{what}-{place[0]}", family, size, axis, side, s,
                                          place, model, warper_type))
        if model == "q15" and not names:
            for s in (10 ** 7, -10 ** 7, 10 ** 9, -10 ** 9):   # far beyond the rounding pattern: generic, and 1e9 is still an int
                out.append(one_sample(f"{family}-{model}-{warper_type}-{size[0]}-{axis}-far{s:+.0e}", family, size, axis, 1 if s > 0 else -1, s,
                                      PLACES[1], model, warper_type))
    return out


def family_phases(model="q15", warper_type="plane", family="phases", size=(SW, SH)):
    """1, second set: step 33/32 along the lanes and 5/32 along the rows, the limit crossed in the middle wavefront: every sub-pixel
    phase on both sides of it.  Third set: step 1, offset 1/64: 32 v is a tie in every column, of both parities from row to row"""
    out = []
    for axis in "xy":
        n, sz = _major(size, axis)
        for lim, (side, on, _) in limits(n, model).items():
            for kind, a, b, o in (("phases", 33 / 32, 5 / 32, 0.0), ("ties", 1.0, 1 / 32, 1 / 64)):
                major = Axis(a, b, on / 32.0 + o - a * (RECT_W // 2))
                ax, ay = _axes(axis, major, sz[1] if axis == "x" else sz[0])
                out.append(plane_case(f"{family}-{model}-{warper_type}-{axis}-{lim}-{kind}", family, sz, ax, ay, model=model,
                                      warper_type=warper_type, axis=axis, ties=kind == "ties"))
    return out


def family_edge_taps(model="q15", warper_type="plane", family="edge_taps"):
    """2. both taps on the edge pixel: -1.5 .. 0.5 and n - 1.5 .. n + 0.5 in steps of 1/32 (and three pixels more to the left)"""
    out = []
    for n in (2, 3, 331):
        for axis in "xy":
            _, sz = _major((n, SH), axis)
            for edge, at in (("low", 0), ("high", n)):
                major, other = Axis(1 / 32, 0, at - 4.5), Axis(0, 1, 0.25)   # the other axis: rows 0 .. 7 of the nine, inside
                ax, ay = (major, other) if axis == "x" else (other, major)
                out.append(plane_case(f"{family}-{model}-{warper_type}-{n}-{axis}-{edge}", family, sz, ax, ay, model=model,
                                      warper_type=warper_type, axis=axis, n=n))
    return out


PERIOD_N = (2, 3, 5, 41, 331, 16385, 32767)   # 41: the smallest n whose quotient estimate is ever off (one too low, on a multiple)


def family_periods(family="periods"):
    """3. step 2 n pixels: every column on a multiple of the period of BORDER_REFLECT, 1/32 before, on and 1/32 behind it.  192 columns
    from -96 where they stay below 65 536 pixels (the periodic path); for the two long sources three columns do, and the 192 are
    the generic path"""
    out = []
    for n in PERIOD_N:
        sh = 2 if n == 32767 else 3 if n == 16385 else SH
        for axis in ("xy" if n in (331, 32767) else "x"):
            _, sz = _major((n, sh), axis)
            for off in (-1, 0, 1):
                rects = [(-96, 0, RECT_W, RECT_H)] + ([(-1, 0, 3, RECT_H)] if n > 331 else [])
                # n = 41: also half a period further, where the reduced position is a multiple of the period and the first quotient
                # estimate of columns 9 .. 95 comes out one too low
                for rect, half in [(r, 0) for r in rects] + ([(rects[0], n)] if n == 41 else []):
                    major = Axis(2 * n, 0, half + off / 32)
                    ax, ay = _axes(axis, major, sh)
                    out.append(plane_case(f"{family}-{n}-{axis}-{off:+d}-w{rect[2]}" + ("-half" if half else ""), family, sz, ax, ay, rect,
                                          axis=axis, n=n, means=PERIODIC if 2 * n * 96 + 1 < 65536 or rect[2] == 3 else GENERIC))
    return out


LONG = ((32767, 2), (16385, 3))


def _sweeps():
    """around +-32768 pixels in steps of 1/32; from 32 768 to 65 535.97 (171.5 pixels a column, 7/32 a row) and mirrored below zero"""
    return (("at+32768", Axis(1 / 32, 0, 32768 - 3)), ("at-32768", Axis(1 / 32, 0, -32768 - 3)),
            ("up", Axis(171.5, 7 / 32, 32768)), ("down", Axis(-171.5, -7 / 32, -32768)))


def family_saturation(family="saturation", sizes=LONG, axes="xy"):
    """4. the pixel part saturates: sources long enough for the mirror zone to end at int16 and not with the source"""
    out = []
    for n, sh in sizes:
        for axis in (axes if n == 32767 or n == 32768 else "x"):
            _, sz = _major((n, sh), axis)
            for name, major in _sweeps():
                ax, ay = _axes(axis, major, sh)
                out.append(plane_case(f"{family}-{n}-{axis}-{name}", family, sz, ax, ay, axis=axis, n=n))
    if family == "saturation":
        for n, sh in sizes:   # the zone's clipped end and the interior's, one sample at a time
            out += family_thresholds(family=family, size=(n, sh), names=("interior_hi", "zone_lo", "zone_hi"), places=PLACES[1:2])
    return out


def family_refused(family="refused"):
    """8. what the tuned kernel refuses: 32 768 columns or rows (beside family 4's 32 767), one column, one row"""
    out = family_saturation(family, ((32768, 2),))
    for sz in ((1, 9), (9, 1)):
        for name, ax, ay in (("sweep", Axis(1 / 32, 0, -3), Axis(0, 1 / 32, -0.125)), ("far", Axis(171.5, 0, -16384), Axis(0, 171.5, -600.25))):
            out.append(plane_case(f"{family}-{sz[0]}x{sz[1]}-{name}", family, sz, ax, ay))
    return out


def family_mask_ties(family="mask_ties"):
    """9. x = k + 1/2 and y = k + 1/2 at both ends of the source, odd and even sizes: the nearest-neighbour test's ties"""
    out = []
    for sz in ((9, 9), (8, 8), (9, 8), (8, 9), (331, 9), (330, 8)):
        ax = Axis(1, 0, 0.5 - 90) if sz[0] < 100 else Axis(1, 0, 0.5 - 1)   # the long ones: low end in one case, high end in the next
        ay = Axis(0, 1, 0.5 - 3)
        rect = (0, 0, RECT_W, 4 * ROWS)
        out.append(plane_case(f"{family}-{sz[0]}x{sz[1]}", family, sz, ax, ay, rect, ends="both" if sz[0] < 100 else "low"))
        if sz[0] >= 100:
            out.append(plane_case(f"{family}-{sz[0]}x{sz[1]}-high", family, sz, Axis(1, 0, sz[0] - 100.5), ay, rect, ends="high"))
    return out


def family_clamped(family="clamped"):
    """11. 37 x 7: lanes 37 .. 63 compute on column 36 and row 3 of the second block on row 6 — with the one sample in that corner,
    all of them are past the limit — or, in the opposite corner, none of them is"""
    out = []
    for axis in "xy":
        for lim in ("interior_lo", "interior_hi", "zone_hi", "periodic_hi"):
            side, on, past = limits(SW)[lim]
            for place in (PLACES[0], PLACES[1]):
                for what, s in (("on", on), ("past", past)):
                    out.append(one_sample(f"{family}-{axis}-{lim}-{what}-{place[0]}", family, (SW, SH), axis, side, s, place, height=7, width=37))
    return out


# --------------------------------------------------------------------------------------------------------------------- division
def _rot(yaw, pitch, roll):
    cy, sy, cx, sx, cz, sz = (f(math.radians(a)) for a in (yaw, pitch, roll) for f in (math.cos, math.sin))
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return (ry @ rx @ rz).astype(np.float32)


def family_division(family="division"):
    """5. the division in front of the sampling.  facts["division"]: the classes the family's wavefronts hold (all of them, and
    no other); facts["z"]: signs of z that occur; facts["nonfinite"]: positions that are Inf / NaN occur"""
    out = []
    f = 300.0
    K = np.array([[f, 0, 165.0], [0, f, 4.5], [0, 0, 1]], np.float32)
    R = _rot(0.9, 0.6, 0.4)
    rect = (-96, -4, RECT_W, RECT_H)
    out.append(Case(f"{family}-plane-rotated", family, "plane", f, K, R, (SW, SH), rect, dict(division={"easy"}, z="+")))
    for e in (-70, 70):   # x, y and z all scale, the quotients do not; |z| leaves [2^-60, 2^60]
        out.append(Case(f"{family}-plane-rotated-2^{e}", family, "plane", f, K, R * np.float32(2.0 ** e), (SW, SH), rect,
                        dict(division={"fdiv"}, z="+", same_maps_as=f"{family}-plane-rotated")))
    # numerators beyond the host's bound with z = 1: proved at run time (2^53 x 96 < 2^60) or not (2^62: only column 0 is small)
    for e, want in ((53, {"easy"}), (62, {"easy", "fdiv"})):
        Kb = np.array([[2.0 ** e, 0, 100.25], [0, 1, 0.25], [0, 0, 1]], np.float32)
        out.append(Case(f"{family}-plane-numerators-2^{e}", family, "plane", 1.0, Kb, np.eye(3), (SW, SH), (-96, 0, RECT_W, RECT_H),
                        dict(division=want, z="+", num_ok=False)))
    # z = g u + h through R^T's third row (g, 0, h): z < 0, z = 0 and z > 0 in one rectangle; the plane warper divides by all of them
    Kz = np.array([[8, 0, 0], [0, 1, 0.25], [0, 0, 1]], np.float32)
    for name, g, h, nonfinite in (("nan", 1 / 64, 0.0, "nan"), ("inf", 1 / 64, 0.5, "inf")):
        Rz = np.array([[1, 0, g], [0, 1, 0], [0, 0, h]], np.float32)
        out.append(Case(f"{family}-plane-z-{name}", family, "plane", 1.0, Kz, Rz, (SW, SH), (-96, 0, RECT_W, RECT_H),
                        dict(division={"easy", "fdiv"}, z="-0+", nonfinite=nonfinite)))
    # the rotation warpers: z <= 0 gives (-1, -1).  scale 50: the 192 columns span +-1.9 rad around the optical axis
    Kr = np.array([[50, 0, 165.0], [0, 50, 4.5], [0, 0, 1]], np.float32)
    for wt in ("spherical", "cylindrical"):
        out.append(Case(f"{family}-{wt}-behind", family, wt, 50.0, Kr, np.eye(3), (SW, SH), (-96, 74 if wt == "spherical" else -4, RECT_W, RECT_H),
                        dict(division={"easy", "fdiv"}, z="-+")))
        out.append(Case(f"{family}-{wt}-behind-2^-70", family, wt, 50.0, Kr, np.eye(3, dtype=np.float32) * np.float32(2.0 ** -70), (SW, SH),
                        (-96, 74 if wt == "spherical" else -4, RECT_W, RECT_H), dict(division={"fdiv"}, z="-+")))
    return out


# ------------------------------------------------------------------------------------------------- the other instantiations
PITCHED_SIZE = (333, 251)
PITCHED_ANGLES = ((20.0, 50.0, 7.0), (-15.0, -50.0, -5.0), (5.0, 50.0, 0.0))   # tests/test_gpu_warp_outputs.py: SHAPES["pitched"]


def pitched_camera(k):
    w, h = PITCHED_SIZE
    K = np.array([[0.75 * w, 0, w / 2.0], [0, 0.75 * w, h / 2.0], [0, 0, 1]], np.float32)
    return 0.75 * w, K, _rot(*PITCHED_ANGLES[k])


# Found by a search over the maps of tests/numpy_warper.py, 512 columns and 128 rows around camera 0's ROI, in steps of one wavefront
# (search() in tests/test_constructed_warps.py is that search, and a test there finds these rectangles with it again): (warper, camera, rectangle, the classes of its 2 x 3 wavefronts, the pairs
# of adjacent classes that lanes of ONE of its wavefronts belong to)
SEARCHED = (
    ("spherical", 0, (-737, 216, 192, 8), [[3, 3, 2], [1, 3, 2]], [(1, 2), (2, 3)]),
    ("spherical", 0, (-737, -72, 192, 8), [[0, 0, 1], [0, 0, 1]], [(0, 1)]),
    ("cylindrical", 0, (-737, -207, 192, 8), [[3, 3, 2], [1, 3, 2]], [(1, 2), (2, 3)]),
    ("cylindrical", 0, (-97, -1067, 192, 8), [[1, 1, 1], [1, 1, 0]], [(0, 1)]),
)


def family_searched(family="searched"):
    out = []
    for wt, cam, rect, waves, pairs in SEARCHED:
        scale, K, R = pitched_camera(cam)
        out.append(Case(f"{family}-{wt}-cam{cam}-{rect[0]}_{rect[1]}", family, wt, scale, K, R, PITCHED_SIZE, rect,
                        dict(waves=np.array(waves), pairs=set(pairs))))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
def build_all():
    cases = []
    cases += family_thresholds() + family_phases()
    cases += family_edge_taps()
    cases += family_periods()
    cases += family_saturation()
    cases += family_division()
    cases += family_searched()
    cases += family_thresholds(warper_type="affine", family="affine_thresholds") + family_phases(warper_type="affine", family="affine_phases")
    cases += family_edge_taps(warper_type="affine", family="affine_edge_taps")
    for m in ("float", "float_fma"):
        cases += family_thresholds(model=m, family="float_thresholds") + family_edge_taps(model=m, family="float_edge_taps")
    cases += family_refused()
    cases += family_mask_ties()
    cases += family_clamped()
    names = [c.name for c in cases]
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    return {c.name: c for c in cases}


def tuned(case):
    """the source is one the tuned kernel takes (fast_ok); else warp_kernel runs, for every image of the case's launch"""
    return 2 <= min(case.size) and max(case.size) <= TUNED_MAX


CASES = build_all()
FAMILIES = sorted({c.family for c in CASES.values()})


def family(name):
    return [c for c in CASES.values() if c.family == name]
