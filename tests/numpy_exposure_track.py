"""The contract of exposure-gain tracking on a known rig (stitching_amd.ExposureTracker, csrc/stx_exposure_track.hip; DESIGN.md
section 25), in numpy.  The device statistics equal `pair_stats` integer for integer, `stitching_amd.exposure_tracking.track_update`
equals `track_update` here in the bits of every float64, the scaled gain maps equal `effective_gains` byte for byte.

Lattice: stride s; the sample points are the panorama pixels (X, Y) with X % s == 0 and Y % s == 0 (Python's %: floor-mod, corners
are often negative).  Image i is warped into the rectangle (x, y, w, h); its warped mask M covers the rectangle; V[Y, X] =
(M[Y - y, X - x] == 255) at the lattice points inside the rectangle (grey values do not count).  A pair job is (a, b), a < b, whose
rectangles intersect — also where the intersection holds no lattice point.  Its statistics are eight integers: c, aB, aG, aR, bB, bG,
bR, rej over the lattice points of both rectangles with V_a & V_b; a sample counts if all six bytes lie in 1 .. 254 (a saturated
product cannot be de-compensated), else it adds 1 to rej.
"""
import numpy as np

from tests import numpy_exposure as NE

KINDS = ("gain", "channel")
DEFAULT_RATE, DEFAULT_LIMITS = 0.25, (0.25, 4.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# lattice, grids, pair jobs
# ---------------------------------------------------------------------------------------------------------------------------------
def lattice_range(x0, x1, s):
    """The lattice indices l with x0 <= l * s < x1, as (first, count); count 0: none."""
    first = -((-x0) // s)  # ceil(x0 / s), floor division of Python
    last = (x1 - 1) // s
    return first, max(0, last - first + 1)


def grid(rect, mask, s):
    """V of one image: a bool array over the lattice points inside rect, (ny, nx) — either may be 0 — and (lx0, ly0)."""
    x, y, w, h = (int(v) for v in rect)
    mask = np.asarray(mask)
    assert mask.shape == (h, w), (mask.shape, rect)
    lx0, nx = lattice_range(x, x + w, s)
    ly0, ny = lattice_range(y, y + h, s)
    v = mask[ly0 * s - y::s, lx0 * s - x::s][:ny, :nx] == 255
    if nx == 0 or ny == 0:
        v = np.zeros((ny, nx), bool)
    return v, (lx0, ly0)


def grids(rects, masks, s):
    """-> ([V_i], [(lx0, ly0)], self counts c_ii (n,) int64)"""
    out = [grid(r, m, s) for r, m in zip(rects, masks)]
    return [g[0] for g in out], [g[1] for g in out], np.array([int(g[0].sum()) for g in out], np.int64)


def pair_jobs(rects):
    """Every (a, b), a < b, whose rectangles intersect, in lexicographic order."""
    out = []
    for a in range(len(rects)):
        ax, ay, aw, ah = rects[a]
        for b in range(a + 1, len(rects)):
            bx, by, bw, bh = rects[b]
            if max(ax, bx) < min(ax + aw, bx + bw) and max(ay, by) < min(ay + ah, by + bh):
                out.append((a, b))
    return out


def pair_stats(rects, vs, origins, imgs, s):
    """-> (J, 8) int64: c, aB, aG, aR, bB, bG, bR, rej of every pair job.  vs, origins: `grids`; imgs: the warped, compensated u8x3
    images of the rectangles."""
    pairs = pair_jobs(rects)
    out = np.zeros((len(pairs), 8), np.int64)
    for j, (a, b) in enumerate(pairs):
        ax, ay, aw, ah = rects[a]
        bx, by, bw, bh = rects[b]
        lx0, nx = lattice_range(max(ax, bx), min(ax + aw, bx + bw), s)
        ly0, ny = lattice_range(max(ay, by), min(ay + ah, by + bh), s)
        if nx == 0 or ny == 0:
            continue

        def cut(i, x, y):
            ox, oy = origins[i]
            v = vs[i][ly0 - oy:ly0 - oy + ny, lx0 - ox:lx0 - ox + nx]
            p = np.asarray(imgs[i])[ly0 * s - y::s, lx0 * s - x::s][:ny, :nx]
            return v, p.astype(np.int64)

        va, pa = cut(a, ax, ay)
        vb, pb = cut(b, bx, by)
        both = va & vb
        six = np.concatenate([pa, pb], axis=2)
        ok = both & ((six >= 1) & (six <= 254)).all(axis=2)
        out[j, 0] = int(ok.sum())
        out[j, 1:4] = pa[ok].sum(axis=0)
        out[j, 4:7] = pb[ok].sum(axis=0)
        out[j, 7] = int((both & ~ok).sum())
    return out


def pair_stats_loop(rects, masks, imgs, s, floor_mod=True, white=True, saturation=True):
    """The same statistics by a loop over every panorama pixel of every intersection, from the masks themselves.  The switches make
    the near variants the contract must tell itself from: floor_mod=False finds the first lattice point of an intersection with C's
    truncating division, white=False counts every non-zero
    mask value, saturation=False counts samples with bytes at 0 or 255."""
    def first(v0):
        """the first lattice coordinate at or after v0: s * ceil(v0 / s) — the wrong variant takes the ceiling by C's truncating division,
        (v0 + s - 1) / s, which is one too many for negative v0 that are no multiple of s"""
        if floor_mod:
            return s * -((-v0) // s)
        return s * int((v0 + s - 1) / s)

    def on_lattice(v, v0):
        return v >= first(v0) and (v - first(v0)) % s == 0

    pairs = pair_jobs(rects)
    out = np.zeros((len(pairs), 8), np.int64)
    for j, (a, b) in enumerate(pairs):
        ax, ay, aw, ah = rects[a]
        bx, by, bw, bh = rects[b]
        for Y in range(max(ay, by), min(ay + ah, by + bh)):
            if not on_lattice(Y, max(ay, by)):
                continue
            for X in range(max(ax, bx), min(ax + aw, bx + bw)):
                if not on_lattice(X, max(ax, bx)):
                    continue
                ma, mb = int(masks[a][Y - ay, X - ax]), int(masks[b][Y - by, X - bx])
                if not ((ma == 255 and mb == 255) if white else (ma != 0 and mb != 0)):
                    continue
                pa = [int(v) for v in imgs[a][Y - ay, X - ax]]
                pb = [int(v) for v in imgs[b][Y - by, X - bx]]
                if saturation and not all(1 <= v <= 254 for v in pa + pb):
                    out[j, 7] += 1
                    continue
                out[j, 0] += 1
                for k in range(3):
                    out[j, 1 + k] += pa[k]
                    out[j, 4 + k] += pb[k]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# update
# ---------------------------------------------------------------------------------------------------------------------------------
def planes_of(kind):
    assert kind in KINDS
    return 3 if kind == "channel" else 1


def plane_means(kind, stats, plane):
    """I'(a,b), I'(b,a) of one plane for every pair (0 where c == 0): float64, one division each"""
    stats = np.asarray(stats, np.int64).reshape(-1, 8)
    ia, ib = np.zeros(len(stats)), np.zeros(len(stats))
    for j, st in enumerate(stats):
        c = int(st[0])
        if c <= 0:
            continue
        if kind == "channel":
            ia[j], ib[j] = float(int(st[1 + plane])) / float(c), float(int(st[4 + plane])) / float(c)
        else:
            ia[j] = float(int(st[1]) + int(st[2]) + int(st[3])) / (3.0 * float(c))
            ib[j] = float(int(st[4]) + int(st[5]) + int(st[6])) / (3.0 * float(c))
    return ia, ib


def track_update(kind, r, pairs, self_counts, stats, rate=DEFAULT_RATE, limits=DEFAULT_LIMITS, decompensate=True, solve=None):
    """One update of the residual gains.  r: (n, planes) float64, the residuals the measured images were made with; pairs: the pair
    jobs; self_counts: c_ii; stats: (J, 8).  -> (r_next (n, planes), info {"solve_failures", "rejected_share"}).
    decompensate=False is the wrong variant without the division by r (a feedback product, for the contract's own test);
    solve: a stand-in for numpy_exposure.single_feed_gains (failure injection)."""
    solve = solve or NE.single_feed_gains
    r = np.array(r, np.float64)
    n, planes = r.shape
    assert planes == planes_of(kind) and 0.0 < rate <= 1.0
    stats = np.asarray(stats, np.int64).reshape(-1, 8)
    lo, hi = float(limits[0]), float(limits[1])
    out = r.copy()
    failures = 0
    for p in range(planes):
        ia, ib = plane_means(kind, stats, p)
        # N, I, skip as numpy_exposure.stats_matrices fills them, from means instead of sums
        N, I, skip = np.zeros((n, n), np.float64), np.zeros((n, n), np.float64), np.ones(n, bool)
        for i in range(n):
            N[i, i] = max(1, int(self_counts[i]))
        for j, (a, b) in enumerate(pairs):
            c = int(stats[j, 0])
            N[a, b] = N[b, a] = max(1, c)
            if c == 0:
                continue
            skip[a] = skip[b] = False
            sa, sb = ia[j], ib[j]
            if decompensate:  # absolute again: what the cameras would show under the plan's gains alone
                sa, sb = sa / r[a, p], sb / r[b, p]
            I[a, b], I[b, a] = sa, sb
        try:
            with np.errstate(all="ignore"):
                star = np.asarray(solve(N, I, skip), np.float64)
            ok = bool(np.isfinite(star).all())
        except (ZeroDivisionError, FloatingPointError, np.linalg.LinAlgError):
            ok = False
        if not ok:
            failures += 1
            continue
        step = r[:, p] + rate * (star - r[:, p])
        out[:, p] = np.minimum(np.maximum(step, lo), hi)
    total = int(stats[:, 0].sum() + stats[:, 7].sum()) if len(stats) else 0
    share = float(int(stats[:, 7].sum())) / float(total) if total > 0 else 0.0
    return out, {"solve_failures": failures, "rejected_share": share}


# ---------------------------------------------------------------------------------------------------------------------------------
# effective gains
# ---------------------------------------------------------------------------------------------------------------------------------
def effective_kind(plan_kind, tracker_kind):
    """The compensator kind that applies plan gains x residuals: blocks stay blocks, three planes on either side make three"""
    three = plan_kind.startswith("channel") or tracker_kind == "channel"
    if plan_kind.endswith("_blocks"):
        return "channel_blocks" if three else "gain_blocks"
    return "channel" if three else "gain"


def effective_gains(plan_kind, plan_gains, r, tracker_kind):
    """-> the gains of effective_kind(...) per image, as ExposureErrorCompensator.set_gains takes them.  plan_gains: None for "no".
    Scalar kinds: float64 P_i * r_i per channel (apply demotes to float32 afterwards); block kinds: float32(map) * float32(r) per
    value — f32x1 when plan and tracker are single-plane, else f32x3."""
    r = np.asarray(r, np.float64)
    n, planes = r.shape
    three = effective_kind(plan_kind, tracker_kind).startswith("channel")
    out = []
    for i in range(n):
        ri = r[i] if planes == 3 else (np.full(3, r[i, 0]) if three else r[i, :1])
        if plan_kind.endswith("_blocks"):
            m = np.asarray(plan_gains[i], np.float32)
            if three and m.ndim == 2:
                m = np.repeat(m[:, :, None], 3, axis=2)
            r32 = ri.astype(np.float32)
            out.append((m * (r32[None, None, :] if three else r32[0])).astype(np.float32))
        else:
            p = np.ones(1) if plan_kind == "no" else np.atleast_1d(np.asarray(plan_gains[i], np.float64)).reshape(-1)
            p = p[:3] if p.size >= 3 else np.full(3 if three else 1, p[0])
            out.append(p * ri)
    return out
