"""Restatement of exposure-gain estimation (ExposureCompensator::feed, OpenCV 4.x modules/stitching/src/exposure_compensate.cpp, and
cv::solve(DECOMP_LU)) in numpy: the contract `stitching_amd.ExposureEstimator` is tested against.

Written from recollection of OpenCV (no OpenCV source or build is at hand): fidelity to real OpenCV is unpinned, as for the rest of the
oracle.  The points least sure are marked (*): the small-matrix branch of cv::solve, its LU, the symmetric small-kernel filter form.

Units are whole images ("gain", "channel") or blocks ("gain_blocks", "channel_blocks").  A pixel counts where BOTH masks are 255.
"""

import numpy as np

ALPHA, BETA = 0.01, 100.0
KINDS = ("gain", "gain_blocks", "channel", "channel_blocks")


# ---------------------------------------------------------------------------------------------------------------------------------
# units
# ---------------------------------------------------------------------------------------------------------------------------------
def block_grid(w, h, bl):
    """-> (bpi_w, bpi_h, bw, bh): blocks per image and block size of a w x h image (BlocksCompensator::feed)."""
    bpw, bph = -(-w // bl), -(-h // bl)
    return bpw, bph, -(-w // bpw), -(-h // bph)


def block_rects(w, h, bl):
    """Block rectangles (x0, y0, x1, y1) of one image, row-major."""
    bpw, bph, bw, bh = block_grid(w, h, bl)
    return [(bx * bw, by * bh, min(bx * bw + bw, w), min(by * bh + bh, h)) for by in range(bph) for bx in range(bpw)]


def make_units(corners, imgs, blocks, bl):
    """-> list of (image index, x0, y0, x1, y1) in image coordinates; image-major, then row-major."""
    out = []
    for i, img in enumerate(imgs):
        h, w = img.shape[:2]
        rects = block_rects(w, h, bl) if blocks else [(0, 0, w, h)]
        out += [(i,) + r for r in rects]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# statistics
# ---------------------------------------------------------------------------------------------------------------------------------
def overlapping_pairs(corners, units):
    """Unit pairs (a, b), a <= b (a == b included), whose rectangles overlap (overlapRoi), in index order."""
    c = np.asarray(corners, np.int64).reshape(-1, 2)
    u = np.asarray(units, np.int64).reshape(-1, 5)
    x0, y0 = c[u[:, 0], 0] + u[:, 1], c[u[:, 0], 1] + u[:, 2]
    x1, y1 = c[u[:, 0], 0] + u[:, 3], c[u[:, 0], 1] + u[:, 4]
    out = []
    for r0 in range(0, len(u), 512):  # 512 rows of the overlap matrix at a time
        r = slice(r0, r0 + 512)
        ov = ((np.maximum(x0[r, None], x0[None, :]) < np.minimum(x1[r, None], x1[None, :])) &
              (np.maximum(y0[r, None], y0[None, :]) < np.minimum(y1[r, None], y1[None, :])))
        a, b = np.nonzero(ov)
        keep = b >= a + r0
        out += list(zip((a[keep] + r0).tolist(), b[keep].tolist()))
    return out, (x0, y0, x1, y1)


def norms(img):
    """Per-pixel norm in fp64: sqrt((double)(b^2 + g^2 + r^2)) for u8x3, the byte for one channel."""
    v = img.astype(np.int64)
    if v.ndim == 3:
        return np.sqrt((v * v).sum(axis=2).astype(np.float64))
    return v.astype(np.float64)


def seq_sum(vals):
    """fp64 sum in order, starting from 0.0 (np.add.accumulate is strictly sequential)."""
    vals = np.ravel(vals)
    return 0.0 if vals.size == 0 else float(np.add.accumulate(np.concatenate([[0.0], vals]))[-1])


def pair_stats(corners, imgs, masks, units, planes):
    """Overlap statistics of one feed.  planes: None (u8x3 norms: the gain kinds) or (0, 1, 2) (channel kinds).
    -> jobs {(a, b): (c, [sum_a per plane], [sum_b per plane])}, list of pairs in index order."""
    pairs, (gx0, gy0, _, _) = overlapping_pairs(corners, units)
    out = {}
    nrm = {}
    for a, b in pairs:
        ia, ib = units[a][0], units[b][0]
        ax0, ay0, ax1, ay1 = (int(gx0[a]), int(gy0[a]), int(gx0[a]) + units[a][3] - units[a][1], int(gy0[a]) + units[a][4] - units[a][2])
        bx0, by0, bx1, by1 = (int(gx0[b]), int(gy0[b]), int(gx0[b]) + units[b][3] - units[b][1], int(gy0[b]) + units[b][4] - units[b][2])
        tx, ty, rx, ry = max(ax0, bx0), max(ay0, by0), min(ax1, bx1), min(ay1, by1)
        ca, cb = corners[ia], corners[ib]
        sa = (slice(ty - ca[1], ry - ca[1]), slice(tx - ca[0], rx - ca[0]))
        sb = (slice(ty - cb[1], ry - cb[1]), slice(tx - cb[0], rx - cb[0]))
        m = (masks[ia][sa] == 255) & (masks[ib][sb] == 255)
        c = int(m.sum())
        if planes is None:
            for i in (ia, ib):
                if i not in nrm:
                    nrm[i] = norms(imgs[i])
            suma = [seq_sum(np.where(m, nrm[ia][sa], 0.0))]
            sumb = [seq_sum(np.where(m, nrm[ib][sb], 0.0))]
        else:
            suma = [int(imgs[ia][sa][..., p][m].astype(np.int64).sum()) for p in planes]
            sumb = [int(imgs[ib][sb][..., p][m].astype(np.int64).sum()) for p in planes]
        out[(a, b)] = (c, suma, sumb)
    return out, pairs


def stats_matrices(m, jobs, plane=0):
    """-> N (m x m), I (m x m), skip (m,) of one plane, as GainCompensator::singleFeed fills them."""
    N = np.zeros((m, m), np.float64)
    I = np.zeros((m, m), np.float64)
    skip = np.ones(m, bool)
    for (a, b), (c, sa, sb) in jobs.items():
        N[a, b] = N[b, a] = max(1, c)
        if c == 0:
            continue
        if a != b:
            skip[a] = skip[b] = False
        I[a, b] = float(sa[plane]) / N[a, b]
        I[b, a] = float(sb[plane]) / N[a, b]
    return N, I, skip


# ---------------------------------------------------------------------------------------------------------------------------------
# assembly and solve
# ---------------------------------------------------------------------------------------------------------------------------------
def assemble(N, I, skip):
    """-> A, b, index of the non-skipped units (rows ki / columns kj in index order)."""
    idx = np.nonzero(~np.asarray(skip, bool))[0]
    m = idx.size
    A = np.zeros((m, m), np.float64)
    b = np.zeros(m, np.float64)
    for ki, i in enumerate(idx):
        row = N[i, idx]
        for kj in np.nonzero(row)[0]:  # N == 0 adds nothing (x + 0.0 == x; A is never -0)
            j = idx[kj]
            n = float(N[i, j])
            b[ki] += BETA * n
            A[ki, ki] += BETA * n
            if j != i:
                A[ki, ki] += 2 * ALPHA * I[i, j] * I[i, j] * n
                A[ki, kj] -= 2 * ALPHA * I[i, j] * I[j, i] * n
    return A, b, idx


def det2(S):
    return S[0, 0] * S[1, 1] - S[0, 1] * S[1, 0]


def det3(S):
    return (S[0, 0] * (S[1, 1] * S[2, 2] - S[1, 2] * S[2, 1]) -
            S[0, 1] * (S[1, 0] * S[2, 2] - S[1, 2] * S[2, 0]) +
            S[0, 2] * (S[1, 0] * S[2, 1] - S[1, 1] * S[2, 0]))


def solve_small(A, b):
    """cv::solve's branch for m <= 3 (*): x = b / a, Cramer's rule with d = 1 / det."""
    m = A.shape[0]
    S, B = [[float(v) for v in r] for r in A], [float(v) for v in b]
    S = np.array(S, dtype=object)  # python floats: IEEE fp64, no fused multiply-add
    if m == 1:
        return np.array([B[0] / S[0, 0]])
    if m == 2:
        d = 1.0 / det2(S)
        t = (B[0] * S[1, 1] - B[1] * S[0, 1]) * d
        x1 = (B[1] * S[0, 0] - B[0] * S[1, 0]) * d
        return np.array([t, x1])
    d = 1.0 / det3(S)
    x0 = d * (B[0] * (S[1, 1] * S[2, 2] - S[1, 2] * S[2, 1]) -
              S[0, 1] * (B[1] * S[2, 2] - S[1, 2] * B[2]) +
              S[0, 2] * (B[1] * S[2, 1] - S[1, 1] * B[2]))
    x1 = d * (S[0, 0] * (B[1] * S[2, 2] - S[1, 2] * B[2]) -
              B[0] * (S[1, 0] * S[2, 2] - S[1, 2] * S[2, 0]) +
              S[0, 2] * (S[1, 0] * B[2] - B[1] * S[2, 0]))
    x2 = d * (S[0, 0] * (S[1, 1] * B[2] - B[1] * S[2, 1]) -
              S[0, 1] * (S[1, 0] * B[2] - B[1] * S[2, 0]) +
              B[0] * (S[1, 0] * S[2, 1] - S[1, 1] * S[2, 0]))
    return np.array([x0, x1, x2])


def lu_solve(A, b, skip_zeros=True):
    """OpenCV's LU with partial pivoting (*), then back substitution.  skip_zeros=False: the dense loop; True: only rows with
    A(j,i) != 0 and columns with A(i,k) != 0 are touched — the same bits (adding alpha * 0 changes no value, A never holds -0)."""
    A, b = np.array(A, np.float64), np.array(b, np.float64)
    m = A.shape[0]
    for i in range(m):
        p = i + int(np.argmax(np.abs(A[i:, i])))  # the first row holding the largest |A(j,i)|
        if p != i:
            A[[i, p], i:] = A[[p, i], i:]
            b[i], b[p] = b[p], b[i]
        d = -1.0 / A[i, i]
        if skip_zeros:
            rows = i + 1 + np.nonzero(A[i + 1:, i])[0]
            cols = i + 1 + np.nonzero(A[i, i + 1:])[0]
        else:
            rows = np.arange(i + 1, m)
            cols = np.arange(i + 1, m)
        if rows.size == 0:
            continue
        alpha = A[rows, i] * d
        if cols.size:
            blk = np.ix_(rows, cols)
            A[blk] = A[blk] + alpha[:, None] * A[i, cols][None, :]
        b[rows] = b[rows] + alpha * b[i]
    for i in range(m - 1, -1, -1):
        cols = i + 1 + (np.nonzero(A[i, i + 1:])[0] if skip_zeros else np.arange(m - i - 1))
        s = b[i]
        if cols.size:
            s = np.subtract.accumulate(np.concatenate([[s], A[i, cols] * b[cols]]))[-1]  # s -= A(i,k) * x(k), k increasing
        b[i] = s / A[i, i]
    return b


def cv_solve(A, b, skip_zeros=True):
    return solve_small(A, b) if A.shape[0] <= 3 else lu_solve(A, b, skip_zeros)


def single_feed_gains(N, I, skip, skip_zeros=True):
    """GainCompensator::singleFeed's solve: gains of all units (skipped ones 1)."""
    m = N.shape[0]
    g = np.ones(m, np.float64)
    if np.all(skip):
        return g
    A, b, idx = assemble(N, I, skip)
    g[idx] = cv_solve(A, b, skip_zeros)
    return g


# ---------------------------------------------------------------------------------------------------------------------------------
# gain-map filter and the whole feed
# ---------------------------------------------------------------------------------------------------------------------------------
def _smooth_axis(m, axis):
    """[0.25, 0.5, 0.25] along one axis, REFLECT_101, fp32 as 0.5f * c + 0.25f * (l + r) (*); length 1: unchanged."""
    n = m.shape[axis]
    if n == 1:
        return m.copy()
    idx = np.arange(n)
    left, right = np.abs(idx - 1), idx + 1
    right[-1] = n - 2
    lv, rv = np.take(m, left, axis=axis), np.take(m, right, axis=axis)
    return (np.float32(0.5) * m + np.float32(0.25) * (lv + rv)).astype(np.float32)


def filter_gain_map(g):
    """BlocksCompensator's sepFilter2D([.25 .5 .25]) applied twice (rows, then columns, each time), fp32, per channel."""
    g = np.asarray(g, np.float32)
    for _ in range(2):
        g = _smooth_axis(_smooth_axis(g, 1), 0)
    return g


def _apply_unit_gains(kind, imgs, units, g_units, bl):
    """Between feeds: every unit multiplied by its own gain (or BGR triple), as cv::multiply rounds (oracle.gain_apply)."""
    out = [np.array(im, copy=True) for im in imgs]
    for u, (i, x0, y0, x1, y1) in enumerate(units):
        g = g_units[:, u] if g_units.ndim == 2 else np.full(3, g_units[u])
        gf = np.asarray(g, np.float64).astype(np.float32)
        v = out[i][y0:y1, x0:x1].astype(np.float32) * gf[None, None, :]
        out[i][y0:y1, x0:x1] = np.clip(np.rint(v), 0, 255).astype(np.uint8)
    return out


def feed(kind, corners, imgs, masks, nr_feeds=1, block_size=32, want_stats=False):
    """The whole ExposureCompensator::feed -> getMatGains() list (shapes as cv2 returns them).  want_stats: also the first feed's
    job statistics (pair_stats)."""
    assert kind in KINDS
    corners = [tuple(int(v) for v in c) for c in corners]
    imgs = [np.asarray(i, np.uint8) for i in imgs]
    masks = [np.asarray(m, np.uint8) for m in masks]
    blocks = kind.endswith("_blocks")
    channels = kind.startswith("channel")
    units = make_units(corners, imgs, blocks, block_size)
    m = len(units)
    nplanes = 3 if channels else 1
    acc = np.ones((nplanes, m), np.float64)
    cur = imgs
    first = None
    for n in range(nr_feeds):
        if n > 0:
            cur = _apply_unit_gains(kind, cur, units, g if channels else g[0], block_size)
        jobs, _ = pair_stats(corners, cur, masks, units, (0, 1, 2) if channels else None)
        if first is None:
            first = jobs
        g = np.empty((nplanes, m), np.float64)
        for p in range(nplanes):
            N, I, skip = stats_matrices(m, jobs, p)
            g[p] = single_feed_gains(N, I, skip)
        acc = acc * g
    out = []
    u = 0
    for img in imgs:
        h, w = img.shape[:2]
        if not blocks:
            out.append(acc[:, u].reshape(nplanes, 1).copy() if channels else acc[0, u].reshape(1, 1).copy())
            u += 1
            continue
        bpw, bph, _, _ = block_grid(w, h, block_size)
        k = bpw * bph
        gm = acc[:, u:u + k].astype(np.float32)
        u += k
        gm = gm.reshape(nplanes, bph, bpw).transpose(1, 2, 0)
        out.append(filter_gain_map(gm) if channels else filter_gain_map(gm[..., 0]))
    return (out, first, units) if want_stats else out
