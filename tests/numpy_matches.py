"""The descriptor matcher and homography RANSAC of this project in numpy: the contract `stitching_amd.MatchEstimator` is tested against
— byte for byte in every integer array and in the float64 bits of the winning sample homography.

This is the project's OWN matcher.  It is NOT cv.detail.BestOf2NearestMatcher and does not claim the names "homography" / "affine".
Nothing is taken from the package.  For the features of n images (256-bit descriptors, keypoints x, y of a pyramid level) and
match_conf, range_width, ransac_iters, ransac_threshold, seed:

  two nearest  for an ordered pair (a, b) and a descriptor q of a: d1 <= d2 the two smallest Hamming distances to b's descriptors (with
               multiplicity: duplicates in b give d1 == d2), i1 the index of d1, the smaller index among equals.  q is matched iff b
               has at least 2 descriptors and 1024 d1 < T d2, T = floor((1 - match_conf) 1024 + 0.5) in float64, an integer
  union        for i < j: the forward matches (q, i1, d1) by ascending q, then by ascending t every backward match (i1(t), t, d1) of
               j -> i whose (query, train) is not a forward match.  With range_width >= 0 only pairs with j - i <= range_width
  coordinates  x0 = (x + 0.5) * w0 / wl - 0.5 - w0 * 0.5 in float64, in this order; y alike
  sampling     pair p = i n + j with m >= 6 matches, hypothesis k, t = 0 .. 3 (all in uint32):
               r_t = mix32(seed ^ mix32(p 0x9E3779B9 + mix32(4 k + t + 1))) mod (m - t), then stepped past the earlier choices in
               ascending order (if r >= c: r += 1).  mix32: x ^= x >> 16, x *= 0x7FEB352D, x ^= x >> 15, x *= 0x846CA68B, x ^= x >> 16
  homography   of the 4 sampled correspondences, division free: M = [p0 p1 p2] (homogeneous columns), lambda = adj(M) p3,
               A = M diag(lambda); B alike of the destination points; H = B adj(A).  Every 2 x 2 minor is a*b - c*d (two rounded
               products, one rounded difference), every 3-term sum (t0 + t1) + t2; no fused multiply-add anywhere.  With
               W0 = (h6 x + h7 y) + h8 at sample point 0: W0 < 0 negates H, W0 == 0 leaves the hypothesis without inliers
  inliers      X = (h0 x + h1 y) + h2, Y, W alike; ex = X - u W, ey = Y - v W; inlier iff W > 0 and ex ex + ey ey <= (t t) (W W)
  best         the largest count, the smallest k among equals
  refit        num_inliers >= 6: Hartley-normalised DLT over the inliers (SVD), scaled to h22 = 1; confidence =
               num_inliers / (8 + 0.3 m), 0 when above 3.  Below 6 matches or 6 inliers, or with a refit that is not finite or has no
               finite inverse (many matches onto a few points): confidence 0, H None, no inliers
  mirror       entry (j, i): query / train swapped, H inverted; diagonal and skipped entries are empty with both indices -1
"""
import math

import numpy as np

POP = np.array([bin(v).count("1") for v in range(256)], np.int32)
M32 = 0xFFFFFFFF
MIN_MATCHES = 6
NO_D2 = 0xFFFF  # the second distance where the other image has a single descriptor (never used: such a query is unmatched)


def _field(f, name):
    return f[name] if isinstance(f, dict) else getattr(f, name)


def ratio_threshold(match_conf):
    return int(math.floor((1.0 - float(match_conf)) * 1024.0 + 0.5))


def ratio_test(d1, d2, T):
    return 1024 * int(d1) < int(T) * int(d2)


def centred(f):
    """(n, 2) float64: the keypoints of one image in level-0 pixels relative to the image centre"""
    level, x, y = (np.asarray(_field(f, k)) for k in ("level", "x", "y"))
    sizes = list(_field(f, "level_sizes"))
    if len(level) == 0:
        return np.zeros((0, 2), np.float64)
    w0, h0 = (f.get("img_size") if isinstance(f, dict) else getattr(f, "img_size", None)) or sizes[0]
    out = np.zeros((len(level), 2), np.float64)
    for k, (l, xx, yy) in enumerate(zip(level.tolist(), x.tolist(), y.tolist())):
        wl, hl = sizes[l]
        out[k, 0] = (xx + 0.5) * w0 / wl - 0.5 - w0 * 0.5
        out[k, 1] = (yy + 0.5) * h0 / hl - 0.5 - h0 * 0.5
    return out


def two_nn(A, B):
    """i1, d1, d2 (int32 each) of every descriptor of A among the descriptors of B (at least one)"""
    A, B = np.asarray(A, np.uint8).reshape(-1, 32), np.asarray(B, np.uint8).reshape(-1, 32)
    d = np.zeros((len(A), len(B)), np.int32)
    for k in range(32):
        d += POP[A[:, k, None] ^ B[None, :, k]]
    i1 = np.argmin(d, axis=1).astype(np.int32)  # the first minimum: the smaller index
    rows = np.arange(len(A))
    d1 = d[rows, i1]
    if len(B) < 2:
        return i1, d1, np.full(len(A), NO_D2, np.int32)
    d[rows, i1] = 1 << 20
    return i1, d1, d.min(axis=1)


def one_way(A, B, T):
    """matched (bool), i1, d1 of A's descriptors in B"""
    na = len(A)
    if len(B) < 2 or na == 0:
        return np.zeros(na, bool), np.zeros(na, np.int32), np.zeros(na, np.int32)
    i1, d1, d2 = two_nn(A, B)
    return 1024 * d1.astype(np.int64) < T * d2.astype(np.int64), i1, d1


def union(A, B, T):
    """(m, 3) int32 rows query, train, distance of the pair (A, B)"""
    fm, fi, fd = one_way(A, B, T)
    bm, bi, bd = one_way(B, A, T)
    rows = [(q, int(fi[q]), int(fd[q])) for q in range(len(A)) if fm[q]]
    for t in range(len(B)):
        if bm[t]:
            q = int(bi[t])
            if not (fm[q] and fi[q] == t):
                rows.append((q, t, int(bd[t])))
    return np.array(rows, np.int32).reshape(-1, 3)


def mix32(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def sample(seed, p, k, m):
    """the 4 distinct match indices of hypothesis k of pair p with m matches, in the order drawn"""
    chosen = []
    for t in range(4):
        r = mix32((seed & M32) ^ mix32(((p * 0x9E3779B9) & M32) + mix32(4 * k + t + 1))) % (m - t)
        for c in sorted(chosen):
            if r >= c:
                r += 1
        chosen.append(r)
    return chosen


def _adj(m):
    """adjugate of a 3 x 3 list of lists of float64 scalars: every entry one a*b - c*d"""
    return [[m[1][1] * m[2][2] - m[1][2] * m[2][1], m[0][2] * m[2][1] - m[0][1] * m[2][2], m[0][1] * m[1][2] - m[0][2] * m[1][1]],
            [m[1][2] * m[2][0] - m[1][0] * m[2][2], m[0][0] * m[2][2] - m[0][2] * m[2][0], m[0][2] * m[1][0] - m[0][0] * m[1][2]],
            [m[1][0] * m[2][1] - m[1][1] * m[2][0], m[0][1] * m[2][0] - m[0][0] * m[2][1], m[0][0] * m[1][1] - m[0][1] * m[1][0]]]


def _basis(pts):
    """M diag(adj(M) p3) of 4 points: the matrix that takes the projective basis to them"""
    one = np.float64(1.0)
    m = [[pts[0][0], pts[1][0], pts[2][0]], [pts[0][1], pts[1][1], pts[2][1]], [one, one, one]]
    a = _adj(m)
    lam = [(a[r][0] * pts[3][0] + a[r][1] * pts[3][1]) + a[r][2] * one for r in range(3)]
    return [[m[r][c] * lam[c] for c in range(3)] for r in range(3)]


def closed_form(src, dst):
    """(9,) float64: H = B adj(A) of 4 correspondences (4 x 2 each), before the sign rule"""
    src = [[np.float64(v) for v in p] for p in np.asarray(src, np.float64)]
    dst = [[np.float64(v) for v in p] for p in np.asarray(dst, np.float64)]
    with np.errstate(all="ignore"):
        a = _adj(_basis(src))
        b = _basis(dst)
        return np.array([(b[r][0] * a[0][c] + b[r][1] * a[1][c]) + b[r][2] * a[2][c] for r in range(3) for c in range(3)], np.float64)


def hypothesis(xyuv, idx):
    """H (9,) with the sign rule applied, and whether it can have inliers at all (W0 != 0)"""
    h = closed_form(xyuv[idx, 0:2], xyuv[idx, 2:4])
    x, y = xyuv[idx[0], 0], xyuv[idx[0], 1]
    with np.errstate(all="ignore"):
        w0 = (h[6] * x + h[7] * y) + h[8]
    if w0 < 0:
        h = -h
    return h, bool(w0 != 0)


def inliers(h, xyuv, t2):
    x, y, u, v = xyuv[:, 0], xyuv[:, 1], xyuv[:, 2], xyuv[:, 3]
    with np.errstate(all="ignore"):
        X = (h[0] * x + h[1] * y) + h[2]
        Y = (h[3] * x + h[4] * y) + h[5]
        W = (h[6] * x + h[7] * y) + h[8]
        ex, ey = X - u * W, Y - v * W
        return (W > 0) & (ex * ex + ey * ey <= t2 * (W * W))


def ransac(xyuv, p, iters, threshold, seed):
    """-> k, H_sample (9,), mask (m,) u8 of the best hypothesis of pair p"""
    m = len(xyuv)
    t2 = np.float64(threshold) * np.float64(threshold)
    best = (-1, 0, None, None)
    for k in range(iters):
        h, ok = hypothesis(xyuv, sample(seed, p, k, m))
        mask = inliers(h, xyuv, t2) if ok else np.zeros(m, bool)
        if int(mask.sum()) > best[0]:
            best = (int(mask.sum()), k, h, mask)
    return best[1], best[2], best[3].astype(np.uint8)


def _normalise(p):
    c = p.mean(axis=0)
    d = np.sqrt(((p - c) ** 2).sum(axis=1)).mean()
    s = math.sqrt(2.0) / d if d > 0 else 1.0
    return np.array([[s, 0.0, -s * c[0]], [0.0, s, -s * c[1]], [0.0, 0.0, 1.0]]), (p - c) * s


def refit(src, dst):
    """(3, 3) float64 with h22 = 1: the Hartley-normalised DLT of k >= 4 correspondences"""
    ts, s = _normalise(np.asarray(src, np.float64))
    td, d = _normalise(np.asarray(dst, np.float64))
    k = len(s)
    a = np.zeros((2 * k, 9), np.float64)
    a[0::2, 0:2], a[0::2, 2] = -s, -1.0
    a[0::2, 6:8], a[0::2, 8] = d[:, 0:1] * s, d[:, 0]
    a[1::2, 3:5], a[1::2, 5] = -s, -1.0
    a[1::2, 6:8], a[1::2, 8] = d[:, 1:2] * s, d[:, 1]
    h = np.linalg.svd(a)[2][-1].reshape(3, 3)
    h = np.linalg.inv(td) @ h @ ts
    return h / h[2, 2]


def inverse(h):
    """the inverse the mirrored entry carries, or None where h is not finite or has no finite inverse: the pair then has no homography"""
    if not np.isfinite(h).all():
        return None
    try:
        inv = np.linalg.inv(h)
    except np.linalg.LinAlgError:
        return None
    return inv if np.isfinite(inv).all() else None


def confidence(num_inliers, m):
    c = num_inliers / (8 + 0.3 * m)
    return 0.0 if c > 3 else c


def empty():
    return {"src_img_idx": -1, "dst_img_idx": -1, "matches": np.zeros((0, 3), np.int32), "inliers_mask": np.zeros(0, np.uint8),
            "num_inliers": 0, "H": None, "confidence": 0.0, "H_sample": None, "hypothesis": -1}


def mirrored(e, i, j):
    """entry (j, i) of entry (i, j), whose H has passed inverse()"""
    return {"src_img_idx": j, "dst_img_idx": i, "matches": np.ascontiguousarray(e["matches"][:, [1, 0, 2]]),
            "inliers_mask": e["inliers_mask"].copy(), "num_inliers": e["num_inliers"],
            "H": None if e["H"] is None else np.linalg.inv(e["H"]), "confidence": e["confidence"], "H_sample": None, "hypothesis": -1}


def match(features, match_conf=0.3, range_width=-1, ransac_iters=500, ransac_threshold=3.0, seed=0x5EED):
    """n * n dicts, row-major: src_img_idx, dst_img_idx, matches (m, 3) int32, inliers_mask (m,) u8, num_inliers, H, confidence,
    H_sample (9,) float64 and hypothesis of the pairs i < j that RANSAC ran on (None and -1 elsewhere)"""
    n = len(features)
    T = ratio_threshold(match_conf)
    desc = [np.asarray(_field(f, "descriptors"), np.uint8).reshape(-1, 32) for f in features]
    pts = [centred(f) for f in features]
    out = [empty() for _ in range(n * n)]
    for i in range(n):
        for j in range(i + 1, n):
            if range_width >= 0 and j - i > range_width:
                continue
            e = empty()
            e["src_img_idx"], e["dst_img_idx"] = i, j
            mt = e["matches"] = union(desc[i], desc[j], T)
            m = len(mt)
            e["inliers_mask"] = np.zeros(m, np.uint8)
            if m >= MIN_MATCHES:
                xyuv = np.concatenate([pts[i][mt[:, 0]], pts[j][mt[:, 1]]], axis=1)
                e["hypothesis"], e["H_sample"], mask = ransac(xyuv, i * n + j, ransac_iters, ransac_threshold, seed)
                if int(mask.sum()) >= MIN_MATCHES:
                    keep = mask != 0
                    with np.errstate(all="ignore"):
                        h = refit(xyuv[keep, 0:2], xyuv[keep, 2:4])
                    if inverse(h) is not None:
                        e["inliers_mask"], e["num_inliers"], e["H"] = mask, int(mask.sum()), h
                        e["confidence"] = confidence(e["num_inliers"], m)
            out[i * n + j] = e
            out[j * n + i] = mirrored(e, i, j)
    return out
