"""Affine registration of this project in numpy: the contract `stitching_amd.MatchEstimator(model="affine")` and
`stitching_amd.CameraSolver(model="affine")` are tested against — byte for byte in every integer array, in the float64 bits of the
winning sample transform and in the bits of all 45 sums of every edge; the host parts within 1e-9.

This is the project's OWN algorithm, in the way of OpenCV's AffineBestOf2NearestMatcher, AffineBasedEstimator and
BundleAdjusterAffinePartial.  It is NOT them and answers to none of their names.  Nothing is taken from the package.  What is not said
here is tests/numpy_matches.py's and tests/numpy_cameras.py's, unchanged: the two nearest neighbours, the ratio test, the union and its
order, the generator of the sampler, the inlier test, "largest count, smallest k", the confidence, the mirrored entries, the subset, the
spanning tree and its centre, the edges and their points, the ordered sum, the assembly and the Levenberg-Marquardt loop.

  coordinates  level-0 pixels, NOT centred: x0 = (x + 0.5) * w0 / wl - 0.5 in float64, in this order; y alike.  The affine warper
               applies camera.R to raw pixels (ppx = ppy = 0), so every transform lives in that frame
  model        "affine_partial": a similarity, 4 degrees of freedom, samples of s = 2; "affine_full": 6 degrees, s = 3
  sampling     numpy_matches.sample restricted to t < s: the same generator, the same counter 4 k + t + 1, the same stepping past the
               earlier choices; pair p = i n + j, m >= 6
  hypothesis   division free and homogeneous, 9 doubles with h6 = h7 = +0.0; every product and sum rounded by itself, nothing fused,
               3-term sums (t0 + t1) + t2.
               partial, of (x0, y0) -> (u0, v0), (x1, y1) -> (u1, v1): dx = x1 - x0, dy, du, dv alike; W = dx dx + dy dy;
               A = du dx + dv dy; B = dv dx - du dy; C = u0 W - (A x0 - B y0); D = v0 W - (B x0 + A y0); H = [A, -B, C, B, A, D, 0, 0, W]
               full: M = the three source points as homogeneous columns, a = adj(M) (numpy_matches._adj); rows 0 and 1 of H are
               (N[r][0] a[0][c] + N[r][1] a[1][c]) + N[r][2] a[2][c], N the destination points' x row and y row;
               h8 = (x0 a[0][0] + x1 a[1][0]) + x2 a[2][0] = det M
               sign: h8 < 0 negates h0 .. h5 and h8 (every clockwise sample of the full model); h8 == 0 (coincident or collinear sample
               points) leaves the hypothesis without inliers
  refit        num_inliers >= 6, over the inliers on the host.  partial: least squares about the two centroids cp, cq:
               a = sum(dx du + dy dv) / sum(dx dx + dy dy), b = sum(dx dv - dy du) / the same, t = cq - [[a, -b], [b, a]] cp.  full:
               np.linalg.lstsq of the 6 unknowns on the centred points.  H is 3 x 3 with the last row exactly 0, 0, 1; not finite or
               without a finite inverse: no H (numpy_matches.inverse)
  estimate     T_centre = I; breadth first along the spanning tree T_to = T_from H_(to -> from), the entry (to, from)'s H or the inverse
               of (from, to)'s.  focal = 1, aspect = 1, ppx = ppy = 0, R = T as float32.  A graph that is not connected: "Homography
               estimation failed."
  adjustment   4 parameters per camera (a, b, tx, ty), T = [[a, -b, tx], [b, a, ty], [0, 0, 1]]; start: a = (T00 + T11) / 2,
               b = (T10 - T01) / 2, the translation kept.  9 variants of 8 doubles {a, b, tx, ty, a', b', tx', ty'}, the map and its
               inverse: the base, then + and - 1e-3 on each parameter; d = a a + b b, a' = a / d, b' = -b / d,
               tx' = -(a' tx - b' ty), ty' = -(b' tx + a' ty) (d == 0: not finite).  Residual of a match (x, y) | (u, v) of edge (i, j),
               in image j's frame: Px = (a_i x - b_i y) + tx_i, Py = (b_i x + a_i y) + ty_i, Qx = (a'_j Px - b'_j Py) + tx'_j,
               Qy = (b'_j Px + a'_j Py) + ty'_j, r = (u - Qx, v - Qy).  Jacobian column k of 8 = (r(+) - r(-)) 500, the other camera at
               its base.  45 terms: E += r0 r0 + r1 r1; g_k += J0k r0 + J1k r1; B_kl += J0k J0l + J1k J1l, k <= l; summed by
               numpy_cameras.ordered_sum.  Multiply, add, subtract only
  LM           numpy_cameras' loop; afterwards T_i <- T_centre^-1 T_i.  A parameter that is not finite, or a = b = 0: "Camera parameters
               adjusting failed."  No wave correction
"""
from collections import deque

import numpy as np

from tests import numpy_cameras as NC
from tests import numpy_matches as NM

MODELS = {"affine_partial": 2, "affine_full": 3}  # model -> sample size
STEP = NC.STEP
_field = NM._field


# ---- matching ------------------------------------------------------------------------------------------------------------------------------
def uncentred(f):
    """(n, 2) float64: the keypoints of one image in level-0 pixels"""
    level, x, y = (np.asarray(_field(f, k)) for k in ("level", "x", "y"))
    sizes = list(_field(f, "level_sizes"))
    if len(level) == 0:
        return np.zeros((0, 2), np.float64)
    w0, h0 = NC._size(f)
    out = np.zeros((len(level), 2), np.float64)
    for k, (l, xx, yy) in enumerate(zip(level.tolist(), x.tolist(), y.tolist())):
        wl, hl = sizes[l]
        out[k, 0] = (xx + 0.5) * w0 / wl - 0.5
        out[k, 1] = (yy + 0.5) * h0 / hl - 0.5
    return out


def sample(seed, p, k, m, s):
    """the s distinct match indices of hypothesis k of pair p with m matches, in the order drawn"""
    return NM.sample(seed, p, k, m)[:s]


def closed_form_partial(src, dst):
    """(9,) float64 of 2 correspondences (2 x 2 each), before the sign rule"""
    (x0, y0), (x1, y1) = [[np.float64(v) for v in p] for p in np.asarray(src, np.float64)]
    (u0, v0), (u1, v1) = [[np.float64(v) for v in p] for p in np.asarray(dst, np.float64)]
    zero = np.float64(0.0)
    with np.errstate(all="ignore"):
        dx, dy, du, dv = x1 - x0, y1 - y0, u1 - u0, v1 - v0
        W = dx * dx + dy * dy
        A = du * dx + dv * dy
        B = dv * dx - du * dy
        C = u0 * W - (A * x0 - B * y0)
        D = v0 * W - (B * x0 + A * y0)
        return np.array([A, -B, C, B, A, D, zero, zero, W], np.float64)


def closed_form_full(src, dst):
    """(9,) float64 of 3 correspondences (3 x 2 each), before the sign rule"""
    src = [[np.float64(v) for v in p] for p in np.asarray(src, np.float64)]
    dst = [[np.float64(v) for v in p] for p in np.asarray(dst, np.float64)]
    one = np.float64(1.0)
    with np.errstate(all="ignore"):
        a = NM._adj([[src[0][0], src[1][0], src[2][0]], [src[0][1], src[1][1], src[2][1]], [one, one, one]])
        N = [[dst[0][0], dst[1][0], dst[2][0]], [dst[0][1], dst[1][1], dst[2][1]]]
        h = [(N[r][0] * a[0][c] + N[r][1] * a[1][c]) + N[r][2] * a[2][c] for r in range(2) for c in range(3)]
        h8 = (src[0][0] * a[0][0] + src[1][0] * a[1][0]) + src[2][0] * a[2][0]
    return np.array(h + [0.0, 0.0, h8], np.float64)


def closed_form(src, dst, model):
    return closed_form_partial(src, dst) if model == "affine_partial" else closed_form_full(src, dst)


def hypothesis(xyuv, idx, model):
    """H (9,) with the sign rule applied, and whether it can have inliers at all (h8 != 0)"""
    h = closed_form(xyuv[idx, 0:2], xyuv[idx, 2:4], model)
    w = h[8]
    if w < 0:
        h[0:6] = -h[0:6]
        h[8] = -w
    return h, bool(w != 0)


def ransac(xyuv, p, iters, threshold, seed, model):
    """-> k, H_sample (9,), mask (m,) u8 of the best hypothesis of pair p"""
    m, s = len(xyuv), MODELS[model]
    t2 = np.float64(threshold) * np.float64(threshold)
    best = (-1, 0, None, None)
    for k in range(iters):
        h, ok = hypothesis(xyuv, sample(seed, p, k, m, s), model)
        mask = NM.inliers(h, xyuv, t2) if ok else np.zeros(m, bool)
        if int(mask.sum()) > best[0]:
            best = (int(mask.sum()), k, h, mask)
    return best[1], best[2], best[3].astype(np.uint8)


def refit_partial(src, dst):
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    cp, cq = src.mean(axis=0), dst.mean(axis=0)
    dx, dy = (src - cp).T
    du, dv = (dst - cq).T
    d = (dx * dx + dy * dy).sum()
    a, b = (dx * du + dy * dv).sum() / d, (dx * dv - dy * du).sum() / d
    L = np.array([[a, -b], [b, a]])
    t = cq - L @ cp
    return np.array([[a, -b, t[0]], [b, a, t[1]], [0.0, 0.0, 1.0]])


def refit_full(src, dst):
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    cp, cq = src.mean(axis=0), dst.mean(axis=0)
    A = np.concatenate([src - cp, np.ones((len(src), 1))], axis=1)
    sol = np.linalg.lstsq(A, dst - cq, rcond=None)[0]  # (3, 2): the linear part transposed, then the offset
    L = sol[0:2].T
    t = cq + sol[2] - L @ cp
    return np.array([[L[0, 0], L[0, 1], t[0]], [L[1, 0], L[1, 1], t[1]], [0.0, 0.0, 1.0]])


def refit(src, dst, model):
    return refit_partial(src, dst) if model == "affine_partial" else refit_full(src, dst)


def match(features, model="affine_partial", match_conf=0.3, range_width=-1, ransac_iters=500, ransac_threshold=3.0, seed=0x5EED):
    """numpy_matches.match with the affine model: the same n * n dicts"""
    n = len(features)
    T = NM.ratio_threshold(match_conf)
    desc = [np.asarray(_field(f, "descriptors"), np.uint8).reshape(-1, 32) for f in features]
    pts = [uncentred(f) for f in features]
    out = [NM.empty() for _ in range(n * n)]
    for i in range(n):
        for j in range(i + 1, n):
            if range_width >= 0 and j - i > range_width:
                continue
            e = NM.empty()
            e["src_img_idx"], e["dst_img_idx"] = i, j
            mt = e["matches"] = NM.union(desc[i], desc[j], T)
            m = len(mt)
            e["inliers_mask"] = np.zeros(m, np.uint8)
            if m >= NM.MIN_MATCHES:
                xyuv = np.concatenate([pts[i][mt[:, 0]], pts[j][mt[:, 1]]], axis=1)
                e["hypothesis"], e["H_sample"], mask = ransac(xyuv, i * n + j, ransac_iters, ransac_threshold, seed, model)
                if int(mask.sum()) >= NM.MIN_MATCHES:
                    keep = mask != 0
                    with np.errstate(all="ignore"):
                        h = refit(xyuv[keep, 0:2], xyuv[keep, 2:4], model)
                    if NM.inverse(h) is not None:
                        e["inliers_mask"], e["num_inliers"], e["H"] = mask, int(mask.sum()), h
                        e["confidence"] = NM.confidence(e["num_inliers"], m)
            out[i * n + j] = e
            out[j * n + i] = NM.mirrored(e, i, j)
    return out


# ---- camera estimate -----------------------------------------------------------------------------------------------------------------------
def transforms(matches, n):
    """float64 (3, 3) per camera: image pixels -> the centre image's pixels, along the spanning tree"""
    adj, centre = NC.spanning_tree(matches, n)
    if adj is None:
        raise NC.ContractError("Homography estimation failed.")
    T = [None] * n
    T[centre] = np.eye(3)
    q = deque([centre])
    while q:
        a = q.popleft()
        for b in adj[a]:
            if T[b] is None:
                T[b] = T[a] @ NC._pair_H(matches, n, b, a)
                q.append(b)
    return T


def estimate(features, matches):
    """[R float32]"""
    return [T.astype(np.float32) for T in transforms(matches, len(features))]


# ---- adjustment ----------------------------------------------------------------------------------------------------------------------------
def start_parameters(Rs):
    """(n, 4) float64 rows a, b, tx, ty: the similarity nearest to each estimate's linear part, its translation kept"""
    out = np.zeros((len(Rs), 4), np.float64)
    for k, R in enumerate(Rs):
        T = np.asarray(R, np.float64)
        out[k] = [(T[0, 0] + T[1, 1]) / 2, (T[1, 0] - T[0, 1]) / 2, T[0, 2], T[1, 2]]
    return out


def similarity(p):
    a, b, tx, ty = (float(v) for v in p)
    return np.array([[a, -b, tx], [b, a, ty], [0.0, 0.0, 1.0]])


def variants(params):
    """(n, 9, 8) float64 of params (n, 4) rows a, b, tx, ty: the base, then + and - STEP on each parameter; each the map and its inverse"""
    params = np.asarray(params, np.float64).reshape(-1, 4)
    out = np.zeros((len(params), 9, 8), np.float64)
    with np.errstate(all="ignore"):
        for c, p in enumerate(params):
            rows = [p + np.zeros(4)]
            for k in range(4):
                for sign in (1.0, -1.0):
                    shift = np.zeros(4)
                    shift[k] = sign * STEP
                    rows.append(p + shift)
            for v, (a, b, tx, ty) in enumerate(rows):
                d = a * a + b * b
                ai, bi = a / d, -b / d
                out[c, v] = [a, b, tx, ty, ai, bi, -(ai * tx - bi * ty), -(bi * tx + ai * ty)]
    return out


def _forward(V, x, y):
    return (V[0] * x - V[1] * y) + V[2], (V[1] * x + V[0] * y) + V[3]


def _residual(Vj, P, u, v):
    qx, qy = _forward(Vj[4:8], P[0], P[1])
    return [u - qx, v - qy]


def match_terms(Vi, Vj, xyuv):
    """(m, 45) float64: the terms E, g[8], B[36] of every match of an edge whose cameras have the variants Vi, Vj (9, 8)"""
    x, y, u, v = (np.ascontiguousarray(xyuv[:, k]) for k in range(4))
    with np.errstate(all="ignore"):
        P = _forward(Vi[0], x, y)
        r = _residual(Vj[0], P, u, v)
        J = []
        for k in range(4):
            p = _residual(Vj[0], _forward(Vi[1 + 2 * k], x, y), u, v)
            m = _residual(Vj[0], _forward(Vi[2 + 2 * k], x, y), u, v)
            J.append([(p[c] - m[c]) * 500.0 for c in range(2)])
        for k in range(4):
            p = _residual(Vj[1 + 2 * k], P, u, v)
            m = _residual(Vj[2 + 2 * k], P, u, v)
            J.append([(p[c] - m[c]) * 500.0 for c in range(2)])
        out = np.zeros((len(x), 45), np.float64)
        out[:, 0] = r[0] * r[0] + r[1] * r[1]
        for k in range(8):
            out[:, 1 + k] = J[k][0] * r[0] + J[k][1] * r[1]
        for t, (k, l) in enumerate(NC.TRIU):
            out[:, 9 + t] = J[k][0] * J[l][0] + J[k][1] * J[l][1]
    return out


def normal_equations(features, matches, params, conf_thresh=1.0, pts=None):
    """E (e,), g (e, 8), B (e, 36) of the edges in ascending order"""
    n = len(features)
    V = variants(params)
    if pts is None:
        pts = [uncentred(f) for f in features]
    ed = NC.edges(matches, n, conf_thresh)
    out = np.zeros((len(ed), 45), np.float64)
    for k, (i, j) in enumerate(ed):
        out[k] = NC.ordered_sum(match_terms(V[i], V[j], NC.edge_points(features, matches, n, i, j, pts)))
    return out[:, 0].copy(), out[:, 1:9].copy(), out[:, 9:].copy()


def adjust(features, matches, Rs, conf_thresh=1.0, max_evals=100, evaluate=None):
    """Rs [(3, 3)] -> [R float32], info.  evaluate(params) -> E, g, B replaces the evaluation (the tests count with it)"""
    n = len(features)
    pts = [uncentred(f) for f in features]
    ed = NC.edges(matches, n, conf_thresh)
    if evaluate is None:
        def evaluate(p):
            return normal_equations(features, matches, p, conf_thresh, pts)
    p = start_parameters(Rs)
    with np.errstate(all="ignore"):
        E, g, A = NC.assemble(n, ed, *evaluate(p))
        info = {"edges": len(ed), "matches": int(sum(len(NC.edge_points(features, matches, n, i, j, pts)) for i, j in ed)),
                "evaluations": 1, "accepted": 0, "first_E": float(E), "last_E": float(E)}
        lam = 1e-3
        while info["evaluations"] < max_evals:
            try:
                d = np.linalg.solve(A + lam * np.diag(np.diag(A)), -g)
            except np.linalg.LinAlgError:
                d = None
            better = False
            if d is not None and np.isfinite(variants(p + d.reshape(n, 4))).all():  # else a rejected step, not evaluated
                q = p + d.reshape(n, 4)
                E2, g2, A2 = NC.assemble(n, ed, *evaluate(q))
                info["evaluations"] += 1
                better = bool(E2 < E)
            if better:
                gain = (E - E2) / E
                p, E, g, A = q, E2, g2, A2
                lam = max(lam / 10.0, 1e-12)
                info["accepted"] += 1
                if gain < 1e-10:
                    break
            else:
                lam *= 10.0
                if lam > 1e12:
                    break
    info["last_E"], info["parameters"] = float(E), p.copy()
    if not np.isfinite(p).all() or ((p[:, 0] == 0) & (p[:, 1] == 0)).any():
        raise NC.ContractError("Camera parameters adjusting failed.")
    _, centre = NC.spanning_tree(matches, n)
    if centre < 0:
        raise NC.ContractError("Camera parameters adjusting failed.")
    T = [similarity(q) for q in p]
    inv = np.linalg.inv(T[centre])
    return [(inv @ Ti).astype(np.float32) for Ti in T], info


def register(features, matches, conf_thresh=1.0, max_evals=100):
    """-> indices, [{"focal", "R", "ppx", "ppy", "aspect"}], info of the adjustment"""
    n = len(features)
    indices = NC.subset(matches, n, conf_thresh)
    features = [features[i] for i in indices]
    matches = NC.subset_matches(matches, indices)
    Rs, info = adjust(features, matches, estimate(features, matches), conf_thresh, max_evals)
    return indices, [{"focal": 1.0, "R": R, "ppx": 0.0, "ppy": 0.0, "aspect": 1.0} for R in Rs], info
