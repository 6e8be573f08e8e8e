"""Camera registration of this project in numpy: the contract `stitching_amd.CameraSolver` is tested against — subset, focals, rotations,
ray bundle adjustment and wave correction.  The device part (the normal equations of every edge) equals it in the bits of all 45 float64
sums of every edge; the host part equals it within 1e-9.

This is the project's OWN solver, in the way of OpenCV's homography-based estimator, ray adjuster and wave correction, restated from
recollection.  It is NOT cv.detail.HomographyBasedEstimator, BundleAdjusterRay or waveCorrect and answers to none of their names.
Nothing is taken from the package.  Inputs: the features of n images, the n x n match entries of tests/numpy_matches.match (dicts or
objects with the same fields), conf_thresh = 1.0, wave_correct = "horiz", max_evals = 100.  Points are numpy_matches.centred: level-0
pixels relative to the image centre, so the principal point is (0, 0) throughout; the cameras returned carry ppx = w0 / 2, ppy = h0 / 2,
aspect = 1 and a float32 R.

  subset     union-find over the pairs i < j with confidence >= conf_thresh; the largest component, among equals the one with the
             smallest index; ascending.  Fewer than 2: an error; fewer than n: a warning
  focals     for every i < j with an H the two candidates of the closed form over h0 .. h8 (the v1 < v2 swap, the |d1| > |d2| choice);
             where both exist sqrt(f0 f1) is collected.  With n - 1 values or more every camera starts from their median (the mean of
             the two middle values of an even count), else from the mean of w0 + h0 over the images
  rotations  maximum spanning tree over the edges with an H (Kruskal, num_inliers descending, then (i, j) ascending); the centre is the
             node of least eccentricity, the smallest index among equals; breadth first from it, neighbours ascending: R_centre = I,
             R_to = R_from (K_from^-1 H_from->to^-1 K_to), H_from->to the entry (from, to)'s or the inverse of the entry (to, from)'s
  rays       4 parameters per camera: focal and the Rodrigues vector of the SVD-orthonormalised R (negated where det < 0).  Edges: the
             pairs i < j with confidence > conf_thresh, ascending; their points: the inlier matches in match order.  9 variants per camera,
             (f', H' = Rodrigues(r') diag(1 / f', 1 / f', 1)): the base, then + and - 1e-3 on each parameter.  Per match (x, y) of
             camera i and (u, v) of camera j, per variant: X = (h0 x + h1 y) + h2 (rows alike), s = sqrt((X0 X0 + X1 X1) + X2 X2),
             ray = X / s; residual r = sqrt(f_i' f_j') (ray_i - ray_j); Jacobian column k of 8 = (r(+) - r(-)) 500, the other camera at
             its base.  45 terms: E += (r0 r0 + r1 r1) + r2 r2; g_k += (J0k r0 + J1k r1) + J2k r2; B_kl += (J0k J0l + J1k J1l) + J2k J2l,
             k <= l.  IEEE float64 multiply, add, subtract, divide, sqrt in this order; nothing fused
  the sum    lane l of 256 adds the terms of the matches l, l + 256, .. in that order from +0.0 (a missing match adds +0.0); the 256
             lane sums are folded by v[l] += v[l + s], s = 128, 64, .. 1
  LM         the 4n x 4n system from the edges in ascending order, each 8 x 8 block mirrored; lam = 1e-3; (A + lam diag(A)) d = -g;
             E' < E: accept, lam = max(lam / 10, 1e-12), stop when (E - E') / E < 1e-10; else lam *= 10, stop above 1e12; a LinAlgError
             or a step to variants that are not finite is a rejected step without an evaluation; at most max_evals evaluations.  Then R_i <- R_centre^-1 R_i
  wave       M = sum x_i x_i^T (x_i the first column of R_i); rg1 = the eigh vector of the smallest ("horiz") or largest ("vert")
             eigenvalue; k = the sum of the third columns; rg0 = normalise(rg1 x k), rg2 = rg0 x rg1; sum rg0 . x_i < 0 negates rg0 and
             rg1; R_i <- [rg0; rg1; rg2] R_i
"""
import math
import warnings
from collections import deque

import numpy as np

from tests import numpy_matches as NM

LANES = 256
STEP = 1e-3
NO_MATCH = ("No match exceeds the given confidence threshold. Do your images have enough overlap and common features? If yes, you might "
            "want to lower the 'confidence_threshold' or try another 'detector'.")
NOT_ALL = ("Not all images are included in the final panorama. If this is not intended, use the 'matches_graph_dot_file' parameter to "
           "analyze your matches. You might want to lower the 'confidence_threshold' or try another 'detector' to include all your images.")
TRIU = [(k, l) for k in range(8) for l in range(k, 8)]


class ContractError(Exception):
    pass


class ContractWarning(UserWarning):
    pass


_field = NM._field


def _find(parent, a):
    while parent[a] != a:
        parent[a] = parent[parent[a]]
        a = parent[a]
    return a


# ---- subset ------------------------------------------------------------------------------------------------------------------------------
def subset(matches, n, conf_thresh=1.0):
    parent = list(range(n))
    for i in range(n):
        for j in range(i + 1, n):
            if _field(matches[i * n + j], "confidence") >= conf_thresh:
                a, b = _find(parent, i), _find(parent, j)
                if a != b:
                    parent[max(a, b)] = min(a, b)
    groups = {}
    for i in range(n):
        groups.setdefault(_find(parent, i), []).append(i)
    best = min(groups.values(), key=lambda g: (-len(g), g[0])) if groups else []
    if len(best) < 2:
        raise ContractError(NO_MATCH)
    if len(best) < n:
        warnings.warn(NOT_ALL, ContractWarning)
    return best


def subset_matches(matches, indices):
    n = int(math.sqrt(len(matches)))
    return [matches[i * n + j] for i in indices for j in indices]


# ---- focals ------------------------------------------------------------------------------------------------------------------------------
def focals_from_homography(H):
    """(f0, f1), each None where the closed form gives none"""
    h = np.asarray(H, np.float64).reshape(9)
    with np.errstate(all="ignore"):
        d1 = h[6] * h[7]
        d2 = (h[7] - h[6]) * (h[7] + h[6])
        v1 = -(h[0] * h[1] + h[3] * h[4]) / d1
        v2 = (h[0] * h[0] + h[3] * h[3] - h[1] * h[1] - h[4] * h[4]) / d2
        f1 = _pick(v1, v2, d1, d2)
        d1 = h[0] * h[3] + h[1] * h[4]
        d2 = h[0] * h[0] + h[1] * h[1] - h[3] * h[3] - h[4] * h[4]
        v1 = -h[2] * h[5] / d1
        v2 = (h[5] * h[5] - h[2] * h[2]) / d2
        f0 = _pick(v1, v2, d1, d2)
    return f0, f1


def _pick(v1, v2, d1, d2):
    if v1 < v2:
        v1, v2, d1, d2 = v2, v1, d2, d1
    if v1 > 0 and v2 > 0:
        v = v1 if abs(d1) > abs(d2) else v2
    elif v1 > 0:
        v = v1
    else:
        return None
    return float(np.sqrt(v)) if np.isfinite(v) else None


def _median(values):
    v = sorted(values)
    k = len(v)
    return v[k // 2] if k % 2 else (v[k // 2 - 1] + v[k // 2]) * 0.5


def initial_focal(features, matches, n):
    found = []
    for i in range(n):
        for j in range(i + 1, n):
            H = _field(matches[i * n + j], "H")
            if H is not None:
                f0, f1 = focals_from_homography(H)
                if f0 is not None and f1 is not None:
                    found.append(math.sqrt(f0 * f1))
    if len(found) >= n - 1:
        return _median(found)
    return sum(_size(f)[0] + _size(f)[1] for f in features) / n


def _size(f):
    s = f.get("img_size") if isinstance(f, dict) else getattr(f, "img_size", None)
    return s or list(_field(f, "level_sizes"))[0]


# ---- rotations ---------------------------------------------------------------------------------------------------------------------------
def _pair_H(matches, n, a, b):
    """H that takes points of image a to image b, or None"""
    H = _field(matches[a * n + b], "H")
    if H is not None:
        return np.asarray(H, np.float64)
    H = _field(matches[b * n + a], "H")
    return None if H is None else np.linalg.inv(np.asarray(H, np.float64))


def spanning_tree(matches, n):
    """adjacency lists (ascending) of the maximum spanning tree, and the centre; None where the graph is not connected"""
    cand = []
    for i in range(n):
        for j in range(i + 1, n):
            e = matches[i * n + j] if _field(matches[i * n + j], "H") is not None else matches[j * n + i]
            if _field(e, "H") is not None:
                cand.append((-int(_field(e, "num_inliers")), i, j))
    parent, adj, used = list(range(n)), [[] for _ in range(n)], 0
    for _, i, j in sorted(cand):
        a, b = _find(parent, i), _find(parent, j)
        if a != b:
            parent[a] = b
            adj[i].append(j)
            adj[j].append(i)
            used += 1
    if used != n - 1:
        return None, -1
    adj = [sorted(a) for a in adj]
    ecc = [max(_depths(adj, s)) for s in range(n)]
    return adj, ecc.index(min(ecc))


def _depths(adj, start):
    d = [-1] * len(adj)
    d[start] = 0
    q = deque([start])
    while q:
        a = q.popleft()
        for b in adj[a]:
            if d[b] < 0:
                d[b] = d[a] + 1
                q.append(b)
    return d


def rotations(matches, n, focals):
    """float64 (3, 3) per camera"""
    adj, centre = spanning_tree(matches, n)
    if adj is None:
        raise ContractError("Homography estimation failed.")
    R = [None] * n
    R[centre] = np.eye(3)
    q = deque([centre])
    while q:
        a = q.popleft()
        for b in adj[a]:
            if R[b] is None:
                Ka_inv = np.diag([1.0 / focals[a], 1.0 / focals[a], 1.0])
                Kb = np.diag([focals[b], focals[b], 1.0])
                R[b] = R[a] @ (Ka_inv @ np.linalg.inv(_pair_H(matches, n, a, b)) @ Kb)
                q.append(b)
    return R


def estimate(features, matches):
    """[(focal, R float32)]"""
    n = len(features)
    f = initial_focal(features, matches, n)
    return [(f, R.astype(np.float32)) for R in rotations(matches, n, [f] * n)]


# ---- Rodrigues ---------------------------------------------------------------------------------------------------------------------------
def rodrigues(r):
    """vector -> matrix, in float64 scalars: th = sqrt((x x + y y) + z z); k = r / th; c, s = cos th, sin th; c1 = 1 - c;
    R_ab = (c1 k_a) k_b + (c on the diagonal, -+ s k elsewhere); th < 1e-12: I"""
    x, y, z = (np.float64(v) for v in r)
    th = np.sqrt((x * x + y * y) + z * z)
    if not th >= 1e-12:
        return np.eye(3) if th == th else np.full((3, 3), np.nan)
    c, s = np.cos(th), np.sin(th)
    c1 = 1.0 - c
    kx, ky, kz = x / th, y / th, z / th
    return np.array([[(c1 * kx) * kx + c, (c1 * kx) * ky - s * kz, (c1 * kx) * kz + s * ky],
                     [(c1 * ky) * kx + s * kz, (c1 * ky) * ky + c, (c1 * ky) * kz - s * kx],
                     [(c1 * kz) * kx - s * ky, (c1 * kz) * ky + s * kx, (c1 * kz) * kz + c]], np.float64)


def rodrigues_vector(R):
    """matrix -> vector of the SVD-orthonormalised R (negated where det < 0)"""
    u, _, vt = np.linalg.svd(np.asarray(R, np.float64))
    R = u @ vt
    if np.linalg.det(R) < 0:
        R = -R
    axis = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = np.sqrt((axis * axis).sum()) * 0.5
    c = min(max((R[0, 0] + R[1, 1] + R[2, 2] - 1.0) * 0.5, -1.0), 1.0)
    th = math.atan2(s, c)  # exact for small turns, where acos is not
    if s < 1e-12 and c > 0:
        return np.zeros(3)
    if s < 1e-6 and c < 0:
        # next to a half turn R = 2 k k^T - I and the skew part vanishes: |k| from the diagonal, the signs relative to the largest
        # component from its row, the sign of all of it from what is left of the skew part
        d = np.sqrt(np.maximum((np.diag(R) + 1.0) * 0.5, 0.0))
        i = int(np.argmax(d))
        for j in range(3):
            if j != i and R[i, j] + R[j, i] < 0:
                d[j] = -d[j]
        if d @ axis < 0:
            d = -d
        return d * (th / np.sqrt((d * d).sum()))
    return axis * (th / (2.0 * s))


# ---- rays --------------------------------------------------------------------------------------------------------------------------------
def variants(params):
    """(n, 9, 10) float64 of params (n, 4) rows f, rx, ry, rz: the base, then + and - STEP on each parameter; each f', H' row-major"""
    params = np.asarray(params, np.float64).reshape(-1, 4)
    out = np.zeros((len(params), 9, 10), np.float64)
    with np.errstate(all="ignore"):
        for c, p in enumerate(params):
            rows = [p + np.zeros(4)]
            for k in range(4):
                for sign in (1.0, -1.0):
                    shift = np.zeros(4)
                    shift[k] = sign * STEP
                    rows.append(p + shift)
            for v, q in enumerate(rows):
                R = rodrigues(q[1:4])
                inv = 1.0 / q[0]
                out[c, v, 0] = q[0]
                out[c, v, 1:] = (R * np.array([inv, inv, 1.0])).reshape(9)
    return out


def edges(matches, n, conf_thresh=1.0):
    return [(i, j) for i in range(n) for j in range(i + 1, n) if _field(matches[i * n + j], "confidence") > conf_thresh]


def edge_points(features, matches, n, i, j, pts=None):
    """(m, 4) float64 x, y, u, v: the inlier matches of the pair in match order"""
    e = matches[i * n + j]
    mt = np.asarray(_field(e, "matches")).reshape(-1, 3)
    keep = np.asarray(_field(e, "inliers_mask")) != 0
    a = NM.centred(features[i]) if pts is None else pts[i]
    b = NM.centred(features[j]) if pts is None else pts[j]
    return np.concatenate([a[mt[keep, 0]].reshape(-1, 2), b[mt[keep, 1]].reshape(-1, 2)], axis=1)


def _rays(V, x, y):
    """(3, m) unit rays of variant V (10,) at the points x, y"""
    X = [(V[1 + 3 * r] * x + V[2 + 3 * r] * y) + V[3 + 3 * r] for r in range(3)]
    s = np.sqrt((X[0] * X[0] + X[1] * X[1]) + X[2] * X[2])
    return [X[0] / s, X[1] / s, X[2] / s]


def _residual(Vi, Vj, ri, rj):
    s = np.sqrt(Vi[0] * Vj[0])
    return [s * (ri[k] - rj[k]) for k in range(3)]


def match_terms(Vi, Vj, xyuv):
    """(m, 45) float64: the terms E, g[8], B[36] of every match of an edge whose cameras have the variants Vi, Vj (9, 10)"""
    x, y, u, v = (np.ascontiguousarray(xyuv[:, k]) for k in range(4))
    with np.errstate(all="ignore"):
        bi, bj = _rays(Vi[0], x, y), _rays(Vj[0], u, v)
        r = _residual(Vi[0], Vj[0], bi, bj)
        J = []
        for k in range(4):
            p = _residual(Vi[1 + 2 * k], Vj[0], _rays(Vi[1 + 2 * k], x, y), bj)
            m = _residual(Vi[2 + 2 * k], Vj[0], _rays(Vi[2 + 2 * k], x, y), bj)
            J.append([(p[c] - m[c]) * 500.0 for c in range(3)])
        for k in range(4):
            p = _residual(Vi[0], Vj[1 + 2 * k], bi, _rays(Vj[1 + 2 * k], u, v))
            m = _residual(Vi[0], Vj[2 + 2 * k], bi, _rays(Vj[2 + 2 * k], u, v))
            J.append([(p[c] - m[c]) * 500.0 for c in range(3)])
        out = np.zeros((len(x), 45), np.float64)
        out[:, 0] = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]
        for k in range(8):
            out[:, 1 + k] = (J[k][0] * r[0] + J[k][1] * r[1]) + J[k][2] * r[2]
        for t, (k, l) in enumerate(TRIU):
            out[:, 9 + t] = (J[k][0] * J[l][0] + J[k][1] * J[l][1]) + J[k][2] * J[l][2]
    return out


def ordered_sum(terms):
    """(45,) of terms (m, 45): 256 lanes, then eight halvings.  One vector add per chunk: no einsum, dot or sum"""
    m = len(terms)
    chunks = (m + LANES - 1) // LANES
    padded = np.zeros((max(chunks, 1) * LANES, terms.shape[1]), np.float64)
    padded[:m] = terms
    with np.errstate(all="ignore"):
        v = np.zeros((LANES, terms.shape[1]), np.float64)
        for c in range(chunks):
            v = v + padded[c * LANES:(c + 1) * LANES]
        s = LANES // 2
        while s:
            v = v[:s] + v[s:2 * s]
            s //= 2
    return v[0]


def normal_equations(features, matches, params, conf_thresh=1.0, pts=None):
    """E (e,), g (e, 8), B (e, 36) of the edges in ascending order"""
    n = len(features)
    V = variants(params)
    if pts is None:
        pts = [NM.centred(f) for f in features]
    ed = edges(matches, n, conf_thresh)
    out = np.zeros((len(ed), 45), np.float64)
    for k, (i, j) in enumerate(ed):
        out[k] = ordered_sum(match_terms(V[i], V[j], edge_points(features, matches, n, i, j, pts)))
    return out[:, 0].copy(), out[:, 1:9].copy(), out[:, 9:].copy()


def assemble(n, ed, E, g, B):
    """E, g (4n,), A (4n, 4n) of the edges' sums"""
    A, gv, total = np.zeros((4 * n, 4 * n), np.float64), np.zeros(4 * n, np.float64), 0.0
    for k, (i, j) in enumerate(ed):
        blk = np.zeros((8, 8), np.float64)
        for t, (a, b) in enumerate(TRIU):
            blk[a, b] = blk[b, a] = B[k, t]
        idx = np.array([4 * i, 4 * i + 1, 4 * i + 2, 4 * i + 3, 4 * j, 4 * j + 1, 4 * j + 2, 4 * j + 3])
        A[np.ix_(idx, idx)] += blk
        gv[idx] += g[k]
        total = total + E[k]
    return total, gv, A


def adjust(features, matches, cameras, conf_thresh=1.0, max_evals=100, evaluate=None):
    """cameras [(focal, R)] -> [(focal, R float32)], info.  evaluate(params) -> E, g, B replaces the evaluation (the tests count with it)"""
    n = len(features)
    pts = [NM.centred(f) for f in features]
    ed = edges(matches, n, conf_thresh)
    if evaluate is None:
        def evaluate(p):
            return normal_equations(features, matches, p, conf_thresh, pts)
    p = np.array([[f] + list(rodrigues_vector(R)) for f, R in cameras], np.float64)
    with np.errstate(all="ignore"):
        E, g, A = assemble(n, ed, *evaluate(p))
        info = {"edges": len(ed), "matches": int(sum(len(edge_points(features, matches, n, i, j, pts)) for i, j in ed)), "evaluations": 1,
                "accepted": 0, "first_E": float(E), "last_E": float(E)}
        lam = 1e-3
        while info["evaluations"] < max_evals:
            try:
                d = np.linalg.solve(A + lam * np.diag(np.diag(A)), -g)
            except np.linalg.LinAlgError:
                d = None
            better = False
            if d is not None and np.isfinite(variants(p + d.reshape(n, 4))).all():  # else a rejected step, not evaluated
                q = p + d.reshape(n, 4)
                E2, g2, A2 = assemble(n, ed, *evaluate(q))
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
    if not np.isfinite(p).all() or (p[:, 0] <= 0).any():
        raise ContractError("Camera parameters adjusting failed.")
    _, centre = spanning_tree(matches, n)
    if centre < 0:
        raise ContractError("Camera parameters adjusting failed.")
    R = [rodrigues(q[1:4]) for q in p]
    inv = np.linalg.inv(R[centre])
    return [(float(q[0]), (inv @ Ri).astype(np.float32)) for q, Ri in zip(p, R)], info


# ---- wave correction ---------------------------------------------------------------------------------------------------------------------
def wave_correct(Rs, kind="horiz", flip=False):
    """[R float32]; flip: take the eigenvector with the other sign (the result does not depend on it)"""
    if kind == "no":
        return [np.asarray(R) for R in Rs]
    if kind not in ("horiz", "vert"):
        raise ContractError(f"wave correction {kind!r} is not supported")
    Rs = [np.asarray(R, np.float64) for R in Rs]
    M = np.zeros((3, 3))
    for R in Rs:
        M = M + np.outer(R[:, 0], R[:, 0])
    _, vec = np.linalg.eigh(M)
    rg1 = vec[:, 0] if kind == "horiz" else vec[:, 2]
    if flip:
        rg1 = -rg1
    k = np.zeros(3)
    for R in Rs:
        k = k + R[:, 2]
    rg0 = np.cross(rg1, k)
    norm = np.sqrt((rg0 * rg0).sum())
    if not norm > 0:
        return [R.astype(np.float32) for R in Rs]
    rg0 = rg0 / norm
    rg2 = np.cross(rg0, rg1)
    if sum(float(rg0 @ R[:, 0]) for R in Rs) < 0:
        rg0, rg1 = -rg0, -rg1
    C = np.stack([rg0, rg1, rg2])
    return [(C @ R).astype(np.float32) for R in Rs]


def register(features, matches, conf_thresh=1.0, wave_correct_kind="horiz", max_evals=100):
    """-> indices, [{"focal", "R", "ppx", "ppy", "aspect"}], info of the adjustment"""
    n = len(features)
    indices = subset(matches, n, conf_thresh)
    features = [features[i] for i in indices]
    matches = subset_matches(matches, indices)
    cams, info = adjust(features, matches, estimate(features, matches), conf_thresh, max_evals)
    Rs = wave_correct([R for _, R in cams], wave_correct_kind)
    out = []
    for (f, _), R, feat in zip(cams, Rs, features):
        w0, h0 = _size(feat)
        out.append({"focal": f, "R": R, "ppx": w0 / 2, "ppy": h0 / 2, "aspect": 1.0})
    return indices, out, info
