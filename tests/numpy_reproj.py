"""Reprojection bundle adjustment of this project in numpy: the contract `stitching_amd.CameraSolver(model="reproj")` is tested against —
in the bits of all 120 float64 sums of every edge; the host part within 1e-9.

This is the project's OWN algorithm, in the way of OpenCV's BundleAdjusterReproj and its refinement mask.  It is NOT
cv.detail.BundleAdjusterReproj and answers to its name only through an injected solver whose own `model` says "reproj".  Nothing is
taken from the package.  What is not said here is tests/numpy_cameras.py's, unchanged: the subset, the focals, the spanning tree and its
rotations (estimate), the edges and their points (numpy_matches.centred: level-0 pixels relative to the image centre), the ordered sum,
the Rodrigues formulas, the Levenberg-Marquardt schedule, the wave correction.

  parameters  7 per camera, in this order: focal f, cx, cy, aspect a, rx, ry, rz.  cx, cy are the principal point's offsets from the
              image centre (the points are centred): cx = ppx - w0 / 2, cy = ppy - h0 / 2; after estimate they are 0 and a is 1.  The
              Rodrigues vector is that of the SVD-orthonormalised R (negated where det < 0), taken through the unit quaternion
              (rotation_vector below): the principal point and the aspect are observed weakly, so that a start that differs in its
              last bit moves them by far more than 1e-9, and the start is therefore stated to the operation
  variants    (n, 15, 18): the base, then + and - 1e-3 on each parameter (+ before -).  A variant is two 3 x 3 matrices, row-major,
              with R = Rodrigues(r'), every product and sum rounded by itself:
                P = R K^-1:   P[c][0] = R[c][0] (1 / f);  P[c][1] = R[c][1] (1 / (f a));
                              P[c][2] = (R[c][0] (-(cx / f)) + R[c][1] (-(cy / (f a)))) + R[c][2]
                Q = K R^T:    Q[0][c] = f R[c][0] + cx R[c][2];  Q[1][c] = (f a) R[c][1] + cy R[c][2];  Q[2][c] = R[c][2]
              K = [[f, 0, cx], [0, f a, cy], [0, 0, 1]].  The variants are made on the host and uploaded: host and device read the same bits
  residual    of a match (x, y) | (u, v) of an edge i < j, in image j's pixels, one direction only:
                X_c = (P_i[c][0] x + P_i[c][1] y) + P_i[c][2];  Y_c = (Q_j[c][0] X_0 + Q_j[c][1] X_1) + Q_j[c][2] X_2
                r = (u - Y_0 / Y_2, v - Y_1 / Y_2)          IEEE divide; no special case for Y_2 <= 0
  Jacobian    14 columns: column k < 7 from the + and - variant of parameter k of camera i with camera j at its base; column 7 + k from
              the + and - variant of parameter k of camera j with the base X.  J = (r(+) - r(-)) 500
  sums        120 terms a match: E += r . r; g_k += J_k . r (14); B_kl += J_k . J_l for k <= l (105, upper triangle row-major); every
              dot product a0 b0 + a1 b1; summed by numpy_cameras.ordered_sum (256 lanes, then eight halvings).  Nothing fused
  mask        five characters, each "x" (free) or "_" (held), in the cell order of the reference's refinement mask: 0 focal, 1 skew
              (there is no skew parameter: accepted and ignored), 2 ppx, 3 aspect, 4 ppy.  The rotation is always free.  All 120 sums
              are always computed; the rows and columns of held parameters are removed from the 7n x 7n system before
              (A + lam diag A) d = -g, and held parameters are never written: they come back bit-equal to their start
  LM          numpy_cameras' loop on that system; afterwards R_i <- R_centre^-1 R_i.  A parameter that is not finite, focal <= 0 or
              aspect <= 0: "Camera parameters adjusting failed."  Cameras come back with focal, aspect, ppx = w0 / 2 + cx,
              ppy = h0 / 2 + cy and a float32 R
"""
import math

import numpy as np

from tests import numpy_cameras as NC
from tests import numpy_matches as NM

STEP = NC.STEP
WIDTH = 7  # parameters per camera
SUMS = 120
TRIU = [(k, l) for k in range(14) for l in range(k, 14)]
FULL_MASK = "xxxxx"
_MASK_CELL = {0: 0, 1: 2, 2: 4, 3: 3}  # parameter (focal, cx, cy, aspect) -> its character of the mask


def free_parameters(mask):
    """the indices 0 .. 6 of the parameters of one camera that move under the mask, ascending"""
    if not isinstance(mask, str) or len(mask) != 5 or any(ch not in "x_" for ch in mask):
        raise NC.ContractError(f"refinement mask {mask!r}: five characters, each 'x' or '_'")
    return [k for k in range(4) if mask[_MASK_CELL[k]] == "x"] + [4, 5, 6]


def rotation_vector(R):
    """(3, 3) -> Rodrigues vector of the nearest rotation u v^T of the SVD (negated where the determinant is negative), through the unit
    quaternion (w, v): the largest of trace, R00, R11, R22 picks the component that comes from a square root — w = sqrt(1 + trace) / 2,
    v = (R21 - R12, R02 - R20, R10 - R01) / (4 w), or v_i = sqrt(1 + R_ii - R_jj - R_kk) / 2 with v_j = (R_ji + R_ij) / (4 v_i),
    v_k = (R_ki + R_ik) / (4 v_i), w = (R_kj - R_jk) / (4 v_i) for (i, j, k) cyclic; w < 0 negates all four; the vector is
    v (2 atan2(|v|, w) / |v|), and 0 where |v| is 0"""
    u, _, vt = np.linalg.svd(np.asarray(R, np.float64))
    R = u @ vt
    if np.linalg.det(R) < 0:
        R = -R
    trace = R[0, 0] + R[1, 1] + R[2, 2]
    lead = int(np.argmax([trace, R[0, 0], R[1, 1], R[2, 2]]))
    if lead == 0:
        w = 0.5 * math.sqrt(max(1.0 + trace, 0.0))
        v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / (4.0 * w)
    else:
        i = lead - 1
        j, k = (i + 1) % 3, (i + 2) % 3
        v = np.zeros(3)
        v[i] = 0.5 * math.sqrt(max(1.0 + R[i, i] - R[j, j] - R[k, k], 0.0))
        v[j] = (R[j, i] + R[i, j]) / (4.0 * v[i])
        v[k] = (R[k, i] + R[i, k]) / (4.0 * v[i])
        w = (R[k, j] - R[j, k]) / (4.0 * v[i])
    if w < 0:
        w, v = -w, -v
    length = math.sqrt(float(v @ v))
    return v * (2.0 * math.atan2(length, w) / length) if length > 0 else np.zeros(3)


def variant(q):
    """(18,) float64 of one parameter row: P, then Q"""
    f, cx, cy, a = (np.float64(v) for v in q[:4])
    R = NC.rodrigues(q[4:7])
    fa = f * a
    s0, s1 = 1.0 / f, 1.0 / fa
    t0, t1 = -(cx / f), -(cy / fa)
    P, Q = np.zeros((3, 3), np.float64), np.zeros((3, 3), np.float64)
    for c in range(3):
        P[c, 0] = R[c, 0] * s0
        P[c, 1] = R[c, 1] * s1
        P[c, 2] = (R[c, 0] * t0 + R[c, 1] * t1) + R[c, 2]
        Q[0, c] = f * R[c, 0] + cx * R[c, 2]
        Q[1, c] = fa * R[c, 1] + cy * R[c, 2]
        Q[2, c] = R[c, 2]
    return np.concatenate([P.reshape(9), Q.reshape(9)])


def variants(params):
    """(n, 15, 18) float64 of params (n, 7): the base, then + and - STEP on each parameter"""
    params = np.asarray(params, np.float64).reshape(-1, WIDTH)
    out = np.zeros((len(params), 15, 18), np.float64)
    with np.errstate(all="ignore"):
        for c, p in enumerate(params):
            rows = [p + np.zeros(WIDTH)]
            for k in range(WIDTH):
                for sign in (1.0, -1.0):
                    shift = np.zeros(WIDTH)
                    shift[k] = sign * STEP
                    rows.append(p + shift)
            for v, q in enumerate(rows):
                out[c, v] = variant(q)
    return out


def _world(V, x, y):
    return [(V[3 * c] * x + V[3 * c + 1] * y) + V[3 * c + 2] for c in range(3)]


def _residual(V, X, u, v):
    Y = [(V[9 + 3 * c] * X[0] + V[10 + 3 * c] * X[1]) + V[11 + 3 * c] * X[2] for c in range(3)]
    return [u - Y[0] / Y[2], v - Y[1] / Y[2]]


def match_terms(Vi, Vj, xyuv):
    """(m, 120) float64: the terms E, g[14], B[105] of every match of an edge whose cameras have the variants Vi, Vj (15, 18)"""
    x, y, u, v = (np.ascontiguousarray(xyuv[:, k]) for k in range(4))
    with np.errstate(all="ignore"):
        X = _world(Vi[0], x, y)
        r = _residual(Vj[0], X, u, v)
        J = []
        for k in range(WIDTH):
            p = _residual(Vj[0], _world(Vi[1 + 2 * k], x, y), u, v)
            m = _residual(Vj[0], _world(Vi[2 + 2 * k], x, y), u, v)
            J.append([(p[c] - m[c]) * 500.0 for c in range(2)])
        for k in range(WIDTH):
            p = _residual(Vj[1 + 2 * k], X, u, v)
            m = _residual(Vj[2 + 2 * k], X, u, v)
            J.append([(p[c] - m[c]) * 500.0 for c in range(2)])
        out = np.zeros((len(x), SUMS), np.float64)
        out[:, 0] = r[0] * r[0] + r[1] * r[1]
        for k in range(14):
            out[:, 1 + k] = J[k][0] * r[0] + J[k][1] * r[1]
        for t, (k, l) in enumerate(TRIU):
            out[:, 15 + t] = J[k][0] * J[l][0] + J[k][1] * J[l][1]
    return out


def normal_equations(features, matches, params, conf_thresh=1.0, pts=None):
    """E (e,), g (e, 14), B (e, 105) of the edges in ascending order"""
    n = len(features)
    V = variants(params)
    if pts is None:
        pts = [NM.centred(f) for f in features]
    ed = NC.edges(matches, n, conf_thresh)
    out = np.zeros((len(ed), SUMS), np.float64)
    for k, (i, j) in enumerate(ed):
        out[k] = NC.ordered_sum(match_terms(V[i], V[j], NC.edge_points(features, matches, n, i, j, pts)))
    return out[:, 0].copy(), out[:, 1:15].copy(), out[:, 15:].copy()


def assemble(n, ed, E, g, B):
    """E, g (7n,), A (7n, 7n) of the edges' sums, added in ascending order; each 14 x 14 block mirrored"""
    A, gv, total = np.zeros((WIDTH * n, WIDTH * n), np.float64), np.zeros(WIDTH * n, np.float64), 0.0
    for k, (i, j) in enumerate(ed):
        blk = np.zeros((14, 14), np.float64)
        for t, (a, b) in enumerate(TRIU):
            blk[a, b] = blk[b, a] = B[k, t]
        idx = np.array([WIDTH * i + c for c in range(WIDTH)] + [WIDTH * j + c for c in range(WIDTH)])
        A[np.ix_(idx, idx)] += blk
        gv[idx] += g[k]
        total = total + E[k]
    return total, gv, A


def start_parameters(features, cameras):
    """(n, 7) float64 of cameras [(focal, R)] (offsets 0, aspect 1) or [(focal, R, ppx, ppy, aspect)] (ppx, ppy in image pixels)"""
    out = np.zeros((len(cameras), WIDTH), np.float64)
    for k, (cam, feat) in enumerate(zip(cameras, features)):
        w0, h0 = NC._size(feat)
        f, R = cam[0], cam[1]
        ppx, ppy, a = (cam[2], cam[3], cam[4]) if len(cam) > 2 else (w0 / 2, h0 / 2, 1.0)
        out[k] = [f, ppx - w0 / 2, ppy - h0 / 2, a] + list(rotation_vector(R))
    return out


def adjust(features, matches, cameras, mask=FULL_MASK, conf_thresh=1.0, max_evals=100, evaluate=None):
    """cameras as start_parameters takes them -> [(focal, R float32, ppx, ppy, aspect)], info.  evaluate(params) -> E, g, B replaces the
    evaluation (the tests count with it)"""
    n = len(features)
    pts = [NM.centred(f) for f in features]
    ed = NC.edges(matches, n, conf_thresh)
    if evaluate is None:
        def evaluate(p):
            return normal_equations(features, matches, p, conf_thresh, pts)
    free = np.array([WIDTH * c + k for c in range(n) for k in free_parameters(mask)])
    p = start_parameters(features, cameras)
    start = p.copy()

    def moved(d):
        q = p.copy()
        q.reshape(-1)[free] = p.reshape(-1)[free] + d  # a held parameter is never written
        return q

    with np.errstate(all="ignore"):
        E, g, A = assemble(n, ed, *evaluate(p))
        info = {"edges": len(ed), "matches": int(sum(len(NC.edge_points(features, matches, n, i, j, pts)) for i, j in ed)), "evaluations": 1,
                "accepted": 0, "first_E": float(E), "last_E": float(E)}
        lam = 1e-3
        while info["evaluations"] < max_evals:
            Af, gf = A[np.ix_(free, free)], g[free]
            try:
                d = np.linalg.solve(Af + lam * np.diag(np.diag(Af)), -gf)
            except np.linalg.LinAlgError:
                d = None
            better = False
            if d is not None and np.isfinite(variants(moved(d))).all():  # else a rejected step, not evaluated
                q = moved(d)
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
    info["last_E"], info["parameters"], info["start"] = float(E), p.copy(), start
    if not np.isfinite(p).all() or (p[:, 0] <= 0).any() or (p[:, 3] <= 0).any():
        raise NC.ContractError("Camera parameters adjusting failed.")
    _, centre = NC.spanning_tree(matches, n)
    if centre < 0:
        raise NC.ContractError("Camera parameters adjusting failed.")
    R = [NC.rodrigues(q[4:7]) for q in p]
    inv = np.linalg.inv(R[centre])
    out = []
    for q, Ri, feat in zip(p, R, features):
        w0, h0 = NC._size(feat)
        out.append((float(q[0]), (inv @ Ri).astype(np.float32), w0 / 2 + float(q[1]), h0 / 2 + float(q[2]), float(q[3])))
    return out, info


def register(features, matches, mask=FULL_MASK, conf_thresh=1.0, wave_correct_kind="horiz", max_evals=100):
    """-> indices, [{"focal", "R", "ppx", "ppy", "aspect"}], info of the adjustment"""
    n = len(features)
    indices = NC.subset(matches, n, conf_thresh)
    features = [features[i] for i in indices]
    matches = NC.subset_matches(matches, indices)
    cams, info = adjust(features, matches, NC.estimate(features, matches), mask, conf_thresh, max_evals)
    Rs = NC.wave_correct([c[1] for c in cams], wave_correct_kind)
    return indices, [{"focal": c[0], "R": R, "ppx": c[2], "ppy": c[3], "aspect": c[4]} for c, R in zip(cams, Rs)], info
