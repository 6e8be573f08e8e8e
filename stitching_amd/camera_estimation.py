"""Camera registration: which images belong to the panorama, their focals and rotations, a ray bundle adjustment on the device, and
wave correction.

`CameraSolver` is the project's OWN solver, in the way of OpenCV's homography-based estimator, ray adjuster and wave correction.  It is
NOT cv.detail.HomographyBasedEstimator, BundleAdjusterRay or waveCorrect and answers to none of their names: "homography", "ray" and
the wave-correction kinds by name stay cv2's (subsetter.Subsetter, camera_estimator.CameraEstimator, camera_adjuster.CameraAdjuster,
camera_wave_corrector.WaveCorrector take it as solver=).  tests/numpy_cameras.py states it exactly and is the contract.

The work that grows with the matches — per Levenberg-Marquardt step the residuals of every inlier match of every confident pair and
their Jacobian with respect to both cameras, summed into the normal equations — is one launch per step over matches that stay on the
device (csrc/stx_cameras.hip), equal to the contract in the bits of all 45 float64 sums of an edge; DESIGN.md section 17 has the kernel
and the limits.  What is small and wants float64 with a library behind it is numpy on the host: the subset, the focals, the spanning
tree and its rotations, the 9 variants of every camera, the 4n x 4n solve, the wave correction.

With model="affine" the same solver registers scans and flat tiles: a camera is a transform of the plane (camera.R the 3 x 3 map from
image pixels to the panorama plane, focal = 1, ppx = ppy = 0, as the affine warper takes it), estimated along the same spanning tree
and refined as a similarity (a, b, tx, ty) by the same Levenberg-Marquardt loop over a residual in pixels; tests/numpy_affine.py is
that contract and DESIGN.md section 18 the description.

With model="reproj" the registration is the rotation model's except for the adjustment: 7 parameters per camera (focal, the principal
point, the aspect, the Rodrigues vector) over the reprojection error in pixels, 120 sums per edge from one launch of a (edges, 3) grid,
and a refinement mask that holds focal, principal point or aspect where they started; tests/numpy_reproj.py is that contract and
DESIGN.md section 19 the description.
"""
import ctypes as C
import math
import warnings

import numpy as np

from . import _lib
from ._marshal import info_dict, ptr
from .camera import CameraParams
from .device import get_context
from .match_estimation import centred_points, level0_points
from .stitching_error import StitchingError, StitchingWarning

STEP = 1e-3  # of the central differences, on every parameter
MODELS = ("rotation", "affine", "reproj")
FULL_MASK = "xxxxx"  # the refinement mask under which every parameter moves
_UNSET = object()  # a wave_correct that was not passed: "horiz" for rotations, "no" for the affine model
WAVE_KINDS = ("horiz", "vert", "no")
NO_MATCH_MESSAGE = ("No match exceeds the given confidence threshold. Do your images have enough overlap and common features? If yes, "
                    "you might want to lower the 'confidence_threshold' or try another 'detector'.")
NOT_ALL_MESSAGE = ("Not all images are included in the final panorama. If this is not intended, use the 'matches_graph_dot_file' "
                   "parameter to analyze your matches. You might want to lower the 'confidence_threshold' or try another 'detector' to "
                   "include all your images.")
_TRI = {4: np.triu_indices(8), 7: np.triu_indices(14)}  # parameters per camera -> the upper triangle of an edge's block
_MASK_CELL = (0, 2, 4, 3)  # focal, ppx, ppy, aspect -> their characters of a refinement mask (1 is the skew, which is no parameter)


def free_parameters(mask):
    """the indices 0 .. 6 of the reprojection model's parameters (focal, ppx, ppy, aspect, rx, ry, rz) that move under a refinement mask,
    ascending; the rotation always does"""
    if not isinstance(mask, str) or len(mask) != 5 or any(ch not in "x_" for ch in mask):
        raise StitchingError(f"refinement mask {mask!r}: five characters, each 'x' (refined) or '_' (held)")
    return [k for k in range(4) if mask[_MASK_CELL[k]] == "x"] + [4, 5, 6]


# ---- subset ------------------------------------------------------------------------------------------------------------------------------
def largest_component(conf, conf_thresh):
    """Ascending indices of the largest group of images joined by pairs i < j with conf[i, j] >= conf_thresh; among groups of equal
    size the one that holds the smallest index."""
    n = len(conf)
    label = np.arange(n)
    for i in range(n):
        for j in range(i + 1, n):
            if conf[i, j] >= conf_thresh and label[i] != label[j]:
                lo, hi = sorted((int(label[i]), int(label[j])))
                label[label == hi] = lo  # a group is named by its smallest member
    names, counts = np.unique(label, return_counts=True)
    if n == 0:
        return []
    return np.flatnonzero(label == names[np.argmax(counts)]).tolist()  # argmax: the first maximum, names ascend


def confidences(matches, n):
    return np.array([[float(matches[i * n + j].confidence) for j in range(n)] for i in range(n)], np.float64).reshape(n, n)


# ---- focals ------------------------------------------------------------------------------------------------------------------------------
def _focal_choice(v1, v2, d1, d2):
    """the focal of two candidate squares v = numerator / d: the larger one where it alone is positive; where both are, the one with the
    larger |d| (the better conditioned quotient)"""
    larger, smaller = ((v2, d2), (v1, d1)) if v1 < v2 else ((v1, d1), (v2, d2))
    if not larger[0] > 0:
        return None
    square = larger[0]
    if smaller[0] > 0 and not abs(larger[1]) > abs(smaller[1]):
        square = smaller[0]
    return float(np.sqrt(square)) if np.isfinite(square) else None


def focals_from_homography(H):
    """The two focal candidates (f0 of the source image, f1 of the destination) of a homography between two views of a rotating camera
    with the principal point at the origin, each None where its closed form has no positive solution (a pure translation, say)."""
    a, b, c, d, e, f, g, h, _ = np.asarray(H, np.float64).reshape(9)
    with np.errstate(all="ignore"):
        f1 = _focal_choice(-(a * b + d * e) / (g * h), (a * a + d * d - b * b - e * e) / ((h - g) * (h + g)), g * h, (h - g) * (h + g))
        f0 = _focal_choice(-c * f / (a * d + b * e), (f * f - c * c) / (a * a + b * b - d * d - e * e), a * d + b * e,
                           a * a + b * b - d * d - e * e)
    return f0, f1


def starting_focal(features, matches):
    """One focal for all cameras: the median of sqrt(f0 f1) over the pairs i < j whose homography gives both, where there are at least
    n - 1 of them; else the mean of width + height."""
    n = len(features)
    got = []
    for i in range(n):
        for j in range(i + 1, n):
            H = matches[i * n + j].H
            if H is not None:
                f0, f1 = focals_from_homography(H)
                if f0 is not None and f1 is not None:
                    got.append(math.sqrt(f0 * f1))
    if len(got) >= n - 1:
        got.sort()
        half = len(got) // 2
        return got[half] if len(got) % 2 else (got[half - 1] + got[half]) * 0.5
    return sum(f.img_size[0] + f.img_size[1] for f in features) / n


# ---- spanning tree and rotations -----------------------------------------------------------------------------------------------------------
def spanning_tree(matches, n):
    """(neighbour lists in ascending order, centre) of the maximum spanning tree over the pairs with a homography — Kruskal by
    num_inliers descending, then (i, j) ascending; the centre is the node of least eccentricity, the smallest index among equals.
    (None, -1) where those pairs do not connect all n images."""
    edges = []
    for i in range(n):
        for j in range(i + 1, n):
            e = matches[i * n + j]
            if e.H is None:
                e = matches[j * n + i]
            if e.H is not None:
                edges.append((-int(e.num_inliers), i, j))
    edges.sort()
    group = list(range(n))
    near = [[] for _ in range(n)]
    taken = 0
    for _, i, j in edges:
        if group[i] != group[j]:
            old, new = group[i], group[j]
            group = [new if g == old else g for g in group]
            near[i].append(j)
            near[j].append(i)
            taken += 1
    if taken != n - 1:
        return None, -1
    near = [sorted(a) for a in near]
    reach = [max(_hops(near, s)) for s in range(n)]
    return near, int(np.argmin(reach))


def _hops(near, start):
    hops = {start: 0}
    front = [start]
    while front:
        nxt = []
        for a in front:
            for b in near[a]:
                if b not in hops:
                    hops[b] = hops[a] + 1
                    nxt.append(b)
        front = nxt
    return [hops[k] for k in range(len(near))]


def _homography(matches, n, a, b):
    H = matches[a * n + b].H
    if H is not None:
        return np.asarray(H, np.float64)
    return np.linalg.inv(np.asarray(matches[b * n + a].H, np.float64))


def tree_rotations(matches, n, focals):
    """float64 rotations along the spanning tree from its centre (R = I there): R_to = R_from (K_from^-1 H_from->to^-1 K_to)"""
    near, centre = spanning_tree(matches, n)
    if near is None:
        raise StitchingError("Homography estimation failed.")
    R = {centre: np.eye(3)}
    front = [centre]
    while front:
        nxt = []
        for a in front:
            for b in near[a]:
                if b not in R:
                    k_from_inv = np.diag([1.0 / focals[a], 1.0 / focals[a], 1.0])
                    k_to = np.diag([focals[b], focals[b], 1.0])
                    R[b] = R[a] @ (k_from_inv @ np.linalg.inv(_homography(matches, n, a, b)) @ k_to)
                    nxt.append(b)
        front = nxt
    return [R[k] for k in range(n)]


def tree_transforms(matches, n):
    """float64 affine transforms along the spanning tree from its centre (T = I there): T_to = T_from H_(to -> from), image pixels to
    the centre image's pixels"""
    near, centre = spanning_tree(matches, n)
    if near is None:
        raise StitchingError("Homography estimation failed.")
    T = {centre: np.eye(3)}
    front = [centre]
    while front:
        nxt = []
        for a in front:
            for b in near[a]:
                if b not in T:
                    T[b] = T[a] @ _homography(matches, n, b, a)
                    nxt.append(b)
        front = nxt
    return [T[k] for k in range(n)]


# ---- Rodrigues -----------------------------------------------------------------------------------------------------------------------------
def rotation_matrix(r):
    """Rodrigues vector -> (3, 3) float64: (1 - c) k k^T + c I + s [k]x with (1 - c) k_a multiplied first, as the contract writes it"""
    r = np.asarray(r, np.float64)
    th = np.sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2])
    if not th >= 1e-12:
        return np.eye(3) if th == th else np.full((3, 3), np.nan)
    c, s = np.cos(th), np.sin(th)
    k = r / th
    sk = s * k
    return ((1.0 - c) * k)[:, None] * k[None, :] + np.array([[c, -sk[2], sk[1]], [sk[2], c, -sk[0]], [-sk[1], sk[0], c]])


def rotation_vector(R):
    """(3, 3) -> Rodrigues vector of the nearest rotation (SVD; negated where the determinant is negative), through the unit quaternion:
    its largest component comes from a square root of the trace or of a diagonal element, the others from sums and differences of
    off-diagonal pairs — no branch of its own for small turns or half turns.  A half turn comes out with either sign of its axis."""
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


def camera_variants(params):
    """(n, 9, 10) float64 for params (n, 4) rows focal, rx, ry, rz: per camera its parameters, then + and - STEP on each of the four
    (+ before -); a variant is f' and H' = R(r') diag(1 / f', 1 / f', 1), row-major."""
    params = np.ascontiguousarray(params, np.float64).reshape(-1, 4)
    shifts = np.zeros((9, 4), np.float64)
    for k in range(4):
        shifts[1 + 2 * k, k], shifts[2 + 2 * k, k] = STEP, -STEP
    out = np.zeros((len(params), 9, 10), np.float64)
    with np.errstate(all="ignore"):
        moved = params[:, None, :] + shifts[None, :, :]
        out[:, :, 0] = moved[:, :, 0]
        scale = np.ones((len(params), 9, 3), np.float64)
        scale[:, :, 0] = scale[:, :, 1] = 1.0 / moved[:, :, 0]
        for c in range(len(params)):
            for v in range(9):
                out[c, v, 1:] = (rotation_matrix(moved[c, v, 1:]) * scale[c, v][None, :]).reshape(9)
    return out


def similarity_parameters(R):
    """a, b, tx, ty of the similarity nearest to the linear part of the transform R, its translation kept"""
    T = np.asarray(R, np.float64)
    return [(T[0, 0] + T[1, 1]) / 2, (T[1, 0] - T[0, 1]) / 2, T[0, 2], T[1, 2]]


def similarity_matrix(p):
    a, b, tx, ty = (float(v) for v in p)
    return np.array([[a, -b, tx], [b, a, ty], [0.0, 0.0, 1.0]])


def similarity_variants(params):
    """(n, 9, 8) float64 for params (n, 4) rows a, b, tx, ty: per camera its parameters, then + and - STEP on each of the four (+ before
    -); a variant is the map a, b, tx, ty and its inverse a' = a / d, b' = -b / d, tx' = -(a' tx - b' ty), ty' = -(b' tx + a' ty),
    d = a a + b b (not finite where d is 0)."""
    params = np.ascontiguousarray(params, np.float64).reshape(-1, 4)
    shifts = np.zeros((9, 4), np.float64)
    for k in range(4):
        shifts[1 + 2 * k, k], shifts[2 + 2 * k, k] = STEP, -STEP
    out = np.zeros((len(params), 9, 8), np.float64)
    with np.errstate(all="ignore"):
        moved = params[:, None, :] + shifts[None, :, :]
        a, b, tx, ty = (moved[:, :, k] for k in range(4))
        d = a * a + b * b
        ai, bi = a / d, -b / d
        out[:, :, 0:4] = moved
        out[:, :, 4], out[:, :, 5] = ai, bi
        out[:, :, 6], out[:, :, 7] = -(ai * tx - bi * ty), -(bi * tx + ai * ty)
    return out


def reproj_variants(params):
    """(n, 15, 18) float64 for params (n, 7) rows focal, cx, cy, aspect, rx, ry, rz (cx, cy: the principal point relative to the image
    centre): per camera its parameters, then + and - STEP on each of the seven (+ before -); a variant is P = R(r') K'^-1 and
    Q = K' R(r')^T, row-major, K' = [[f, 0, cx], [0, f a, cy], [0, 0, 1]], in the contract's order of operations."""
    params = np.ascontiguousarray(params, np.float64).reshape(-1, 7)
    n = len(params)
    shifts = np.zeros((15, 7), np.float64)
    for k in range(7):
        shifts[1 + 2 * k, k], shifts[2 + 2 * k, k] = STEP, -STEP
    out = np.zeros((n, 15, 18), np.float64)
    with np.errstate(all="ignore"):
        moved = params[:, None, :] + shifts[None, :, :]
        f, cx, cy, a = (moved[:, :, k] for k in range(4))
        fa = f * a
        s0, s1, t0, t1 = 1.0 / f, 1.0 / fa, -(cx / f), -(cy / fa)
        R = np.zeros((n, 15, 3, 3), np.float64)
        for c in range(n):
            for v in range(15):
                R[c, v] = rotation_matrix(moved[c, v, 4:])
        P, Q = out[:, :, :9].reshape(n, 15, 3, 3), out[:, :, 9:].reshape(n, 15, 3, 3)
        for c in range(3):
            P[:, :, c, 0] = R[:, :, c, 0] * s0
            P[:, :, c, 1] = R[:, :, c, 1] * s1
            P[:, :, c, 2] = (R[:, :, c, 0] * t0 + R[:, :, c, 1] * t1) + R[:, :, c, 2]
            Q[:, :, 0, c] = f * R[:, :, c, 0] + cx * R[:, :, c, 2]
            Q[:, :, 1, c] = fa * R[:, :, c, 1] + cy * R[:, :, c, 2]
            Q[:, :, 2, c] = R[:, :, c, 2]
    return out


# ---- the ray problem on the device ---------------------------------------------------------------------------------------------------------
def ray_edges(matches, n, conf_thresh):
    """the pairs i < j whose confidence is above conf_thresh, ascending"""
    return [(i, j) for i in range(n) for j in range(i + 1, n) if matches[i * n + j].confidence > conf_thresh]


def edge_points(features, matches, edges, pts=None):
    """offsets (e + 1,) int64 and xyuv (total, 4) float64: per edge its inlier matches in match order, (x, y) of image i and (u, v) of
    image j in centred level-0 pixels"""
    n = len(features)
    if pts is None:
        pts = [centred_points(f) for f in features]
    blocks, offsets = [np.zeros((0, 4), np.float64)], np.zeros(len(edges) + 1, np.int64)
    for k, (i, j) in enumerate(edges):
        e = matches[i * n + j]
        keep = np.asarray(e.inliers_mask) != 0
        mt = np.asarray(e.matches).reshape(-1, 3)[keep]
        blocks.append(np.concatenate([pts[i][mt[:, 0]].reshape(-1, 2), pts[j][mt[:, 1]].reshape(-1, 2)], axis=1))
        offsets[k + 1] = offsets[k] + len(mt)
    return offsets, np.ascontiguousarray(np.concatenate(blocks, axis=0))


class RayProblem:
    """The edges of one adjustment on the device (stx_ray_problem): uploaded once, evaluated once per Levenberg-Marquardt step.  Use it
    as a context manager: the handle must go before its context does."""

    def __init__(self, edges, offsets, xyuv, ctx=None, model="rotation"):
        """model "affine": the edges are the same; an evaluation takes (n, 9, 8) similarity variants (stx_affine_problem_eval); model
        "reproj": (n, 15, 18) variants, 120 sums an edge (stx_reproj_problem_eval)"""
        self.ctx = ctx or get_context()
        self.model = model
        self.n_edges = len(edges)
        self._h = C.c_void_p()
        cams = np.ascontiguousarray(np.asarray(edges, np.int32).reshape(-1, 2))
        offsets = np.ascontiguousarray(offsets, np.int64)
        xyuv = np.ascontiguousarray(xyuv, np.float64)
        _lib.check(self.ctx._lib.stx_ray_problem_create(self.ctx.handle, self.n_edges, ptr(cams), ptr(offsets), ptr(xyuv), C.byref(self._h)))
        self.info = None

    def evaluate(self, variants):
        """(n, 9, 10) variants -> (e, 45) float64 sums E, g[8], B[36] of every edge ("reproj": (n, 15, 18) -> (e, 120), E, g[14], B[105]);
        one launch, one wait"""
        variants = np.ascontiguousarray(variants, np.float64)
        if self.model == "affine" and (variants.ndim != 3 or variants.shape[1:] != (9, 8)):
            raise StitchingError(f"variants of shape {variants.shape}: the affine adjustment takes (cameras, 9, 8)")
        if self.model == "reproj" and (variants.ndim != 3 or variants.shape[1:] != (15, 18)):
            raise StitchingError(f"variants of shape {variants.shape}: the reprojection adjustment takes (cameras, 15, 18)")
        out, info = np.zeros((self.n_edges, 120 if self.model == "reproj" else 45), np.float64), np.zeros(4, np.float64)
        entry = {"affine": self.ctx._lib.stx_affine_problem_eval, "reproj": self.ctx._lib.stx_reproj_problem_eval}.get(
            self.model, self.ctx._lib.stx_ray_problem_eval)
        _lib.check(entry(self._h, int(variants.shape[0]), ptr(variants), ptr(out), ptr(info)))
        self.info = info_dict(info, [("edges", int), ("matches", int), ("device_ms", float), ("device_ms_with_copy", float)])
        return out

    def free(self):
        h, self._h = self._h, C.c_void_p()
        if h:
            _lib.check(self.ctx._lib.stx_ray_problem_free(h))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()


def assemble_system(n, edges, sums, width=4):
    """E, g (4n,), A (4n, 4n) from the (e, 45) sums of the edges, added in ascending order; each 8 x 8 block mirrored to its lower half.
    width = 7 (the reprojection model): 7n unknowns from (e, 120) sums, blocks of 14 x 14"""
    w, tri = width, _TRI[width]
    A, g, E = np.zeros((w * n, w * n), np.float64), np.zeros(w * n, np.float64), 0.0
    for (i, j), row in zip(edges, sums):
        block = np.zeros((2 * w, 2 * w), np.float64)
        block[tri] = row[1 + 2 * w:]
        block.T[tri] = row[1 + 2 * w:]
        at = np.r_[w * i:w * i + w, w * j:w * j + w]
        A[np.ix_(at, at)] += block
        g[at] += row[1:1 + 2 * w]
        E = E + row[0]
    return E, g, A


# ---- wave correction -------------------------------------------------------------------------------------------------------------------------
def wave_corrected(rotations, kind):
    """float32 rotations with the waviness of a hand-held sweep taken out: one rotation for all cameras whose second row is, for
    "horiz", the normal of the plane the cameras' x axes lie nearest to, and for "vert" the direction those axes share."""
    if kind == "no":
        return [np.asarray(R) for R in rotations]
    Rs = np.stack([np.asarray(R, np.float64) for R in rotations])
    xs = Rs[:, :, 0]
    moment = np.zeros((3, 3))
    for x in xs:
        moment = moment + x[:, None] * x[None, :]
    _, vectors = np.linalg.eigh(moment)
    up = vectors[:, 0] if kind == "horiz" else vectors[:, 2]
    forward = np.zeros(3)
    for R in Rs:
        forward = forward + R[:, 2]
    right = np.cross(up, forward)
    length = np.sqrt((right * right).sum())
    if not length > 0:
        return [R.astype(np.float32) for R in Rs]
    right = right / length
    ahead = np.cross(right, up)
    if sum(float(right @ x) for x in xs) < 0:
        right, up = -right, -up
    turn = np.stack([right, up, ahead])
    return [(turn @ R).astype(np.float32) for R in Rs]


class CameraSolver:
    """The project's own camera registration — NOT cv.detail.HomographyBasedEstimator, BundleAdjusterRay or waveCorrect, and not behind
    their names.  From the ImageFeatures of FeatureEstimator.detect and the n * n MatchesInfo of MatchEstimator.match:

        subset    the largest group of images joined by pairs of confidence >= conf_thresh
        estimate  one focal from the homographies' closed form, rotations along the maximum spanning tree
        adjust    Levenberg-Marquardt on focal + Rodrigues vector per camera over the rays of every inlier match of every pair with
                  confidence > conf_thresh; the normal equations of a step are one launch on the device
        correct   wave correction "horiz", "vert" or "no"
        register  all four -> (indices, cameras)

    tests/numpy_cameras.py states it exactly and is the contract; DESIGN.md section 17 has the launch shape.  Construction needs no GPU.
    Limits, refused with a StitchingError before anything is launched: at most MAX_CAMERAS images, at most MAX_MATCHES inlier matches
    on a pair, parameters that are finite.  Nothing handed in is written; cameras come back as new CameraParams with a float32 R.

    model="affine" (scans and flat tiles, on the matches of MatchEstimator(model="affine")): estimate chains the pairs' transforms along
    the spanning tree (R is the 3 x 3 map from image pixels to the panorama plane, focal = 1, ppx = ppy = 0); adjust refines a
    similarity a, b, tx, ty per camera over the residual (u, v) - T_j^-1 T_i (x, y) in pixels, one launch a step as well; there is no
    wave correction (a wave_correct that is not passed means "no", "horiz" and "vert" are refused).  tests/numpy_affine.py is that
    contract; DESIGN.md section 18.

    model="reproj" (frames cropped off-centre, pixels that are not square): subset, estimate, correct and register are the rotation
    model's; adjust refines focal, principal point, aspect and Rodrigues vector of every camera over the reprojection error
    (u, v) - project(K_j R_j^T R_i K_i^-1 (x, y, 1)) in pixels, 120 sums an edge from one launch a step.  refinement_mask: five
    characters "x" (refined) or "_" (held) in the reference's cell order — focal, skew (no parameter: ignored), ppx, aspect, ppy; held
    parameters come back exactly as they went in, the rotation always moves.  It is the project's own algorithm, not
    cv.detail.BundleAdjusterReproj.  tests/numpy_reproj.py is that contract; DESIGN.md section 19."""

    MAX_CAMERAS, MAX_MATCHES = _lib.RAY_MAX_CAMERAS, _lib.RAY_MAX_MATCHES

    def __init__(self, conf_thresh=1.0, wave_correct=_UNSET, max_evals=100, model="rotation", refinement_mask=FULL_MASK):
        if model not in MODELS:
            raise StitchingError(f"unknown camera model {model!r}: the solver takes {MODELS}")
        self.model = model
        self.refinement_mask = self._check_mask(refinement_mask)
        if wave_correct is _UNSET:
            wave_correct = "no" if model == "affine" else "horiz"
        elif model == "affine" and wave_correct in ("horiz", "vert"):
            raise StitchingError(f'the affine camera model has no wave correction: "no" only, got {wave_correct!r}')
        if wave_correct == "auto":
            raise StitchingError('wave correction "auto" is cv2\'s: the solver takes "horiz", "vert" or "no"')
        if wave_correct not in WAVE_KINDS:
            raise StitchingError(f"unknown wave correction {wave_correct!r}: the solver takes {WAVE_KINDS}")
        if int(max_evals) < 1:
            raise StitchingError(f"camera adjustment needs at least one evaluation, got max_evals={max_evals}")
        self.conf_thresh, self.wave_correct, self.max_evals = float(conf_thresh), wave_correct, int(max_evals)
        self.info = None  # of the last adjust / register / normal_equations

    # -- subset
    def subset(self, features, matches):
        n = len(features)
        keep = largest_component(confidences(matches, n), self.conf_thresh)
        if len(keep) < 2:
            raise StitchingError(NO_MATCH_MESSAGE)
        if len(keep) < n:
            warnings.warn(NOT_ALL_MESSAGE, StitchingWarning)
        return keep

    @staticmethod
    def subset_matches(matches, indices):
        """the entries of the kept images, row-major"""
        n = int(math.sqrt(len(matches)))
        grid = np.empty((n, n), object)
        for k, e in enumerate(matches):
            grid[k // n, k % n] = e
        return list(grid[np.ix_(indices, indices)].reshape(-1))

    # -- estimate
    def estimate(self, features, matches):
        features = list(features)
        n = len(features)
        self._check_count(n)
        if self.model == "affine":
            return [self._affine_camera(T) for T in tree_transforms(matches, n)]
        focal = starting_focal(features, matches)
        return [self._camera(f, focal, R) for f, R in zip(features, tree_rotations(matches, n, [focal] * n))]

    @staticmethod
    def _camera(feature, focal, R):
        w0, h0 = feature.img_size
        return CameraParams(focal=focal, aspect=1.0, ppx=w0 / 2, ppy=h0 / 2, R=np.asarray(R).astype(np.float32))

    @staticmethod
    def _affine_camera(T):
        return CameraParams(focal=1.0, aspect=1.0, ppx=0.0, ppy=0.0, R=np.asarray(T).astype(np.float32))

    def _variants(self, params):
        return {"affine": similarity_variants, "reproj": reproj_variants}.get(self.model, camera_variants)(params)

    @property
    def _width(self):
        """parameters per camera"""
        return 7 if self.model == "reproj" else 4

    def _check_mask(self, mask):
        """the mask, where this model has a counterpart for it"""
        if self.model != "reproj":
            if mask != FULL_MASK:
                raise StitchingError(f'the {self.model} camera model moves all of its parameters: refinement mask "xxxxx" only, got {mask!r} '
                                     '(model="reproj" holds focal, principal point or aspect)')
            return mask
        free_parameters(mask)
        return mask

    def _check_count(self, n):
        if n > self.MAX_CAMERAS:
            raise StitchingError(f"camera registration of {n} images: the solver takes up to {self.MAX_CAMERAS}")

    # -- adjust
    def _sums(self, problem, evaluate, params):
        """(e, 45) sums at params, or None where a variant is not finite (a rejected step, not evaluated) — the device's, or evaluate's"""
        variants = self._variants(params)
        if not np.isfinite(variants).all():
            return None
        if evaluate is None:
            return problem.evaluate(variants)
        E, g, B = evaluate(params, variants)
        w = self._width
        return np.concatenate([np.asarray(E).reshape(-1, 1), np.asarray(g).reshape(-1, 2 * w), np.asarray(B).reshape(-1, w * (2 * w + 1))], axis=1)

    def _check_params(self, params, n):
        params = np.array(params, np.float64).reshape(-1, self._width)
        if len(params) != n:
            raise StitchingError(f"{len(params)} parameter rows for {n} cameras")
        if not np.isfinite(params).all():
            what = {"affine": "a, b, tx, ty", "reproj": "focal, principal point, aspect and Rodrigues vector"}.get(self.model, "focal and Rodrigues vector")
            raise StitchingError(f"camera adjustment needs finite parameters ({what} per camera)")
        return params

    def _problem(self, features, matches, conf_thresh=None):
        n = len(features)
        self._check_count(n)
        edges = ray_edges(matches, n, self.conf_thresh if conf_thresh is None else float(conf_thresh))
        offsets, xyuv = edge_points(features, matches, edges, [level0_points(f) for f in features] if self.model == "affine" else None)
        counts = np.diff(offsets)
        if len(counts) and int(counts.max()) > self.MAX_MATCHES:
            raise StitchingError(f"a pair with {int(counts.max())} inlier matches: the solver takes up to {self.MAX_MATCHES}")
        return edges, offsets, xyuv

    def normal_equations(self, features, matches, params, ctx=None):
        """E (e,), g (e, 8) and the upper triangle B (e, 36) of the normal equations of every edge (the pairs i < j with confidence above
        conf_thresh, ascending) at params (n, 4) rows focal, rx, ry, rz (model "affine": a, b, tx, ty) — one launch on the device.  Model
        "reproj": params (n, 7) rows focal, cx, cy, aspect, rx, ry, rz (cx, cy relative to the image centre) -> E (e,), g (e, 14), B (e, 105)."""
        features = list(features)
        params = self._check_params(params, len(features))
        edges, offsets, xyuv = self._problem(features, matches)
        with RayProblem(edges, offsets, xyuv, ctx, self.model) as problem:
            sums = problem.evaluate(self._variants(params))
            self.info = dict(problem.info, evaluations=1)
        w = 2 * self._width
        return sums[:, 0].copy(), sums[:, 1:1 + w].copy(), sums[:, 1 + w:].copy()

    def adjust(self, features, matches, cameras, ctx=None, conf_thresh=None, evaluate=None, refinement_mask=None):
        """conf_thresh: in place of the solver's own, for this call; refinement_mask alike (model "reproj").  evaluate(params, variants) -> (E, g, B) per edge: takes the device's place
        (measurements and tests of the host steps); everything else, the rejection of steps to variants that are not finite included,
        is as with the device."""
        features, cameras = list(features), list(cameras)
        n = len(features)
        if len(cameras) != n:
            raise StitchingError(f"{len(cameras)} cameras for {n} images")
        mask = self.refinement_mask if refinement_mask is None else self._check_mask(refinement_mask)
        free = None
        if self.model == "affine":
            start = self._check_params([similarity_parameters(c.R) for c in cameras], n)
        elif self.model == "reproj":
            sizes = [f.img_size for f in features]
            start = self._check_params([[c.focal, c.ppx - w0 / 2, c.ppy - h0 / 2, c.aspect] + list(rotation_vector(c.R))
                                        for c, (w0, h0) in zip(cameras, sizes)], n)
            if mask != FULL_MASK:
                free = np.array([7 * c + k for c in range(n) for k in free_parameters(mask)])
        else:
            start = self._check_params([[c.focal] + list(rotation_vector(c.R)) for c in cameras], n)
        edges, offsets, xyuv = self._problem(features, matches, conf_thresh)
        if evaluate is not None:
            params, info = self._levenberg_marquardt(None, evaluate, edges, start, free)
        else:
            with RayProblem(edges, offsets, xyuv, ctx, self.model) as problem:
                params, info = self._levenberg_marquardt(problem, None, edges, start, free)
        info["edges"], info["matches"] = len(edges), int(offsets[-1])
        if self.model == "reproj":
            info["refinement_mask"], info["start"] = mask, start
        self.info = info
        if self.model == "affine":
            failed = ((params[:, 0] == 0) & (params[:, 1] == 0)).any()
        else:
            failed = (params[:, 0] <= 0).any() or (self.model == "reproj" and (params[:, 3] <= 0).any())
        if not np.isfinite(params).all() or failed:
            raise StitchingError("Camera parameters adjusting failed.")
        _, centre = spanning_tree(matches, n)
        if centre < 0:
            raise StitchingError("Camera parameters adjusting failed.")
        if self.model == "affine":
            Ts = [similarity_matrix(p) for p in params]
            back = np.linalg.inv(Ts[centre])
            return [self._affine_camera(back @ T) for T in Ts]
        if self.model == "reproj":
            Rs = [rotation_matrix(p[4:7]) for p in params]
            back = np.linalg.inv(Rs[centre])
            out = []
            for (w0, h0), p, R in zip(sizes, params, Rs):
                out.append(CameraParams(focal=float(p[0]), aspect=float(p[3]), ppx=w0 / 2 + float(p[1]), ppy=h0 / 2 + float(p[2]),
                                        R=(back @ R).astype(np.float32)))
            return out
        Rs = [rotation_matrix(p[1:4]) for p in params]
        back = np.linalg.inv(Rs[centre])
        return [self._camera(f, float(p[0]), back @ R) for f, p, R in zip(features, params, Rs)]

    def _levenberg_marquardt(self, problem, evaluate_sums, edges, p, free=None):
        """free: the indices of the flat parameter vector that move (None: all of them); the rows and columns of the others are taken
        out of the system, and they are never written"""
        n, width = len(p), self._width
        info = {"evaluations": 1, "accepted": 0, "device_ms": 0.0, "device_ms_with_copy": 0.0}

        def evaluate(q):
            sums = self._sums(problem, evaluate_sums, q)
            if sums is None:
                return None
            if problem is not None:
                info["device_ms"] += problem.info["device_ms"]
                info["device_ms_with_copy"] += problem.info["device_ms_with_copy"]
            return assemble_system(n, edges, sums, width)

        with np.errstate(all="ignore"):
            first = evaluate(p)
            if first is None:
                raise StitchingError("Camera parameters adjusting failed.")
            E, g, A = first
            info["first_E"] = float(E)
            lam = 1e-3
            while info["evaluations"] < self.max_evals:
                better = False
                Af, gf = (A, g) if free is None else (A[np.ix_(free, free)], g[free])
                try:
                    step = np.linalg.solve(Af + lam * np.diag(np.diag(Af)), -gf)
                except np.linalg.LinAlgError:
                    step = None
                if step is not None:
                    if free is None:
                        q = p + step.reshape(n, width)
                    else:
                        q = p.copy()
                        q.reshape(-1)[free] = p.reshape(-1)[free] + step
                    moved = evaluate(q)
                    if moved is not None:
                        E2, g2, A2 = moved
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
        return p, info

    # -- wave correction
    def correct(self, cameras, kind=None):
        """kind: in place of the solver's own wave_correct, for this call ("horiz", "vert" or "no")"""
        kind = self.wave_correct if kind is None else kind
        if kind not in WAVE_KINDS:
            raise StitchingError(f"unknown wave correction {kind!r}: the solver takes {WAVE_KINDS}")
        cameras = list(cameras)
        if self.model == "affine":
            if kind != "no":
                raise StitchingError(f'the affine camera model has no wave correction: "no" only, got {kind!r}')
            return cameras
        out = []
        for cam, R in zip(cameras, wave_corrected([c.R for c in cameras], kind)):
            out.append(CameraParams(focal=cam.focal, aspect=cam.aspect, ppx=cam.ppx, ppy=cam.ppy, R=R, t=cam.t))
        return out

    # -- all of it
    def register(self, features, matches, ctx=None, evaluate=None):
        """-> (indices of the images kept, their cameras): subset, estimate, adjust, correct.  evaluate: as adjust's, over the edges of
        the images kept."""
        features = list(features)
        self._check_count(len(features))
        indices = self.subset(features, matches)
        features = [features[i] for i in indices]
        matches = self.subset_matches(matches, indices)
        cameras = self.adjust(features, matches, self.estimate(features, matches), ctx, evaluate=evaluate)
        return indices, self.correct(cameras)
