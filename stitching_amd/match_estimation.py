"""Feature matching on the device: two-nearest-neighbour descriptor matching and a homography RANSAC.

`MatchEstimator` is the project's OWN matcher.  It is NOT cv.detail.BestOf2NearestMatcher and does not answer to "homography" or
"affine": those names stay cv2's (feature_matcher.FeatureMatcher).  The quadratic work — Hamming distances of all descriptor pairs of all
image pairs, hypotheses times matches — runs on the device (csrc/stx_matches.hip) and equals its contract, tests/numpy_matches.py, in
every integer array and in the float64 bits of the winning sample homography; DESIGN.md section 16 has the kernels and the limits.

What is small and needs float64 with a library behind it is computed here on the host, as the exposure solver does for its small
system: the integer ratio threshold, the centred level-0 coordinates, the refit of the winning hypothesis over its inliers (Hartley
normalised DLT, SVD), the confidence and the mirrored entries.

With model="affine" the RANSAC fits a similarity (2 matches a sample) or, with full_affine=True, an affine map (3) on points that are not
centred — the registration of scans and flat tiles, whose cameras the affine warper applies to raw pixels.  Everything but the hypothesis
and the refit is shared with the homography; tests/numpy_affine.py is that contract and DESIGN.md section 18 the description.
"""
import math

import numpy as np

from . import _lib
from ._marshal import handles, info_dict, ptr
from .device import get_context
from .stitching_error import StitchingError

MIN_MATCHES = 6  # RANSAC runs on pairs with at least this many matches; a homography is kept with at least this many inliers
# and a refit that is finite and has a finite inverse


def ratio_threshold(match_conf):
    """T of the integer ratio test 1024 d1 < T d2: floor((1 - match_conf) 1024 + 0.5) in float64"""
    return int(math.floor((1.0 - float(match_conf)) * 1024.0 + 0.5))


def centred_points(features):
    """(n, 2) float64: the keypoints of one ImageFeatures in level-0 pixels relative to the image centre, as OpenCV centres them:
    x0 = (x + 0.5) * w0 / wl - 0.5 - w0 * 0.5 in this order of operations, y alike."""
    n = len(features.level)
    out = np.zeros((n, 2), np.float64)
    if n == 0:
        return out
    w0, h0 = features.img_size
    sizes = np.asarray(features.level_sizes, np.float64).reshape(-1, 2)[np.asarray(features.level, np.int64)]
    out[:, 0] = (np.asarray(features.x, np.float64) + 0.5) * float(w0) / sizes[:, 0] - 0.5 - float(w0) * 0.5
    out[:, 1] = (np.asarray(features.y, np.float64) + 0.5) * float(h0) / sizes[:, 1] - 0.5 - float(h0) * 0.5
    return out


def level0_points(features):
    """(n, 2) float64: the keypoints of one ImageFeatures in level-0 pixels, not centred (the affine models' frame):
    x0 = (x + 0.5) * w0 / wl - 0.5 in this order of operations, y alike."""
    n = len(features.level)
    out = np.zeros((n, 2), np.float64)
    if n == 0:
        return out
    w0, h0 = features.img_size
    sizes = np.asarray(features.level_sizes, np.float64).reshape(-1, 2)[np.asarray(features.level, np.int64)]
    out[:, 0] = (np.asarray(features.x, np.float64) + 0.5) * float(w0) / sizes[:, 0] - 0.5
    out[:, 1] = (np.asarray(features.y, np.float64) + 0.5) * float(h0) / sizes[:, 1] - 0.5
    return out


def _hartley(p):
    c = p.mean(axis=0)
    d = np.sqrt(((p - c) ** 2).sum(axis=1)).mean()
    s = math.sqrt(2.0) / d if d > 0 else 1.0
    return np.array([[s, 0.0, -s * c[0]], [0.0, s, -s * c[1]], [0.0, 0.0, 1.0]]), (p - c) * s


def refit_homography(src, dst):
    """(3, 3) float64 with h22 = 1: the Hartley-normalised direct linear transform of k >= 4 correspondences src -> dst ((k, 2) each),
    the right singular vector of the smallest singular value."""
    ts, s = _hartley(np.asarray(src, np.float64))
    td, d = _hartley(np.asarray(dst, np.float64))
    a = np.zeros((2 * len(s), 9), np.float64)
    a[0::2, 0:2], a[0::2, 2] = -s, -1.0
    a[0::2, 6:8], a[0::2, 8] = d[:, 0:1] * s, d[:, 0]
    a[1::2, 3:5], a[1::2, 5] = -s, -1.0
    a[1::2, 6:8], a[1::2, 8] = d[:, 1:2] * s, d[:, 1]
    h = np.linalg.svd(a)[2][-1].reshape(3, 3)
    h = np.linalg.inv(td) @ h @ ts
    return h / h[2, 2]


def refit_affine(src, dst, full=False):
    """(3, 3) float64 with the last row 0, 0, 1: the least-squares similarity (full=False: closed form about the two centroids) or
    affine map (full=True: lstsq on the centred points) of k correspondences src -> dst ((k, 2) each)."""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    cp, cq = src.mean(axis=0), dst.mean(axis=0)
    if full:
        sol = np.linalg.lstsq(np.concatenate([src - cp, np.ones((len(src), 1))], axis=1), dst - cq, rcond=None)[0]
        linear, cq = sol[0:2].T, cq + sol[2]
    else:
        dx, dy = (src - cp).T
        du, dv = (dst - cq).T
        d = (dx * dx + dy * dy).sum()
        a, b = (dx * du + dy * dv).sum() / d, (dx * dv - dy * du).sum() / d
        linear = np.array([[a, -b], [b, a]])
    t = cq - linear @ cp
    return np.array([[linear[0, 0], linear[0, 1], t[0]], [linear[1, 0], linear[1, 1], t[1]], [0.0, 0.0, 1.0]])


def finite_inverse(h):
    """The inverse of a refitted H, or None where H is not finite or has no finite inverse (many matches onto a few points): such a
    pair has no homography."""
    if not np.isfinite(h).all():
        return None
    try:
        inv = np.linalg.inv(h)
    except np.linalg.LinAlgError:
        return None
    return inv if np.isfinite(inv).all() else None


def match_confidence(num_inliers, num_matches):
    """num_inliers / (8 + 0.3 m); above 3 the images are taken for near-identical and the confidence is 0 (OpenCV's rule)"""
    c = num_inliers / (8 + 0.3 * num_matches)
    return 0.0 if c > 3 else c


class DMatch:
    """What cv.DMatch carries, for callers that draw."""

    __slots__ = ("queryIdx", "trainIdx", "imgIdx", "distance")

    def __init__(self, query, train, distance):
        self.queryIdx, self.trainIdx, self.imgIdx, self.distance = query, train, -1, float(distance)

    def __repr__(self):
        return f"DMatch(queryIdx={self.queryIdx}, trainIdx={self.trainIdx}, distance={self.distance})"


class MatchesInfo:
    """One entry of the n x n match matrix, with the fields of cv.detail.MatchesInfo (src_img_idx, dst_img_idx, getMatches(),
    getInliers(), num_inliers, H, confidence) and the raw arrays of the contract: matches (m, 3) int32 rows query, train, distance;
    inliers_mask (m,) u8.  H_sample is the winning hypothesis as the device computed it (9 float64) and hypothesis its number k, on the
    entries i < j that RANSAC ran on (None and -1 elsewhere)."""

    def __init__(self, src_img_idx=-1, dst_img_idx=-1, matches=None, inliers_mask=None, num_inliers=0, H=None, confidence=0.0,
                 H_sample=None, hypothesis=-1):
        self.src_img_idx, self.dst_img_idx = int(src_img_idx), int(dst_img_idx)
        self.matches = np.zeros((0, 3), np.int32) if matches is None else matches
        self.inliers_mask = np.zeros(len(self.matches), np.uint8) if inliers_mask is None else inliers_mask
        self.num_inliers, self.H, self.confidence = int(num_inliers), H, float(confidence)
        self.H_sample, self.hypothesis = H_sample, int(hypothesis)

    def getMatches(self):
        return [DMatch(q, t, d) for q, t, d in self.matches.tolist()]

    def getInliers(self):
        return self.inliers_mask

    def mirrored(self):
        """The entry (j, i) of this entry (i, j): query and train swapped, H inverted."""
        return MatchesInfo(self.dst_img_idx, self.src_img_idx, np.ascontiguousarray(self.matches[:, [1, 0, 2]]), self.inliers_mask.copy(),
                           self.num_inliers, None if self.H is None else np.linalg.inv(self.H), self.confidence)


class MatchEstimator:
    """The project's own descriptor matcher and homography RANSAC on the device — NOT cv.detail.BestOf2NearestMatcher, and not behind
    the names "homography" / "affine" (those stay cv2's).  For every image pair: the two nearest descriptors by Hamming distance with an
    integer ratio test, the union of both directions in OpenCV's order, `ransac_iters` homographies of 4 matches drawn by a counter-based
    generator (division-free closed form, IEEE fp64 without FMA), the hypothesis with the most inliers; then on the host the refit over
    its inliers and the confidence.  tests/numpy_matches.py states it exactly and is the contract; DESIGN.md section 16 has the launch
    shapes.  Construction needs no GPU.

    Plug it in where a matcher goes: FeatureMatcher(estimator=MatchEstimator()).

    model: "homography" (the default), or "affine" for scans and flat tiles — a similarity of 2 matches ("affine_partial", as OpenCV's
    full_affine=False default), or with full_affine=True an affine map of 3 ("affine_full"); `model` reads back the resolved name.  The
    affine models work on points that are not centred and refit by least squares; tests/numpy_affine.py is their contract
    (FeatureMatcher("affine", estimator=MatchEstimator(model="affine"))).

    Limits, refused with a StitchingError before anything is launched: at most MAX_FEATURES features in an image, ransac_iters in
    1 .. MAX_ITERS, descriptors of shape (n, 32) u8, as many keypoints as descriptors."""

    MAX_FEATURES, MAX_ITERS = _lib.MATCH_MAX_FEATURES, _lib.MATCH_MAX_ITERS

    def __init__(self, match_conf=0.3, range_width=-1, ransac_iters=500, ransac_threshold=3.0, seed=0x5EED, model="homography",
                 full_affine=False):
        if model not in ("homography", "affine"):
            raise StitchingError(f'unknown match model {model!r}: "homography", or "affine" (a similarity; with full_affine=True an affine map)')
        self.model = model if model == "homography" else "affine_full" if full_affine else "affine_partial"
        if not 0.0 <= float(match_conf) <= 1.0:
            raise StitchingError(f"feature matching needs a match_conf in 0 .. 1, got {match_conf}")
        if not 0.0 <= float(ransac_threshold) <= 1e6:
            raise StitchingError(f"feature matching needs a RANSAC threshold in 0 .. 1e6 pixels, got {ransac_threshold}")
        self.match_conf, self.range_width, self.ransac_iters = float(match_conf), int(range_width), int(ransac_iters)
        self.ransac_threshold, self.seed = float(ransac_threshold), int(seed) & 0xFFFFFFFF
        self.info = None  # of the last call: pairs, matches, device ms of the launches, device ms with the copies

    def match(self, features, ctx=None):
        """n * n MatchesInfo, row-major as cv.detail.FeaturesMatcher.apply2 returns them, for the list of ImageFeatures that
        FeatureEstimator.detect returns.  Nothing handed in is written."""
        features = list(features)
        n = len(features)
        out = [MatchesInfo() for _ in range(n * n)]
        self.info = {"pairs": 0, "matches": 0, "device_ms": 0.0, "device_ms_with_copy": 0.0}
        if n == 0:
            return out
        desc, pts, shape, rows = [], [], np.zeros((n, 3), np.int32), np.zeros(n, np.int32)
        for i, f in enumerate(features):
            d = np.ascontiguousarray(f.descriptors)
            if d.ndim != 2:
                raise StitchingError(f"image {i}: descriptors of shape {d.shape}: feature matching needs n x 32 u8")
            p = np.ascontiguousarray(centred_points(f) if self.model == "homography" else level0_points(f))
            shape[i] = (d.shape[0], d.shape[1], d.dtype.itemsize)
            rows[i] = len(p)
            desc.append(d)
            pts.append(p)
        pairs = [(i, j) for i in range(n) for j in range(i + 1, n) if self.range_width < 0 or j - i <= self.range_width]
        cap = sum(int(rows[i]) + int(rows[j]) for i, j in pairs)
        counts, pick, Hs = np.zeros(len(pairs), np.int32), np.zeros((len(pairs), 2), np.int32), np.zeros((len(pairs), 9), np.float64)
        matches, mask = np.zeros((max(cap, 1), 3), np.int32), np.zeros(max(cap, 1), np.uint8)
        info = np.zeros(4, np.float64)
        ctx = ctx or get_context()
        # host addresses: the descriptors may be of any dtype (the library refuses what is not u8), so not ptr()
        da, pa = handles([d.ctypes.data for d in desc]), handles([p.ctypes.data for p in pts])
        t = self.ransac_threshold
        front = (ctx.handle, n, da, ptr(shape), pa, ptr(rows), ratio_threshold(self.match_conf), self.range_width, self.ransac_iters, t * t,
                 self.seed)
        back = (ptr(counts), ptr(matches), ptr(mask), ptr(pick), ptr(Hs), ptr(info))
        if self.model == "homography":
            _lib.check(ctx._lib.stx_match_features(*front, *back))
        else:
            _lib.check(ctx._lib.stx_match_features_model(*front, _lib.MATCH_MODELS[self.model], *back))
        self.info = info_dict(info, [("pairs", int), ("matches", int), ("device_ms", float), ("device_ms_with_copy", float)])
        slot = 0
        for k, (i, j) in enumerate(pairs):
            m = int(counts[k])
            e = MatchesInfo(i, j, matches[slot:slot + m].copy(), np.zeros(m, np.uint8))
            if m >= MIN_MATCHES:
                e.H_sample, e.hypothesis = Hs[k].copy(), int(pick[k, 1])
                if int(pick[k, 0]) >= MIN_MATCHES:
                    keep = mask[slot:slot + m] != 0
                    with np.errstate(all="ignore"):
                        src, dst = pts[i][e.matches[keep, 0]], pts[j][e.matches[keep, 1]]
                        h = refit_homography(src, dst) if self.model == "homography" else refit_affine(src, dst, self.model == "affine_full")
                    if finite_inverse(h) is not None:
                        e.inliers_mask, e.num_inliers, e.H = mask[slot:slot + m].copy(), int(pick[k, 0]), h
                        e.confidence = match_confidence(e.num_inliers, m)
            out[i * n + j], out[j * n + i] = e, e.mirrored()
            slot += int(rows[i]) + int(rows[j])
        return out
