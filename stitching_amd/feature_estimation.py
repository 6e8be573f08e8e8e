"""Feature detection on the device: corner keypoints and 256-bit binary descriptors.

`FeatureEstimator` is the project's OWN detector, in the family of oriented FAST + rotated BRIEF.  It is NOT cv.ORB (no Harris score in
floating point, no 8-bit orientation, no learned pattern) and does not answer to "orb" or "sift": those names stay cv2's
(feature_detector.FeatureDetector).  It is integer only, so that the device equals its contract, tests/numpy_features.py, byte for
byte; DESIGN.md section 15 has the kernels (csrc/stx_features.hip) and the limits.

What depends on floating point is computed here, once, in float64 and handed to the device as integers: the level sizes, the quotas of
the levels, the direction tables CX / CY and the 36 rotated comparison patterns.
"""
import functools
import math

import numpy as np

from . import _lib
from ._marshal import handles, info_dict, one_context, ptr
from .device import as_device
from .stitching_error import StitchingError

BINS = 36            # orientation bins of 10 degrees
PAIRS = 256          # comparisons: 32 descriptor bytes
PATTERN_RADIUS = 13  # every pattern point lies in this disc: a rotated point stays within +-13, inside the keypoint border of 16
MIN_LEVEL_SIDE = 33  # a level narrower or lower than this is dropped with every level after it: no pixel has its 31 x 31 patch inside
PATTERN_SEED = 0x5EED


@functools.lru_cache(maxsize=None)
def pattern():
    """The base comparison pattern: (256, 4) int8 rows px, py, qx, qy.  A seeded recipe, data rather than code to the contract: pairs of
    rounded Gaussian points (sigma = radius / 2.5, as BRIEF draws its pairs densest near the centre) from numpy's legacy generator
    (whose stream is frozen), kept when both lie in the disc of PATTERN_RADIUS and differ."""
    rs = np.random.RandomState(PATTERN_SEED)
    rows = []
    while len(rows) < PAIRS:
        px, py, qx, qy = (int(v) for v in np.rint(rs.normal(0.0, PATTERN_RADIUS / 2.5, 4)))
        if px * px + py * py > PATTERN_RADIUS ** 2 or qx * qx + qy * qy > PATTERN_RADIUS ** 2 or (px, py) == (qx, qy):
            continue
        rows.append((px, py, qx, qy))
    out = np.array(rows, np.int8)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def rotated_patterns():
    """(36, 256, 4) int8: the pattern turned by 10 b degrees, P_b = (rint(px cos - py sin), rint(px sin + py cos)) in float64."""
    base = pattern().astype(np.float64)
    out = np.zeros((BINS, PAIRS, 4), np.int8)
    for b in range(BINS):
        th = 2.0 * math.pi * b / BINS
        c, s = math.cos(th), math.sin(th)
        for k in (0, 2):
            out[b, :, k] = np.rint(base[:, k] * c - base[:, k + 1] * s)
            out[b, :, k + 1] = np.rint(base[:, k] * s + base[:, k + 1] * c)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def direction_tables():
    """(72,) int32: CX[b] = rint(16384 cos(2 pi b / 36)) for the 36 bins, then CY[b] with the sine."""
    th = 2.0 * math.pi * np.arange(BINS, dtype=np.float64) / BINS
    out = np.concatenate([np.rint(16384.0 * np.cos(th)), np.rint(16384.0 * np.sin(th))]).astype(np.int32)
    out.setflags(write=False)
    return out


def level_sizes(w0, h0, nlevels, scale):
    """[(w, h)] of the levels kept: level l is (floor(w0 / scale**l + 0.5), floor(h0 / scale**l + 0.5)) in float64; the first level with
    a side below MIN_LEVEL_SIDE ends the list."""
    out = []
    for l in range(int(nlevels)):
        f = float(scale) ** l
        w, h = int(math.floor(w0 / f + 0.5)), int(math.floor(h0 / f + 0.5))
        if w < MIN_LEVEL_SIDE or h < MIN_LEVEL_SIDE:
            break
        out.append((w, h))
    return out


def level_quotas(nfeatures, scale, levels):
    """Keypoints per level for `levels` kept levels, in float64: a geometric series with ratio 1 / scale, each term rounded half up, the
    last level taking what is left of nfeatures (never less than 0).  The rounded terms alone can exceed nfeatures by a few (7 features over
    8 levels at scale 1.2), so each is also capped by what the levels before it left: the sum never exceeds nfeatures."""
    if levels == 0:
        return []
    q = 1.0 / float(scale)
    d = nfeatures * (1.0 - q) / (1.0 - q ** levels)
    out, total = [], 0
    for _ in range(levels - 1):
        out.append(min(int(math.floor(d + 0.5)), int(nfeatures) - total))
        total += out[-1]
        d *= q
    out.append(max(int(nfeatures) - total, 0))
    return out


class KeyPoint:
    """What cv.KeyPoint carries, for callers that draw or match: pt in level-0 pixels, size, angle in degrees, response, octave."""

    __slots__ = ("pt", "size", "angle", "response", "octave", "class_id")

    def __init__(self, pt, size, angle, response, octave):
        self.pt, self.size, self.angle, self.response, self.octave, self.class_id = pt, size, angle, response, octave, -1

    def __repr__(self):
        return f"KeyPoint(pt={self.pt}, size={self.size}, angle={self.angle}, response={self.response}, octave={self.octave})"


class ImageFeatures:
    """The features of one image, with the fields of cv.detail.ImageFeatures (img_idx, img_size, getKeypoints(), descriptors) and the raw
    integer arrays of the contract: level, x, y, bin (int32), R (int64), descriptors (n, 32) u8; x, y are pixels of the level."""

    def __init__(self, img_idx, img_size, level_sizes, level, x, y, bin, R, descriptors):
        self.img_idx, self.img_size, self.level_sizes = int(img_idx), (int(img_size[0]), int(img_size[1])), list(level_sizes)
        self.level, self.x, self.y, self.bin, self.R, self.descriptors = level, x, y, bin, R, descriptors

    def __len__(self):
        return len(self.level)

    def getKeypoints(self):
        w0, h0 = self.img_size
        out = []
        for l, x, y, b, r in zip(self.level.tolist(), self.x.tolist(), self.y.tolist(), self.bin.tolist(), self.R.tolist()):
            wl, hl = self.level_sizes[l]
            out.append(KeyPoint(((x + 0.5) * w0 / wl - 0.5, (y + 0.5) * h0 / hl - 0.5), 31.0 * w0 / wl, 10.0 * b, float(r), l))
        return out


class FeatureEstimator:
    """The project's own corner detector and binary descriptor on the device — NOT cv.ORB, and not behind the names "orb" / "sift"
    (those stay cv2's).  Integer only: a grey pyramid (the exact linear resize), the 9-of-16 segment-test score with 3 x 3 suppression, an
    integer Harris-like response that ranks the corners of a level, orientation in 36 bins from the intensity centroid, 256 comparisons
    of a 5 x 5 binomial blur under the rotated pattern.  tests/numpy_features.py states it exactly and is the contract, byte for byte;
    DESIGN.md section 15 has the launch shapes.  Construction needs no GPU.

    Plug it in where a detector goes: FeatureDetector(estimator=FeatureEstimator()).

    Limits, refused with a StitchingError before anything is launched: image sides up to MAX_SIDE (response, y and x of a corner are one
    64-bit sort key), at most MAX_LEVELS levels and MAX_FEATURES features per image."""

    MAX_SIDE, MAX_LEVELS, MAX_FEATURES = _lib.FEATURES_MAX_SIDE, _lib.FEATURES_MAX_LEVELS, _lib.FEATURES_MAX_FEATURES

    def __init__(self, nfeatures=500, nlevels=8, scale=1.2, fast_threshold=20):
        if not float(scale) > 1.0:
            raise StitchingError(f"feature detection needs a pyramid scale above 1, got {scale}")
        self.nfeatures, self.nlevels, self.scale, self.fast_threshold = int(nfeatures), int(nlevels), float(scale), int(fast_threshold)
        self.info = None  # of the last call: levels, candidates, keypoints

    def detect(self, imgs, masks=None):
        """One ImageFeatures per u8 BGR image of `imgs` (numpy arrays, cv.UMat-likes or DeviceImages: those stay in HBM); `masks`: None,
        or per image None or a u8 mask of the image's size (nonzero: keypoints allowed).  Nothing handed in is written."""
        imgs = list(imgs)
        n = len(imgs)
        masks = [None] * n if masks is None else list(masks)
        if len(masks) != n:
            raise StitchingError("image and mask lists must be of same length")
        if n == 0:
            self.info = {"levels": 0, "candidates": 0, "keypoints": 0}
            return []
        ctx = one_context(imgs + masks)
        d_imgs = [as_device(a, ctx) for a in imgs]
        d_masks = [None if m is None else as_device(m, ctx) for m in masks]
        ML = self.MAX_LEVELS
        cap = max(1, min(self.nfeatures, self.MAX_FEATURES))
        counts, wh, quotas, sizes = np.zeros(n, np.int32), np.zeros((n, ML, 2), np.int32), np.zeros((n, ML), np.int32), []
        for i, a in enumerate(d_imgs):
            ls = level_sizes(a.width, a.height, min(self.nlevels, ML), self.scale)
            sizes.append(ls)
            counts[i] = len(ls)
            if ls:  # an image below MIN_LEVEL_SIDE has no level and no keypoint
                wh[i, :len(ls)] = ls
                quotas[i, :len(ls)] = level_quotas(self.nfeatures, self.scale, len(ls))
        found = np.zeros(n, np.int32)
        lxyb, R, desc = np.zeros((n, cap, 4), np.int32), np.zeros((n, cap), np.int64), np.zeros((n, cap, 32), np.uint8)
        info = np.zeros(4, np.float64)
        tables, pats = direction_tables(), rotated_patterns()
        _lib.check(ctx._lib.stx_features_detect(
            ctx.handle, n, handles(d_imgs), handles(d_masks), self.nfeatures, self.nlevels, self.fast_threshold, ptr(counts), ptr(wh),
            ptr(quotas), ptr(tables), ptr(pats), ptr(found), ptr(lxyb), ptr(R), ptr(desc), ptr(info)))
        self.info = info_dict(info, [("levels", int), ("candidates", int), ("keypoints", int)])
        out = []
        for i, a in enumerate(d_imgs):
            k = int(found[i])
            q = lxyb[i, :k]
            out.append(ImageFeatures(i, (a.width, a.height), sizes[i], q[:, 0].copy(), q[:, 1].copy(), q[:, 2].copy(), q[:, 3].copy(),
                                     R[i, :k].copy(), desc[i, :k].copy()))
        return out
