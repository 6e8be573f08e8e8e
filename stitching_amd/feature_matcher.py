"""FeatureMatcher with the reference's surface (stitching/feature_matcher.py:7-90).

Without `estimator=` it is the reference's class: the name picks cv.detail's BestOf2Nearest / BestOf2NearestRange / AffineBestOf2Nearest
matcher — OpenCV's, on the host.  With `estimator=MatchEstimator()` the features go to the device matcher.  That matcher is the
project's own and answers to no name here: "homography" stays cv2's, and "affine" goes with an estimator only where that estimator's own
`model` is an affine one (MatchEstimator(model="affine")).  The numpy helpers need no cv2; the drawing helpers do.
"""
import math

import numpy as np

from .stitching_error import StitchingError


def _cv():
    try:
        import cv2 as cv
    except ImportError as e:
        raise StitchingError("feature matching by name and the drawing helpers need OpenCV, which is not importable here: pass "
                             "estimator=stitching_amd.MatchEstimator() for the device matcher") from e
    return cv


class FeatureMatcher:
    """https://docs.opencv.org/4.x/da/d87/classcv_1_1detail_1_1FeaturesMatcher.html"""

    MATCHER_CHOICES = ("homography", "affine")
    DEFAULT_MATCHER = "homography"
    DEFAULT_RANGE_WIDTH = -1

    def __init__(self, matcher_type=DEFAULT_MATCHER, range_width=DEFAULT_RANGE_WIDTH, estimator=None, **kwargs):
        """`estimator`: any object with match(features) -> n * n match objects, row-major (a MatchEstimator, which carries its own
        range_width and match_conf); the name is then looked at only to refuse "affine" with an estimator whose `model` is not an affine
        one.  Default: the cv2 matcher the reference builds for the name."""
        self.estimator = estimator
        self.matcher = None
        if estimator is not None:
            if matcher_type == "affine" and not str(getattr(estimator, "model", "homography")).startswith("affine"):
                raise StitchingError('the "affine" matcher has no device estimator: only a homography is fitted there')
            if kwargs:
                raise StitchingError(f"a match estimator takes its settings at construction, got {sorted(kwargs)}")
            return
        cv = _cv()
        if matcher_type == "affine":
            self.matcher = cv.detail_AffineBestOf2NearestMatcher(**kwargs)
        elif range_width == -1:
            self.matcher = cv.detail_BestOf2NearestMatcher(**kwargs)
        else:
            self.matcher = cv.detail_BestOf2NearestRangeMatcher(range_width, **kwargs)

    def match_features(self, features, *args, **kwargs):
        if self.estimator is not None:
            if args or kwargs:
                raise StitchingError("a match estimator takes the list of features alone")
            return self.estimator.match(features)
        pairwise_matches = self.matcher.apply2(features, *args, **kwargs)
        self.matcher.collectGarbage()
        return pairwise_matches

    @staticmethod
    def draw_matches_matrix(imgs, features, matches, conf_thresh=1, inliers=False, **kwargs):
        matches_matrix = FeatureMatcher.get_matches_matrix(matches)
        for idx1, idx2 in FeatureMatcher.get_all_img_combinations(len(imgs)):
            match = matches_matrix[idx1, idx2]
            if match.confidence < conf_thresh or len(match.matches) == 0:
                continue
            if inliers:
                kwargs["matchesMask"] = match.getInliers()
            yield idx1, idx2, FeatureMatcher.draw_matches(imgs[idx1], features[idx1], imgs[idx2], features[idx2], match, **kwargs)

    @staticmethod
    def draw_matches(img1, features1, img2, features2, match1to2, **kwargs):
        cv = _cv()
        kwargs.setdefault("flags", cv.DrawMatchesFlags_NOT_DRAW_SINGLE_POINTS)
        return cv.drawMatches(img1, features1.getKeypoints(), img2, features2.getKeypoints(), match1to2.getMatches(), None, **kwargs)

    @staticmethod
    def get_matches_matrix(pairwise_matches):
        return FeatureMatcher.array_in_square_matrix(pairwise_matches)

    @staticmethod
    def get_confidence_matrix(pairwise_matches):
        matches_matrix = FeatureMatcher.get_matches_matrix(pairwise_matches)
        return np.array([[m.confidence for m in row] for row in matches_matrix])

    @staticmethod
    def array_in_square_matrix(array):
        """The n * n list as an (n, n) array of its objects, row-major."""
        n = int(math.sqrt(len(array)))
        return np.array([list(array[r * n:(r + 1) * n]) for r in range(n)])

    @staticmethod
    def get_all_img_combinations(number_imgs):
        ii, jj = np.triu_indices(number_imgs, k=1)
        for i, j in zip(ii, jj):
            yield i, j

    @staticmethod
    def get_match_conf(match_conf, feature_detector_type):
        if match_conf is None:
            match_conf = FeatureMatcher.get_default_match_conf(feature_detector_type)
        return match_conf

    @staticmethod
    def get_default_match_conf(feature_detector_type):
        if feature_detector_type == "orb":
            return 0.3
        return 0.65
