"""FeatureDetector with the reference's surface (stitching/feature_detector.py:9-46).

Without `estimator=` it is the reference's class: the name picks cv.ORB / cv.SIFT and the features come from
cv.detail.computeImageFeatures2 — OpenCV's, on the host.  With `estimator=FeatureEstimator()` the images go to the device detector
untouched (device images stay in HBM).  That detector is the project's own and answers to no name here: "orb" stays cv.ORB.
"""
from collections import OrderedDict

from .stitching_error import StitchingError


def _cv():
    try:
        import cv2 as cv
    except ImportError as e:
        raise StitchingError("feature detection by name needs OpenCV, which is not importable here: pass "
                             "estimator=stitching_amd.FeatureEstimator() for the device detector") from e
    return cv


def _orb(**kwargs):
    return _cv().ORB.create(**kwargs)


def _sift(**kwargs):
    return _cv().SIFT_create(**kwargs)


class FeatureDetector:
    """https://docs.opencv.org/4.x/d0/d13/classcv_1_1Feature2D.html"""

    DETECTOR_CHOICES = OrderedDict()
    DETECTOR_CHOICES["orb"] = _orb
    DETECTOR_CHOICES["sift"] = _sift

    DEFAULT_DETECTOR = list(DETECTOR_CHOICES.keys())[0]

    def __init__(self, detector=DEFAULT_DETECTOR, estimator=None, **kwargs):
        """`estimator`: any object with detect(imgs, masks=None) -> one features object per image (a FeatureEstimator); the name is
        then not looked at, as in SeamFinder.  Default: the cv2 detector the reference builds for the name."""
        self.estimator = estimator
        self.detector = None if estimator is not None else FeatureDetector.DETECTOR_CHOICES[detector](**kwargs)

    def detect_features(self, img, *args, **kwargs):
        if self.estimator is not None:
            mask = kwargs.pop("mask", args[0] if args else None)
            if len(args) > 1 or kwargs:
                raise StitchingError("a feature estimator takes an image and an optional mask")
            return self.estimator.detect([img], None if mask is None else [mask])[0]
        return _cv().detail.computeImageFeatures2(self.detector, img, *args, **kwargs)

    def detect(self, imgs):
        if self.estimator is not None:
            return self.estimator.detect(list(imgs))
        return [self.detect_features(img) for img in imgs]

    def detect_with_masks(self, imgs, masks):
        """The reference's two StitchingError messages (stitching/feature_detector.py:28-40), checked for the whole list before any image
        is looked at.  Two differences: the reference compares the lengths inside its loop over zip(imgs, masks), so it never raises when
        one of the lists is empty — here unequal lengths always raise; and a wrong number of dimensions is an AssertionError there, a
        StitchingError here."""
        imgs, masks = list(imgs), list(masks)
        if len(imgs) != len(masks):
            raise StitchingError("image and mask lists must be of same length")
        for number, (img, mask) in enumerate(zip(imgs, masks), start=1):
            if len(img.shape) != 3 or len(mask.shape) != 2:
                raise StitchingError(f"image {number} must have three dimensions and mask {number} two, got {img.shape} and {mask.shape}")
            if tuple(img.shape[:2]) != tuple(mask.shape):
                raise StitchingError(f"Resolution of mask {number} {mask.shape} does not match the resolution of image {number} {img.shape[:2]}.")
        if self.estimator is not None:
            return self.estimator.detect(imgs, masks)
        return [self.detect_features(img, mask=mask) for img, mask in zip(imgs, masks)]

    @staticmethod
    def draw_keypoints(img, features, **kwargs):
        cv = _cv()
        kwargs.setdefault("color", (0, 255, 0))
        keypoints = features.getKeypoints()
        return cv.drawKeypoints(img, keypoints, None, **kwargs)
