"""CameraEstimator with the reference's surface (stitching/camera_estimator.py:9-27).

Without `solver=` it is the reference's class: the name picks cv.detail's HomographyBasedEstimator or AffineBasedEstimator — OpenCV's, on
the host.  With `solver=CameraSolver()` the cameras come from the project's own solver.  That solver answers to no name here:
"homography" stays cv2's, and "affine" goes with a solver only where that solver's own `model` is "affine".
"""
import numpy as np

from .stitching_error import StitchingError


def _cv():
    try:
        import cv2 as cv
    except ImportError as e:
        raise StitchingError("camera estimation by name needs OpenCV, which is not importable here: pass "
                             "solver=stitching_amd.CameraSolver() for the project's own") from e
    return cv


class CameraEstimator:
    """https://docs.opencv.org/4.x/df/d15/classcv_1_1detail_1_1Estimator.html"""

    CAMERA_ESTIMATOR_CHOICES = ("homography", "affine")
    DEFAULT_CAMERA_ESTIMATOR = "homography"

    def __init__(self, estimator=DEFAULT_CAMERA_ESTIMATOR, solver=None, **kwargs):
        """`solver`: a CameraSolver (it carries its own settings); the name is then looked at only to refuse "affine" with a solver whose
        `model` is not "affine".  Default: the cv2 estimator the reference builds for the name."""
        self.solver = solver
        self.estimator = None
        if solver is not None:
            if estimator == "affine" and getattr(solver, "model", None) != "affine":
                raise StitchingError('the "affine" camera estimator has no counterpart in the solver: it estimates rotations and focals')
            if kwargs:
                raise StitchingError(f"a camera solver takes its settings at construction, got {sorted(kwargs)}")
            return
        cv = _cv()
        choices = {"homography": cv.detail_HomographyBasedEstimator, "affine": cv.detail_AffineBasedEstimator}
        self.estimator = choices[estimator](**kwargs)

    def estimate(self, features, pairwise_matches):
        if self.solver is not None:
            return self.solver.estimate(features, pairwise_matches)
        ok, estimated = self.estimator.apply(features, pairwise_matches, None)
        if not ok:
            raise StitchingError("Homography estimation failed.")
        for camera in estimated:  # OpenCV's adjusters want float32 rotations
            camera.R = np.asarray(camera.R, np.float32)
        return estimated
