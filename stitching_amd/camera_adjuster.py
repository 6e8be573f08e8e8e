"""CameraAdjuster with the reference's surface (stitching/camera_adjuster.py:9-50).

Without `solver=` it is the reference's class: the name picks cv.detail's BundleAdjusterRay / Reproj / AffinePartial / NoBundleAdjuster —
OpenCV's, on the host.  With `solver=CameraSolver()` the cameras are refined by the project's own ray adjustment on the device.  That
adjustment answers to no name here: "ray" stays cv2's; "affine" and "reproj" go with a solver only where that solver's own `model` is
"affine" or "reproj".  A refinement mask other than "xxxxx" goes with a solver of the model "reproj" alone, whose parameters include
the principal point and the aspect (CameraSolver(model="reproj"): the project's own reprojection adjustment, not
cv.detail.BundleAdjusterReproj); it is handed to the solver's adjust with every call.  The rotation and the affine solver move all of
their parameters and refuse any other mask.
"""
import numpy as np

from .camera_estimation import free_parameters
from .stitching_error import StitchingError


def _cv():
    try:
        import cv2 as cv
    except ImportError as e:
        raise StitchingError("camera adjustment by name needs OpenCV, which is not importable here: pass "
                             "solver=stitching_amd.CameraSolver() for the project's own") from e
    return cv


class CameraAdjuster:
    """https://docs.opencv.org/4.x/d5/d56/classcv_1_1detail_1_1BundleAdjusterBase.html"""

    CAMERA_ADJUSTER_CHOICES = ("ray", "reproj", "affine", "no")
    DEFAULT_CAMERA_ADJUSTER = "ray"
    DEFAULT_REFINEMENT_MASK = "xxxxx"

    def __init__(self, adjuster=DEFAULT_CAMERA_ADJUSTER, refinement_mask=DEFAULT_REFINEMENT_MASK, confidence_threshold=1.0, solver=None):
        """`solver`: a CameraSolver; it adjusts with this class's confidence_threshold.  "no" returns the cameras as they are.  Default:
        the cv2 adjuster the reference builds for the name."""
        self.solver = solver
        self.adjuster = None
        self.kind, self.confidence_threshold = adjuster, confidence_threshold
        self.refinement_mask = refinement_mask
        if solver is not None:
            if adjuster in ("reproj", "affine") and getattr(solver, "model", None) != adjuster:
                raise StitchingError(f'the "{adjuster}" camera adjuster has no counterpart in the solver: it adjusts rays')
            if adjuster not in self.CAMERA_ADJUSTER_CHOICES:
                raise StitchingError(f"unknown camera adjuster {adjuster!r}")
            self.set_refinement_mask(refinement_mask)
            return
        cv = _cv()
        choices = {"ray": cv.detail_BundleAdjusterRay, "reproj": cv.detail_BundleAdjusterReproj,
                   "affine": cv.detail_BundleAdjusterAffinePartial, "no": cv.detail_NoBundleAdjuster}
        self.adjuster = choices[adjuster]()
        self.set_refinement_mask(refinement_mask)
        self.adjuster.setConfThresh(confidence_threshold)

    def set_refinement_mask(self, refinement_mask):
        if self.solver is not None:
            if getattr(self.solver, "model", None) == "reproj":
                free_parameters(refinement_mask)  # five of "x" / "_", or refused
            elif refinement_mask != self.DEFAULT_REFINEMENT_MASK:
                raise StitchingError(f'the solver moves focal and rotation of every camera: refinement mask "xxxxx" only, got {refinement_mask!r}')
            self.refinement_mask = refinement_mask
            return
        cells = np.zeros((3, 3), np.uint8)
        for k, (r, c) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2))):
            if refinement_mask[k] == "x":
                cells[r, c] = 1
        self.adjuster.setRefinementMask(cells)

    def adjust(self, features, pairwise_matches, estimated_cameras):
        if self.solver is not None:
            if self.kind == "no":
                return estimated_cameras
            if getattr(self.solver, "model", None) == "reproj":
                return self.solver.adjust(features, pairwise_matches, estimated_cameras, conf_thresh=float(self.confidence_threshold),
                                          refinement_mask=self.refinement_mask)
            return self.solver.adjust(features, pairwise_matches, estimated_cameras, conf_thresh=float(self.confidence_threshold))
        ok, refined = self.adjuster.apply(features, pairwise_matches, estimated_cameras)
        if not ok:
            raise StitchingError("Camera parameters adjusting failed.")
        return refined
