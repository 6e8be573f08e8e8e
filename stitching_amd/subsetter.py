"""Subsetter with the reference's surface (stitching/subsetter.py:11-79).

Without `solver=` it is the reference's class: cv.detail.leaveBiggestComponent and matchesGraphAsString — OpenCV's, on the host.  With
`solver=CameraSolver()` the indices come from the project's own rule (camera_estimation.largest_component) with this class's
confidence_threshold, and no matches graph is written.  The static helpers need no cv2.
"""
import warnings

import numpy as np

from .camera_estimation import NO_MATCH_MESSAGE, NOT_ALL_MESSAGE, CameraSolver, confidences, largest_component
from .stitching_error import StitchingError, StitchingWarning


def _cv():
    try:
        import cv2 as cv
    except ImportError as e:
        raise StitchingError("the subset step by cv.detail.leaveBiggestComponent needs OpenCV, which is not importable here: pass "
                             "solver=stitching_amd.CameraSolver() for the project's own") from e
    return cv


class Subsetter:
    """https://docs.opencv.org/4.x/d7/d74/group__stitching__rotation.html#ga855d2fccbcfc3b3477b34d415be5e786 and
    https://docs.opencv.org/4.x/d7/d74/group__stitching__rotation.html#gabaeb9dab170ea8066ae2583bf3a669e9"""

    DEFAULT_CONFIDENCE_THRESHOLD = 1
    DEFAULT_MATCHES_GRAPH_DOT_FILE = None

    def __init__(self, confidence_threshold=DEFAULT_CONFIDENCE_THRESHOLD, matches_graph_dot_file=DEFAULT_MATCHES_GRAPH_DOT_FILE,
                 solver=None):
        """`solver`: a CameraSolver; it then finds the indices with this class's confidence_threshold.  The matches graph is
        OpenCV's text: with a solver a matches_graph_dot_file is refused.  Default: cv2, as the reference."""
        self.confidence_threshold = confidence_threshold
        self.save_file = matches_graph_dot_file
        self.solver = solver
        if solver is not None:
            if matches_graph_dot_file:
                raise StitchingError("the matches graph dot file is written by OpenCV's matchesGraphAsString: not available with solver=")
        else:
            _cv()

    def subset(self, img_names, features, matches):
        """indices of the images to keep; writes the matches graph first where a file was named"""
        self.save_matches_graph_dot_file(img_names, matches)
        keep = self.get_indices_to_keep(features, matches)
        if len(keep) != len(img_names):
            warnings.warn(NOT_ALL_MESSAGE, StitchingWarning)
        return keep

    def save_matches_graph_dot_file(self, img_names, pairwise_matches):
        if not self.save_file:
            return
        text = self.get_matches_graph(img_names, pairwise_matches)
        with open(self.save_file, "w") as out:
            out.write(text)

    def get_matches_graph(self, img_names, pairwise_matches):
        if self.solver is not None:
            raise StitchingError("the matches graph is OpenCV's matchesGraphAsString: not available with solver=")
        # OpenCV draws no edge at a threshold of exactly 0: a tiny positive one stands in for it
        threshold = self.confidence_threshold if self.confidence_threshold != 0 else 1e-5
        return _cv().detail.matchesGraphAsString(img_names, pairwise_matches, threshold)

    def get_indices_to_keep(self, features, pairwise_matches):
        if self.solver is not None:
            n = len(list(features))
            keep = np.array(largest_component(confidences(pairwise_matches, n), float(self.confidence_threshold)), np.int64)
        else:
            keep = np.ravel(_cv().detail.leaveBiggestComponent(features, pairwise_matches, self.confidence_threshold))
        if len(keep) < 2:
            raise StitchingError(NO_MATCH_MESSAGE)
        return keep

    @staticmethod
    def subset_list(list_to_subset, indices):
        return [list_to_subset[int(k)] for k in indices]

    @staticmethod
    def subset_matches(pairwise_matches, indices):
        """the entries of the kept images, row-major"""
        return CameraSolver.subset_matches(pairwise_matches, indices)
