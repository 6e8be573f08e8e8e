"""WaveCorrector with the reference's surface (stitching/camera_wave_corrector.py:7-28).

Without `solver=` it is the reference's class: cv.detail.waveCorrect — OpenCV's, on the host.  With `solver=CameraSolver()` the
rotations are corrected by the project's own solver, which knows "horiz", "vert" and "no"; "auto" stays cv2's.
"""
import numpy as np

from .stitching_error import StitchingError


def _cv():
    try:
        import cv2 as cv
    except ImportError as e:
        raise StitchingError("wave correction by cv.detail.waveCorrect needs OpenCV, which is not importable here: pass "
                             "solver=stitching_amd.CameraSolver() for the project's own") from e
    return cv


class WaveCorrector:
    """https://docs.opencv.org/4.x/d7/d74/group__stitching__rotation.html#ga8faf9588aebd5aeb6f8c649c82beb1fb"""

    WAVE_CORRECT_CHOICES = ("horiz", "vert", "auto", "no")
    DEFAULT_WAVE_CORRECTION = "horiz"

    def __init__(self, wave_correct_kind=DEFAULT_WAVE_CORRECTION, solver=None):
        """`solver`: a CameraSolver; it corrects with this class's kind.  Default: cv2, as the reference."""
        self.solver = solver
        self.kind = wave_correct_kind
        if wave_correct_kind not in self.WAVE_CORRECT_CHOICES:
            raise StitchingError(f"unknown wave correction {wave_correct_kind!r}")
        if solver is not None:
            if wave_correct_kind == "auto":
                raise StitchingError('wave correction "auto" is cv2\'s: the solver takes "horiz", "vert" or "no"')
            self.wave_correct_kind = wave_correct_kind
            return
        if wave_correct_kind == "no":
            self.wave_correct_kind = None
            return
        cv = _cv()
        self.wave_correct_kind = {"horiz": cv.detail.WAVE_CORRECT_HORIZ, "vert": cv.detail.WAVE_CORRECT_VERT,
                                  "auto": cv.detail.WAVE_CORRECT_AUTO}[wave_correct_kind]

    def correct(self, cameras):
        if self.solver is not None:
            return self.solver.correct(cameras, kind=self.kind)
        if self.wave_correct_kind is None:
            return cameras
        corrected = _cv().detail.waveCorrect([np.array(camera.R) for camera in cameras], self.wave_correct_kind)
        for camera, R in zip(cameras, corrected):
            camera.R = R
        return cameras
