"""stitching_amd — MI355X (gfx950) back end for the warp + blend hot path of
OpenStitching/stitching: `Warper` and `Blender` with the reference's class surface, executed by
hand-written HIP kernels behind the C ABI in include/stitching_amd.h (loaded with ctypes; no
PyTorch, no OpenCV, no CPU fallback)."""
from .blender import Blender
from .camera import CameraParams
from .camera_adjuster import CameraAdjuster
from .camera_estimation import CameraSolver
from .camera_estimator import CameraEstimator
from .camera_wave_corrector import WaveCorrector
from .config import (device_resident, exposure_estimator, exposure_solver, pyrdown_mode, remap_mode, seam_estimator, set_device_resident,
                     set_exposure_estimator, set_exposure_solver, set_pyrdown_mode, set_remap_mode, set_seam_estimator, set_trig_mode,
                     trig_mode)
from .cropper import Cropper, Rectangle
from .device import (Context, DeviceImage, as_device, device_count, get_context, pinned_empty, set_default_device, shrink_masks_all,
                     with_validity)
from .exposure_error_compensator import ExposureErrorCompensator
from .exposure_estimation import ExposureEstimator
from .exposure_tracking import ExposureTracker
from .feature_detector import FeatureDetector
from .feature_estimation import FeatureEstimator, ImageFeatures
from .feature_matcher import FeatureMatcher
from .match_estimation import MatchEstimator, MatchesInfo
from .images import Images, MegapixDownscaler, MegapixScaler
from .emit import emit, emit_all
from .ingest import ingest, ingest_all, parse_cuda_array_interface
from .pipeline import AffineComposer, ComposePlan, Composer
from .rectify import LensMap, rectify, rectify_all
from .seam_estimation import ColorSeamEstimator, SeamEstimator
from .seam_finder import SeamFinder, resize_linear_exact, resize_linear_exact_all
from .stitching_error import StitchingError, StitchingWarning
from .subsetter import Subsetter
from .timelapser import Timelapser
from .warper import Warper

__all__ = [
    "AffineComposer", "Blender", "CameraAdjuster", "CameraEstimator", "CameraParams", "CameraSolver", "ColorSeamEstimator", "ComposePlan", "Composer", "Context", "Cropper", "Rectangle", "DeviceImage", "ExposureErrorCompensator", "ExposureEstimator", "ExposureTracker", "FeatureDetector", "FeatureEstimator", "FeatureMatcher", "ImageFeatures", "Images", "MatchEstimator", "MatchesInfo", "MegapixDownscaler", "MegapixScaler", "StitchingError", "StitchingWarning",
    "SeamEstimator", "SeamFinder", "Subsetter", "Timelapser", "Warper", "WaveCorrector", "resize_linear_exact", "resize_linear_exact_all",
    "LensMap", "rectify", "rectify_all", "with_validity", "shrink_masks_all",
    "as_device", "emit", "emit_all", "ingest", "ingest_all", "parse_cuda_array_interface", "device_count", "pinned_empty", "device_resident", "get_context", "set_default_device", "set_device_resident", "set_trig_mode", "trig_mode", "set_remap_mode", "remap_mode", "set_pyrdown_mode", "pyrdown_mode",
    "set_exposure_estimator", "exposure_estimator", "set_exposure_solver", "exposure_solver", "set_seam_estimator", "seam_estimator",
]
__version__ = "0.1.0"
