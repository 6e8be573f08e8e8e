"""Seam finding on the device: SeamFinder::find for the "voronoi" and "no" finders.

`SeamEstimator` is duck-typed like the cv.detail finders the reference builds (stitching/seam_finder.py:14-35): `find(imgs, corners,
masks)` on the low-resolution warped images returns the seam masks.  The images are read for their sizes only.  "voronoi" runs
PairwiseSeamFinder::run's pairs level by level (host schedule: csrc/stx_seams_host.cpp), two HIP launches per level
(csrc/stx_seams.hip); "no" returns copies of the masks.  The algorithm restates OpenCV 4.x from recollection; tests/numpy_seams.py is
the contract and fidelity to real OpenCV is unpinned.

`ColorSeamEstimator` is the project's own colour-aware finder with the same interface (not OpenCV's DpSeamFinder): it reads the images'
pixels.  tests/numpy_color_seams.py is its contract.
"""
import ctypes as C

import numpy as np

from . import _lib, config
from ._marshal import adopt, count_then_fill, handles, host_array, image_spec, info_dict, int_pairs, one_context, ptr
from .device import DeviceImage, as_device, is_foreign_device_array
from .stitching_error import StitchingError

_INFO = [("pairs", int), ("levels", int), ("device_ms", float), ("device_ms_with_copy", float)]


def schedule(corners, sizes):
    """Host only (no GPU): run()'s overlapping pairs and their dependency levels.  -> (pairs (P, 6) int32 rows i, j, x, y, w, h of the
    roi; levels (P,) int32)."""
    n = len(sizes)
    cs, ss = int_pairs(corners, n), int_pairs(sizes, n)
    L = _lib.lib()

    def call(count, out):
        _lib.check(L.stx_seam_schedule(n, ptr(ss), ptr(cs), count, *([None] * 2 if out is None else [ptr(a) for a in out])))

    (pairs, levels), k = count_then_fill(call, C.c_int, lambda P: (np.zeros((P, 6), np.int32), np.zeros(P, np.int32)))
    return pairs[:k], levels[:k]


def _size_only(a, i):
    """how SeamEstimator reads an image: (w, h), and nothing of it goes to the device"""
    return image_spec(a, "image", i)[1], None


def _find(est, read_image, export, lead, imgs, corners, masks):
    """find() of both estimators.  read_image(a, i) -> ((w, h), the image whose pixels the export reads, or None: it takes masks alone).
    The images it returns go to the device, their handles in front of the masks', and decide with the masks whether the results stay
    there.  lead: the export's arguments between the context and n."""
    imgs, masks, corners = list(imgs), list(masks), [tuple(int(v) for v in c) for c in corners]
    if not (len(imgs) == len(masks) == len(corners)):
        raise StitchingError("find needs as many images, corners and masks")
    n = len(imgs)
    if n == 0:
        est.info = info_dict([0, 0, 0.0, 0.0], _INFO)
        return []
    sizes, read = [], []
    for i in range(n):
        wh, image = read_image(imgs[i], i)
        m, mwh, _, _ = image_spec(masks[i], "mask", i)
        if isinstance(m, np.ndarray) and (m.ndim != 2 or m.dtype != np.uint8):
            raise StitchingError(f"mask {i}: seam finding needs u8 masks with one channel, got {m.dtype} of shape {m.shape}")
        if mwh != wh:
            raise StitchingError(f"mask {i} is {mwh[0]}x{mwh[1]}, its image {wh[0]}x{wh[1]}")
        masks[i] = m
        sizes.append(wh)
        read += [] if image is None else [image]
    ctx = one_context(imgs + read + masks)  # a DeviceImage counts even where only its size is read
    resident = config.device_resident() or any(isinstance(a, DeviceImage) for a in read + masks)
    d_imgs, d_masks = [as_device(a, ctx) for a in read], [as_device(m, ctx) for m in masks]  # alive until the call is made
    image_handles = [handles(d_imgs)] if d_imgs else []
    ss, cs, outs, info = int_pairs(sizes, n), int_pairs(corners, n), handles([None] * n), np.zeros(4, np.float64)
    _lib.check(getattr(ctx._lib, export)(ctx.handle, *lead, n, ptr(ss), ptr(cs), *image_handles, handles(d_masks), outs, ptr(info)))
    est.info = info_dict(info, _INFO)
    return adopt(ctx, outs, resident)


class SeamEstimator:
    """SeamFinder::find on the device.  kind: "voronoi" (VoronoiSeamFinder) | "no" (NoSeamFinder).  Construction needs no GPU."""

    def __init__(self, kind):
        if kind not in _lib.SEAM_KINDS:
            raise StitchingError(f"unknown device seam finder {kind!r}: one of {sorted(_lib.SEAM_KINDS)}")
        self.kind = kind
        self.info = None  # of the last call: pairs, levels, device ms of the levels, device ms with the copy of the inputs

    def find(self, imgs, corners, masks):
        """Seam masks for images `imgs` (numpy arrays, cv.UMat-likes or DeviceImages: only their sizes are read) at `corners` with
        u8 masks `masks` (never written).  Returns new masks: DeviceImages when any mask is a DeviceImage or config.device_resident(),
        numpy arrays otherwise."""
        return _find(self, _size_only, "stx_seam_find", (_lib.SEAM_KINDS[self.kind],), imgs, corners, masks)


def _color_image(a, i):
    """u8 HxWx3 (numpy or DeviceImage) from what a caller hands a finder: u8 images, or the float32 images with integer values in
    0 .. 255 the reference's SeamFinder.find makes of them (stitching/seam_finder.py:33-35)."""
    if isinstance(a, DeviceImage) or is_foreign_device_array(a):
        a, wh, ch, dt = image_spec(a, "image", i)
        if dt != np.uint8 or ch != 3:
            raise StitchingError(f"image {i}: colour seams need u8 images with 3 channels, got {a.dtype} of shape {a.shape}")
        return wh, a
    a = host_array(a)  # its own refusal of every shape but HxWx3
    if a.ndim != 3 or a.shape[2] != 3 or a.dtype not in (np.uint8, np.float32):
        raise StitchingError(f"image {i}: colour seams need u8 (or float32 holding 0 .. 255) images of shape HxWx3, got {a.dtype} of "
                             f"shape {a.shape}")
    if a.dtype == np.float32:
        u = a.astype(np.uint8)
        if a.size and not (a.min() >= 0 and a.max() <= 255 and np.array_equal(u, a)):
            raise StitchingError(f"image {i}: float32 images must hold integers in 0 .. 255")
        a = u
    return (a.shape[1], a.shape[0]), a


class ColorSeamEstimator:
    """The project's own colour-aware seam finder on the device — NOT OpenCV's DpSeamFinder, and not behind the names "dp_color" /
    "dp_colorgrad" (those stay cv2's).  Pairwise like "voronoi" (the same pairs, order and dependency levels), integer only, one dynamic
    programme per overlapping pair: the cost of a pixel both masks hold is the squared BGR difference of the two images, the seam is the
    8-connected path of least cost along the overlap (vertical or horizontal by the images' centres), and it splits the pixels both masks
    hold between the two images.  tests/numpy_color_seams.py states the algorithm exactly and is the contract, byte for byte; DESIGN.md
    section 14 has the launch shape (csrc/stx_color_seams.hip).  Construction needs no GPU.

    Plug it in where a finder object goes: SeamFinder(name, estimator=ColorSeamEstimator()) or Composer(seam_estimator=...).

    Limits, refused with a StitchingError before anything is launched: a seam of at most MAX_SEAM_LENGTH pixels (u32 accumulators:
    16384 * 3 * 255^2 < 2^32) and at most MAX_CROSS_EXTENT pixels across it (two u32 accumulator rows in LDS: 32 KiB)."""

    MAX_SEAM_LENGTH = _lib.COLOR_SEAM_MAX_LENGTH
    MAX_CROSS_EXTENT = _lib.COLOR_SEAM_MAX_CROSS
    reads_device_images = True  # SeamFinder.find hands the images over untouched: device images stay in HBM

    def __init__(self):
        self.info = None  # of the last call: pairs, levels, device ms of the levels, device ms with the copy of the inputs

    def find(self, imgs, corners, masks):
        """Seam masks for the u8 BGR images `imgs` (numpy arrays, cv.UMat-likes or DeviceImages; float32 arrays of integers in 0 .. 255
        are cast) at `corners` with u8 masks `masks`; neither is written.  Returns new masks: DeviceImages when any input is a
        DeviceImage or config.device_resident(), numpy arrays otherwise."""
        return _find(self, _color_image, "stx_color_seam_find", (), imgs, corners, masks)
