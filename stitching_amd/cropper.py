"""Cropper and Rectangle with the reference's surface (stitching/cropper.py:10-151); the largest interior rectangle runs on the device.

`estimate_largest_interior_rectangle` replaces the reference's cv.findContours check and largestinteriorrectangle.lir with one call of
stx_crop_lir (csrc/stx_crop.hip): the mask stays on the device, four ints and two counts come back.  The rectangle arithmetic and the
cropping are the reference's own; cropping a DeviceImage gives a view of it (no copy).  tests/numpy_lir.py is the contract
(DESIGN.md section 11).  Deviations: an empty mask raises the reference's "Invalid Contour" StitchingError (the reference fails with an
AttributeError there), and among several rectangles of the largest area the one with the smallest y, then x, then the largest width is
returned, where the reference's choice is unpinned.
"""
import ctypes as C
from collections import namedtuple

import numpy as np

from . import _lib
from .blender import Blender
from ._marshal import host_array
from .device import DeviceImage, as_device, get_context, is_foreign_device_array
from .stitching_error import StitchingError

INVALID_CONTOUR = ("Invalid Contour. Run with --no-crop (using the stitch interface), crop=false (using the stitcher class) or "
                   "Cropper(False) (using the cropper class)")


class Rectangle(namedtuple("Rectangle", "x y width height")):
    __slots__ = ()

    @property
    def area(self):
        return self.width * self.height

    @property
    def corner(self):
        return (self.x, self.y)

    @property
    def size(self):
        return (self.width, self.height)

    @property
    def x2(self):
        return self.x + self.width

    @property
    def y2(self):
        return self.y + self.height

    def times(self, x):
        return Rectangle(*(int(round(i * x)) for i in self))

    def draw_on(self, img, color=(0, 0, 255), size=1):
        """cv2 drawing code of the verbose mode: the reference's, when cv2 is importable."""
        try:
            import cv2 as cv
        except ImportError as e:
            raise StitchingError("Rectangle.draw_on draws with cv2, which is not importable here") from e
        img = np.asarray(img)
        if len(img.shape) == 2:
            img = cv.cvtColor(img, cv.COLOR_GRAY2RGB)
        start_point = (self.x, self.y)
        end_point = (self.x2 - 1, self.y2 - 1)
        cv.rectangle(img, start_point, end_point, color, size)
        return img


def largest_interior_rectangle(mask, ctx=None):
    """One stx_crop_lir call on a u8 mask (numpy, `.get()`-able or DeviceImage; numpy is uploaded once).  -> ((x, y, w, h),
    (foreground components, holes), device ms).  The rectangle is computed whatever the counts are."""
    if is_foreign_device_array(mask):
        mask = as_device(mask, ctx)
    if not isinstance(mask, DeviceImage):
        mask = host_array(mask)
        if mask.ndim != 2:
            raise StitchingError(f"the panorama mask must be HxW, got shape {mask.shape}")
        if mask.dtype != np.uint8:
            mask = (mask != 0).astype(np.uint8)
    d = as_device(mask, ctx or (mask.ctx if isinstance(mask, DeviceImage) else get_context()))
    xywh, counts, info = (C.c_int * 4)(), (C.c_int * 2)(), (C.c_double * 1)()
    _lib.check(d.ctx._lib.stx_crop_lir(d.ctx.handle, d._h, xywh, counts, info))
    return tuple(int(v) for v in xywh), (int(counts[0]), int(counts[1])), float(info[0])


class Cropper:
    DEFAULT_CROP = True

    def __init__(self, crop=DEFAULT_CROP):
        self.do_crop = crop
        self.overlapping_rectangles = []
        self.cropping_rectangles = []
        self.info = None  # of the last estimate: {"contours": (components, holes), "device_ms": ...}

    def prepare(self, imgs, masks, corners, sizes):
        if self.do_crop:
            mask = self.estimate_panorama_mask(imgs, masks, corners, sizes)
            lir = self.estimate_largest_interior_rectangle(mask)
            corners = self.get_zero_center_corners(corners)
            rectangles = self.get_rectangles(corners, sizes)
            self.overlapping_rectangles = self.get_overlaps(rectangles, lir)
            self.intersection_rectangles = self.get_intersections(rectangles, self.overlapping_rectangles)

    def crop_images(self, imgs, aspect=1):
        for idx, img in enumerate(imgs):
            yield self.crop_img(img, idx, aspect)

    def crop_img(self, img, idx, aspect=1):
        if self.do_crop:
            intersection_rect = self.intersection_rectangles[idx]
            scaled_intersection_rect = intersection_rect.times(aspect)
            cropped_img = self.crop_rectangle(img, scaled_intersection_rect)
            return cropped_img
        return img

    def crop_rois(self, corners, sizes, aspect=1):
        if self.do_crop:
            scaled_overlaps = [r.times(aspect) for r in self.overlapping_rectangles]
            cropped_corners = [r.corner for r in scaled_overlaps]
            cropped_corners = self.get_zero_center_corners(cropped_corners)
            cropped_sizes = [r.size for r in scaled_overlaps]
            return cropped_corners, cropped_sizes
        return corners, sizes

    @staticmethod
    def estimate_panorama_mask(imgs, masks, corners, sizes):
        """this package's Blender.create_panorama: a DeviceImage under device residency, numpy otherwise."""
        _, mask = Blender.create_panorama(imgs, masks, corners, sizes)
        return mask

    def estimate_largest_interior_rectangle(self, mask):
        lir, counts, ms = largest_interior_rectangle(mask)
        self.info = {"contours": counts, "device_ms": ms}
        if counts != (1, 0):
            raise StitchingError(INVALID_CONTOUR)
        return Rectangle(*lir)

    @staticmethod
    def get_zero_center_corners(corners):
        min_corner_x = min([corner[0] for corner in corners])
        min_corner_y = min([corner[1] for corner in corners])
        return [(x - min_corner_x, y - min_corner_y) for x, y in corners]

    @staticmethod
    def get_rectangles(corners, sizes):
        rectangles = []
        for corner, size in zip(corners, sizes):
            rectangle = Rectangle(*corner, *size)
            rectangles.append(rectangle)
        return rectangles

    @staticmethod
    def get_overlaps(rectangles, lir):
        return [Cropper.get_overlap(r, lir) for r in rectangles]

    @staticmethod
    def get_overlap(rectangle1, rectangle2):
        x1 = max(rectangle1.x, rectangle2.x)
        y1 = max(rectangle1.y, rectangle2.y)
        x2 = min(rectangle1.x2, rectangle2.x2)
        y2 = min(rectangle1.y2, rectangle2.y2)
        if x2 < x1 or y2 < y1:
            raise StitchingError("Rectangles do not overlap!")
        return Rectangle(x1, y1, x2 - x1, y2 - y1)

    @staticmethod
    def get_intersections(rectangles, overlapping_rectangles):
        return [Cropper.get_intersection(r, overlap_r) for r, overlap_r in zip(rectangles, overlapping_rectangles)]

    @staticmethod
    def get_intersection(rectangle, overlapping_rectangle):
        x = abs(overlapping_rectangle.x - rectangle.x)
        y = abs(overlapping_rectangle.y - rectangle.y)
        width = overlapping_rectangle.width
        height = overlapping_rectangle.height
        return Rectangle(x, y, width, height)

    @staticmethod
    def crop_rectangle(img, rectangle):
        return img[rectangle.y : rectangle.y2, rectangle.x : rectangle.x2]
