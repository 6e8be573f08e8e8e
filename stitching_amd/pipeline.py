"""Device-resident warp -> blend driver (the hot loop of stitching/stitcher.py:117-128 with the
stages outside the path — exposure compensation, seam masks, cropping — switched off, as in
BASELINE.json's synthetic configurations).

One image is in flight on the host side exactly as in the reference
(stitching/stitcher.py:247-254), but nothing waits for the GPU between images: warps, pyramid
builds and the final gather are enqueued on one HIP stream; the only host syncs are the batched
ROI read-back at the start and whatever the caller does with the result.
"""
import ctypes as C
import warnings

import numpy as np

from . import _lib, config
from .blender import Blender
from .cropper import Cropper
from .device import DeviceImage, as_device, get_context, is_foreign_device_array, shrink_masks_all, with_validity
from .exposure_error_compensator import ExposureErrorCompensator
from .images import Images, MegapixDownscaler
from .rectify import lens_list, rectify_all
from .seam_estimation import SeamEstimator
from .seam_finder import DEVICE_SEAM_FINDERS, SeamFinder
from .stitching_error import StitchingError, StitchingWarning
from .synthetic import blend_strength_for_bands
from .warper import Warper, WarpTables


def mask_box(mask):
    """(first column, one past the last column, width, first row, one past the last row, height) of the non-zero values of a
    host mask, or None when there are none"""
    m2 = mask.reshape(mask.shape[0], mask.shape[1], -1).any(axis=2)
    nx, ny = np.flatnonzero(m2.any(axis=0)), np.flatnonzero(m2.any(axis=1))
    if not nx.size:
        return None
    return (int(nx[0]), int(nx[-1]) + 1, int(mask.shape[1]), int(ny[0]), int(ny[-1]) + 1, int(mask.shape[0]))


def view_rects(handle, corners, sizes, boxes, min_gain=0.9):
    """Per image the rectangle (x0, x1, y0, y1) of its warped image that can influence the panorama, or None (all of it);
    None altogether when nothing is cut.  `handle`: the multi-band blender prepared on (corners, sizes) — a geometry-only one
    (distributed.make_shard_blender(None, roi, bands)) will do; `boxes`: mask_box of the mask each image is fed with, at
    its final or at a lower resolution.

    The fed mask of image k is non-zero inside the columns [m0, m1) and rows [n0, n1) only.  Its weight pyramid W_l is then
    non-zero within 2^(l+1) - 2 level-0 pixels of that box, at most 2^(B+1) — call that box, snapped outwards to the band
    grid, the image's band.  Outside its band the image adds (short)(L * 0.f) = 0 and 0.f whatever its pixels are; inside
    it, L and W are what the whole image gives as long as everything within the pyramids' reach of the band is present:
    exactly the guarantee of the strips of the sharded blender (`stx_strip_rect`; `stx_view_rect` adds the
    same range along y), whose cut edges are farther from the band than any pyramid tap.  So the view for its own band is
    all of image k that has to exist.  Seam masks given at low resolution: the final mask is dilate(3x3) ->
    INTER_LINEAR_EXACT -> AND, non-zero at x only if a dilated low-resolution column floor(sx) or floor(sx) + 1 is,
    sx = (x + 0.5) * lw / w - 0.5 (rows alike).  (tests/test_crop_theory.py checks the statement on the CPU oracle.)"""
    B = handle.num_bands()
    if B <= 0:
        return None
    roi = Blender.result_roi(corners, sizes)
    align, reach = max(8, 1 << B), 2 << B

    def band(lo, hi, size, msize, origin):
        if msize != size:  # low-resolution seam mask: the final-mask positions that can be non-zero
            lo = int(np.floor((lo - 2 + 0.5) * size / msize - 0.5)) - 1
            hi = int(np.ceil((hi + 2 + 0.5) * size / msize - 0.5)) + 1
        lo, hi = max(lo, 0), min(hi, size)
        return max(((origin + lo - reach) // align) * align, 0), -((-(origin + hi + reach)) // align) * align

    out = []
    for (cx, cy), (w, h), box in zip(corners, sizes, boxes):
        if box is None:
            out.append(None)
            continue
        bx0, bx1 = band(box[0], box[1], w, box[2], cx - roi[0])
        by0, by1 = band(box[3], box[4], h, box[5], cy - roi[1])
        r = (C.c_int * 4)()
        _lib.check(_lib.lib().stx_view_rect(handle._h, int(w), int(h), int(cx), int(cy), int(bx0), int(bx1), int(by0), int(by1), r))
        x0, x1, y0, y1 = (int(v) for v in r)
        if x1 <= x0 or y1 <= y0:
            out.append(None)
            continue
        if x1 - x0 > min_gain * w:
            x0, x1 = 0, w
        if y1 - y0 > min_gain * h:
            y0, y1 = 0, h
        out.append((x0, x1, y0, y1) if (x1 - x0) * (y1 - y0) < w * h else None)
    return None if all(o is None for o in out) else out


def clip_rectangle(rect, width, height):
    """(x0, x1, y0, y1) of what `Cropper.crop_rectangle(img, rect)` — img[rect.y:rect.y2, rect.x:rect.x2] — keeps of a width x height
    image: numpy's slice rules (ends clipped to the image, negative indices counted from the far end, never a negative extent)."""
    x0, x1, _ = slice(rect.x, rect.x2).indices(int(width))
    y0, y1, _ = slice(rect.y, rect.y2).indices(int(height))
    return x0, max(x1, x0), y0, max(y1, y0)


def _split_cropper(cropper, crop_aspect):
    """cropper= takes a prepared Cropper (its aspect in crop_aspect=) or the pair (cropper, lir_aspect); a Cropper(False) crops nothing"""
    if isinstance(cropper, (tuple, list)):
        cropper, crop_aspect = cropper
    if cropper is not None and not cropper.do_crop:
        cropper = None
    if cropper is not None and not getattr(cropper, "intersection_rectangles", None):
        raise StitchingError("the cropper is not prepared: Cropper.prepare(imgs, masks, corners, sizes) on the low-resolution warps comes first")
    return cropper, crop_aspect


class _RigGeometry:
    """What a panorama of a rig needs besides its pixels (StitchJob keeps one between runs): the rectangles to warp, where and with which
    masks they are fed, what the blender is prepared on — and the blender's weight pyramids, which follow from all of that."""

    __slots__ = ("key", "rects", "prep_corners", "prep_sizes", "feed_corners", "feed_masks", "blend_strength", "crop", "gain_in_warp",
                 "gain_corners", "gain_sub", "weights", "tables", "blender")

    def __init__(self):
        self.key = self.weights = self.crop = self.gain_corners = self.gain_sub = None
        self.tables = WarpTables()  # the warp's column / row tables: filled by the first images-only warp into the kept rectangles
        self.blender = None  # the pass's own prepared blender, where it needed one before its warps: taken by the run that made it
        self.gain_in_warp = True


def rig_key(cam_bytes, camera_aspect, warper_type, scale, sizes, blender_type, num_bands, blend_strength, modes, cropper, crop_aspect):
    """Everything the geometry of a rig depends on, as one hashable value: cameras (the K, R arrays as bytes) and their aspect, warper and
    the scale as it is NOW (Warper.set_scale may follow the constructor), frame sizes, blender and its width (num_bands where given — the
    strength is then derived from it and the ROIs — else blend_strength), the process-wide trig / remap / pyrDown modes, the cropper's
    rectangles and aspect.  The compensator is no part of it: gains change pixels, never a rectangle or a mask."""
    crop = None
    if cropper is not None:
        crop = (tuple(tuple(int(v) for v in r) for r in cropper.intersection_rectangles), float(crop_aspect))
    return (cam_bytes, float(camera_aspect), str(warper_type), None if scale is None else float(scale), tuple((int(w), int(h)) for w, h in sizes),
            str(blender_type), None if num_bands is None else int(num_bands), float(blend_strength) if num_bands is None else None,
            tuple(modes), crop)


class OwnedMasks(list):
    """Source validity masks the library made itself (a lens's masks, their shrunk copies): device images nobody else writes, so a job
    that is given them may keep its geometry as with host arrays."""


def masks_belong_to_job(feed_masks, seam_masks, source_masks=None):
    """The condition of geometry reuse (and of the seam-cell crops): no mask input, or host arrays — the job uploaded its own copies.  A
    mask given as a device array may be rewritten by its owner between runs.  source_masks: the frames' validity masks likewise — host
    arrays (None entries: no mask) or OwnedMasks belong to the job."""
    given = feed_masks if feed_masks is not None else seam_masks
    if source_masks is not None and not isinstance(source_masks, OwnedMasks) and \
            not all(m is None or isinstance(m, np.ndarray) for m in source_masks):
        return False
    return given is None or all(isinstance(m, np.ndarray) for m in given)


class _LensWarper:
    """StitchJob's warper when the job has lenses: a Warper whose warp_images_and_masks takes DISTORTED frames through their lenses
    (Warper.warp_images_through_lenses).  The job's own code is the same with and without lenses — the rectangles,
    the masks and the ROIs it sees are those of the rectified frames:
      * warped masks do not depend on pixel values: the existing mask-only launch over frames of the rectified sizes makes them (once per
        rig; the frames are placeholders that are never read, they carry the rectified-size source masks where the job has any);
      * images come from stx_warp_lens_batch into the same rectangles;
      * gains are a second pass over the warped images (the plain `apply`, or stx_block_gain_apply_batch with the rectangle's place in
        the whole warped image): byte for byte the gain applied to the ungained warp."""

    def __init__(self, warper, lenses, source_masks):
        self._warper, self._lenses, self._source_masks = warper, lenses, source_masks
        self._rois = None  # (key, ROIs of the rectified frames): what a block gain's map lies over

    def __getattr__(self, name):
        return getattr(self._warper, name)

    def set_scale(self, cameras):
        self._warper.set_scale(cameras)

    def _placeholders(self, ctx):
        out = []
        for i, lens in enumerate(self._lenses):
            h = C.c_void_p()
            _lib.check(ctx._lib.stx_buf_alloc(ctx.handle, lens.dst_size[0], lens.dst_size[1], 3, _lib.U8, C.byref(h)))
            d = DeviceImage(ctx, h)
            m = None if self._source_masks is None else self._source_masks[i]
            out.append(d if m is None else with_validity(d, m))
        return out

    def _full_rois(self, cameras, aspect, camera_arrays):
        sizes = [lens.dst_size for lens in self._lenses]
        Ks, Rs = camera_arrays if camera_arrays is not None else self._warper.camera_arrays(cameras, aspect)
        key = (Ks.tobytes(), Rs.tobytes(), float(aspect), self._warper.scale, self._warper.warper_type, config.trig_mode())
        if self._rois is None or self._rois[0] != key:
            corners, wh = self._warper.warp_rois(sizes, cameras, aspect, camera_arrays=(Ks, Rs))
            self._rois = (key, [tuple(c) + tuple(z) for c, z in zip(corners, wh)])
        return self._rois[1]

    def warp_images_and_masks(self, imgs, cameras, aspect=1, rects=None, compensator=None, with_rois=False, camera_arrays=None, masks=True,
                              tables=None):
        ctx = self._warper._ctx()
        cameras = list(cameras)
        masks_out = None
        if masks:
            _, masks_out, rois = self._warper.warp_images_and_masks(self._placeholders(ctx), cameras, aspect, rects=rects, with_rois=with_rois,
                                                                    camera_arrays=camera_arrays, images=False)
            if rects is None:
                rects = rois
        elif rects is None:
            raise StitchingError("masks=False needs rects: the rectangles of the call that made the masks")
        out, rois = self._warper.warp_images_through_lenses(imgs, self._lenses, cameras, aspect, rects=rects, camera_arrays=camera_arrays,
                                                            tables=tables)
        if compensator is not None and compensator.compensator_type != "no":
            corners, sub = [r[0:2] for r in rois], None
            if compensator.compensator_type in ("gain_blocks", "channel_blocks"):
                full = self._full_rois(cameras, aspect, camera_arrays)
                sub = [(f[2], f[3], r[0] - f[0], r[1] - f[1]) for r, f in zip(rois, full)]
            out = compensator.apply_all(corners, out, None, sub=sub, ctx=ctx)
        return out, masks_out, rois


class StitchJob:
    """Pre-staged inputs of one panorama — or of the panoramas of one rig: device-resident source frames + cameras.

    Between runs the job keeps what does not depend on the pixels (reuse_geometry=True): the ROIs, the rectangles it warps, the masks it
    feeds (the warped masks after SeamFinder.resize_all, slicing or cropping) and the weight pyramids of the multi-band blender — device
    memory of about P_w + 0.8 P_f bytes (P_w: pixels of the warped masks, P_f: pixels of the feed rectangles; roughly 150 MB for eight
    4000 x 3000 frames at 5 bands) until release_geometry() or the end of the job.  Warped images are never kept.  With an
    exposure_tracker the job also keeps the tracker's lattice grids (P_w / stride^2 bytes) and every run measures its warped images for
    the next one (stitching_amd.exposure_tracking)."""

    def __init__(self, frames, cameras, warper_type="spherical", blender_type="multiband", num_bands=None,
                 blend_strength=Blender.DEFAULT_BLEND_STRENGTH, ctx=None, async_upload=False, feed_masks=None, seam_masks=None,
                 crop_to_masks=True, compensator=None, cropper=None, crop_aspect=1, camera_aspect=1, reuse_geometry=True, source_masks=None,
                 lenses=None, exposure_tracker=None):
        """async_upload: numpy frames in page-locked memory (pinned_empty) are only queued for upload; they must stay
        untouched until ctx.sync() (a streaming caller alternates two contexts).
        feed_masks: final-resolution u8 masks fed to the blender instead of the warped masks (seam masks already at the
        warped size); seam_masks: LOW-resolution seam masks, resized on the device exactly as the reference
        does per panorama (SeamFinder.resize, stitching/stitcher.py:124: dilate, INTER_LINEAR_EXACT, AND with the warped
        mask) — its grey edges make the masks non-binary.
        crop_to_masks (multi-band blender, feed_masks / seam_masks given as host arrays): a seam mask keeps one cell of its
        image, and nothing farther than the pyramids reach from that cell can touch the panorama.  The reference warps
        every image whole and cuts afterwards (stitching/stitcher.py:119-127); here only the rectangle the blender can see
        are warped, masked and fed — the same panorama bit for bit (`view_rects`).
        compensator: an ExposureErrorCompensator with its gains set (the low-resolution pass made them): applied to the warped
        images between warp and feed (stitching/stitcher.py:123,219-221) — all images in one batched launch; on cropped images the
        gain maps are laid over the whole warped image (the rectangle's offset travels with it).
        cropper: a prepared Cropper (Cropper.prepare on the low-resolution warps) with crop_aspect= its lir_aspect, or the pair (cropper,
        lir_aspect): stitching/stitcher.py:119-121,198-208 — only intersection_rectangles[i].times(crop_aspect) of every warped image
        is warped, clipped as Cropper.crop_rectangle's slice clips it, and the blender is prepared on crop_rois(corners, sizes,
        crop_aspect): byte for byte "warp whole, Cropper.crop_images, feed".  feed_masks / seam_masks then belong to the CROPPED images,
        and the block compensators' gain maps lie over the cropped image (apply on a cropped image, as in the reference) — a seam-cell
        crop inside it carries its offset in the cropped image.
        camera_aspect: the frames are camera_aspect times the size the cameras were estimated on (Warper's `aspect`).
        reuse_geometry: the first run() makes the geometry of the rig (ROI pass, warped masks, seam-mask resize, weight pyramids) and
        keeps it under rig_key(...); a later run with an equal key warps the images alone into the kept rectangles, feeds the kept masks
        and builds its pyramids without their weight half — the same bytes, made once.  A key that differs (Warper.set_scale with other
        cameras, a process-wide arithmetic mode, ...) drops the kept state, and that run is a first run.  Only where every mask input
        belongs to the job (masks_belong_to_job); jobs with device-array masks, and reuse_geometry=False, redo everything every run.
        source_masks: one validity mask per frame (u8, the frame's size, non-zero = picture; None entries: none): the warped masks are
        the nearest-neighbour warps of these instead of warped rectangles (with_validity) — whatever the job then
        does with warped masks (feeding, SeamFinder.resize) sees them.  Attached once, and again to the frames of set_frames /
        run(frames=).  ROIs, the blender's rectangle and view_rects do not change: a source mask changes what is inside a warped mask,
        never its rectangle.  Host arrays belong to the job; device arrays of the caller turn reuse_geometry off.
        lenses: one LensMap per frame, or one for all: the frames (also those of set_frames / run(frames=)) are DISTORTED frames of the
        lenses' source sizes, and every run takes them to the panorama in one resampling (Warper.warp_images_through_lenses; DESIGN.md
        section 24) instead of rectifying first.  Cameras, source_masks, rectangles and ROIs belong to the rectified frames (the lenses'
        dst_size); the warped masks are those of a job over rectified frames, byte for byte; gains are applied as a second pass;
        source_masks="lens" takes the masks that rectification returns (rectify_all(masks=True), once, at construction).  The
        panorama's pixels differ from rectify-then-warp (one bilinear blend instead of two).
        exposure_tracker: an ExposureTracker (stitching_amd.exposure_tracking) — every run measures its warped,
        compensated images on a lattice of the overlaps and the NEXT run applies compensator gains x the tracker's residual gains
        (run 0: the compensator's own).  The compensator is read, never written.  One tracker per job; it needs reuse_geometry to
        hold (the lattice grids are part of what the job keeps: about P_w / stride^2 bytes), so reuse_geometry=False and device-array
        masks of the caller are refused with it.  The one host wait it adds is for the previous run's statistics, at the start of a run."""
        cropper, crop_aspect = _split_cropper(cropper, crop_aspect)
        if len(frames) != len(cameras) or not frames:
            raise StitchingError("need one camera per frame and at least one frame")
        self.lenses = None if lenses is None else lens_list(lenses, len(frames))
        self.ctx = ctx or get_context()
        self.frames = [as_device(f, self.ctx, wait=not async_upload) for f in frames]
        self.source_masks = None
        if isinstance(source_masks, str):  # "lens" (with lenses): the masks rectification returns, made here, once
            if source_masks != "lens" or self.lenses is None:
                raise StitchingError(f"source_masks={source_masks!r}: a list of masks, or \"lens\" with lenses")
            source_masks = OwnedMasks(rectify_all(self.frames, self.lenses, masks=True, ctx=self.ctx)[1])
        if source_masks is not None:
            if len(source_masks) != len(self.frames):
                raise StitchingError(f"{len(source_masks)} source masks for {len(self.frames)} frames")
            self.source_masks = [None if m is None else as_device(m, self.ctx) for m in source_masks]
            self.frames = self._with_source_masks(self.frames)
        self.cameras = list(cameras)
        self.frame_sizes = self.sizes = [(f.width, f.height) for f in self.frames]  # sizes: what cameras and ROIs belong to
        self.warper = Warper(warper_type, ctx=self.ctx)
        if self.lenses is not None:
            if self.frame_sizes != [lens.src_size for lens in self.lenses]:
                raise StitchingError(f"the lenses were made for frames of sizes {[lens.src_size for lens in self.lenses]}, got {self.frame_sizes}")
            self.sizes = [lens.dst_size for lens in self.lenses]
            self.warper = _LensWarper(self.warper, self.lenses, self.source_masks)
        self.warper.set_scale(self.cameras)
        self.blender_type = blender_type
        self.compensator = compensator
        self.num_bands = num_bands
        self.blend_strength = blend_strength
        self.corners = self.warped_sizes = None
        self.cropper, self.crop_aspect, self.camera_aspect = cropper, crop_aspect, camera_aspect
        if cropper is not None and len(cropper.intersection_rectangles) != len(self.frames):
            raise StitchingError(f"the cropper was prepared on {len(cropper.intersection_rectangles)} images, the job has {len(self.frames)}")
        self._cam_arrays = self.warper.camera_arrays(self.cameras, camera_aspect)  # K, R as the batched entry points take them: built once
        self._cam_bytes = self._cam_arrays[0].tobytes() + self._cam_arrays[1].tobytes()
        # per mask the columns [a, b) and rows [c, d) that hold a non-zero value, and the mask's size (host arrays only: no
        # read-back here)
        self._mask_cols = None
        given = feed_masks if feed_masks is not None else seam_masks
        if crop_to_masks and given is not None and all(isinstance(m, np.ndarray) for m in given):
            self._mask_cols = [mask_box(m) for m in given]
        self._crop_cache = None
        self.reuse_geometry = bool(reuse_geometry) and masks_belong_to_job(feed_masks, seam_masks, source_masks)
        self._geometry = None
        self.last_reused = self.last_weights_adopted = False  # of the last run: kept geometry used / weight pyramids adopted by its blender
        self.feed_masks = None if feed_masks is None else [as_device(m, self.ctx) for m in feed_masks]
        self.seam_masks = None if seam_masks is None else [as_device(m, self.ctx) for m in seam_masks]
        self.exposure_tracker, self._tracked = exposure_tracker, None
        if exposure_tracker is not None:
            from .exposure_tracking import ExposureTracker, _TrackedCompensator

            if not isinstance(exposure_tracker, ExposureTracker):
                raise StitchingError(f"exposure_tracker= takes an ExposureTracker, got {type(exposure_tracker).__name__}")
            if not self.reuse_geometry:
                raise StitchingError("an exposure tracker measures on what the job keeps between runs: it needs reuse_geometry=True and masks "
                                     "that belong to the job (host arrays, not device arrays of the caller)")
            exposure_tracker._bind(self, len(self.frames))
            self._tracked = _TrackedCompensator(compensator, exposure_tracker)

    def _run_compensator(self):
        """the compensator of this run: the job's own, or with a tracker the one that applies its gains x the tracker's residuals —
        after collect + update for the previous run"""
        if self._tracked is None:
            return self.compensator
        self._tracked.refresh(self.exposure_tracker._begin_run())
        return self._tracked

    def _with_source_masks(self, frames):
        """the job's validity masks on (new) frames: new handles, the frames' own are not changed"""
        if self.lenses is not None:  # the masks belong to the rectified frames: _LensWarper has them
            return frames
        return [f if m is None else with_validity(f, m) for f, m in zip(frames, self.source_masks)]

    @property
    def source_pixels(self):
        return sum(w * h for w, h in self.sizes)

    def plan(self):
        """Eager ROI pass (stitching/stitcher.py:188 warp_rois is eager too); one device sync."""
        self._adopt(*self.warper.warp_rois(self.sizes, self.cameras, self.camera_aspect, camera_arrays=self._cam_arrays))
        return self.corners, self.warped_sizes

    def _adopt(self, corners, warped_sizes):
        """this panorama's ROIs -> the job's plan"""
        self.corners, self.warped_sizes = corners, warped_sizes
        if any(w <= 0 or h <= 0 for w, h in self.warped_sizes):
            raise StitchingError(f"degenerate warp roi {self.warped_sizes}: the {self.warper.warper_type!r} projection cannot "
                                 "represent these cameras")
        if self.num_bands is not None:
            roi = Blender.result_roi(self.corners, self.warped_sizes)
            self.blend_strength = blend_strength_for_bands(self.num_bands, roi[2], roi[3])

    def _crop_rects(self, handle, corners, sizes):
        """see view_rects"""
        key = (tuple(corners), tuple(sizes), self.blend_strength)
        if self._crop_cache is None or self._crop_cache[0] != key:
            self._crop_cache = (key, view_rects(handle, corners, sizes, self._mask_cols))
        return self._crop_cache[1]

    def set_frames(self, frames):
        """New frames of the same rig: the same number, the same sizes (ComposePlan.check_frames's rule)."""
        frames = list(frames)
        got = [Images.get_image_size(f) for f in frames]
        if got != [tuple(z) for z in self.frame_sizes]:
            raise StitchingError(f"the job was made for frames of sizes {self.frame_sizes}, got {got}: same rig, same sizes")
        self.frames = [as_device(f, self.ctx) for f in frames]
        if self.source_masks is not None:
            self.frames = self._with_source_masks(self.frames)

    def release_geometry(self):
        """Drop what the job keeps between runs (masks, weight pyramids: see the class docstring); the next run is a first run."""
        g, self._geometry = self._geometry, None
        if g is not None and g.weights is not None:
            g.weights.free()
        if g is not None:
            g.tables.free()
        if self.exposure_tracker is not None:
            self.exposure_tracker._release()  # the lattice grids go with the geometry; the residual gains survive

    def geometry_key(self):
        """rig_key of the job as it stands now"""
        modes = (config.trig_mode(), config.remap_mode()) + tuple(config.pyrdown_mode())
        key = rig_key(self._cam_bytes, self.camera_aspect, self.warper.warper_type, self.warper.scale, self.sizes, self.blender_type,
                      self.num_bands, self.blend_strength, modes, self.cropper, self.crop_aspect)
        # the lenses' identity: another lens is another rig (a LensMap's nodes cannot be written)
        return key if self.lenses is None else key + (tuple(id(lens) for lens in self.lenses),)

    def run(self, frames=None):
        """warp every frame, feed it, blend.  Returns device-resident (panorama u8x3, mask u8).
        frames: new frames of the same sizes — the next panorama of the same rig (set_frames)."""
        if frames is not None:
            self.set_frames(frames)
        prev = config.device_resident()
        config.set_device_resident(True)
        try:
            key = self.geometry_key() if self.reuse_geometry else None
            g = self._geometry
            if g is not None and g.key != key:
                self.release_geometry()
                g = None
            self.last_reused, self.last_weights_adopted = g is not None, False
            compensator = self._run_compensator()
            if g is None:
                g, imgs = self._geometry_pass(compensator)
                g.key = key
            else:
                # a panorama of a known rig: the images alone, into the kept rectangles (no ROI pass, no wait, no mask, no seam_resize)
                imgs, _, _ = self.warper.warp_images_and_masks(self.frames, self.cameras, self.camera_aspect, rects=g.rects,
                                                               compensator=compensator if g.gain_in_warp else None,
                                                               camera_arrays=self._cam_arrays, masks=False, tables=g.tables)
                if compensator is not None and not g.gain_in_warp:
                    imgs = compensator.apply_all(g.gain_corners, imgs, None, sub=g.gain_sub, ctx=self.ctx)
            if self.exposure_tracker is not None:  # the images are final: their statistics ride along, for the next run
                self.exposure_tracker._measure(imgs)
            self.last_crop = g.crop
            blender, g.blender = g.blender, None
            if blender is None:
                blender = Blender(self.blender_type, g.blend_strength, ctx=self.ctx)
                blender.prepare(g.prep_corners, g.prep_sizes)
            for img, mask, corner in zip(imgs, g.feed_masks, g.feed_corners):
                blender.feed(img, mask, corner)
            self.last_num_bands = blender.blender.num_bands()
            if key is not None and blender.blender.kind == _lib.BLEND_MULTIBAND:
                if not self.last_reused:
                    g.weights = blender.blender.keep_weights()  # filled by blend(); None where the blender does not qualify
                elif g.weights is not None:
                    # all images or none: a blender that adopts nothing builds as ever
                    self.last_weights_adopted = blender.blender.use_weights(g.weights)
            pano, pmask = blender.blend()
            if key is not None:
                self._geometry = g
        finally:
            config.set_device_resident(prev)
        return pano, pmask

    def _geometry_pass(self, compensator):
        """The first run of a rig (every run of a job that keeps nothing): ROI pass, warps WITH masks, the masks' way to the blender.
        -> (_RigGeometry, warped images).  The one piece of code that decides rectangles, feed corners and feed masks, for the plain path,
        the seam-cell crops and a cropper alike.  compensator: the run's (_run_compensator)."""
        # one ROI pass (the reference's eager Warper.warp_rois, stitching/stitcher.py:188), batched: one device pass, one wait.  It is the
        # ONE point where the host waits for the device and the device then waits for the host: without seam-cell crops (which need the
        # ROIs before the warps) pass and warps are one native call, and everything Python does with the ROIs happens behind the warp
        # launch (profiles/r05_latency.md)
        g = _RigGeometry()
        if self.cropper is not None:
            return self._geometry_pass_cropped(g, compensator)
        warped = None
        if self._mask_cols is None:
            warped = self.warper.warp_images_and_masks(self.frames, self.cameras, self.camera_aspect, compensator=compensator,
                                                       with_rois=True, camera_arrays=self._cam_arrays,
                                                       tables=g.tables if self.reuse_geometry else None)
            self._adopt([r[0:2] for r in warped[2]], [r[2:4] for r in warped[2]])
        else:
            self.plan()
        g.blender = Blender(self.blender_type, self.blend_strength, ctx=self.ctx)
        g.blender.prepare(self.corners, self.warped_sizes)
        crop = None
        if self._mask_cols is not None and g.blender.blender.kind == _lib.BLEND_MULTIBAND:
            crop = self._crop_rects(g.blender.blender, self.corners, self.warped_sizes)
        if crop is not None:
            box = [c if c is not None else (0, w, 0, h) for c, (w, h) in zip(crop, self.warped_sizes)]
            rects = [(cx + x0, cy + y0, x1 - x0, y1 - y0) for (x0, x1, y0, y1), (cx, cy) in zip(box, self.corners)]
            imgs, masks, rois = self.warper.warp_images_and_masks(self.frames, self.cameras, self.camera_aspect, rects=rects,
                                                                  compensator=compensator, camera_arrays=self._cam_arrays,
                                                                  tables=g.tables if self.reuse_geometry else None)
            self._track_rig(rects, masks)
            if self.feed_masks is not None:
                masks = [m[y0:y1, x0:x1] for m, (x0, x1, y0, y1) in zip(self.feed_masks, box)]
            else:
                masks = SeamFinder.resize_all(self.seam_masks, masks,
                                              sub=[(w, h, x0, y0) for (x0, x1, y0, y1), (w, h) in zip(box, self.warped_sizes)])
            corners = [(r[0], r[1]) for r in rects]
        else:
            imgs, masks, rois = warped or self.warper.warp_images_and_masks(self.frames, self.cameras, self.camera_aspect,
                                                                            compensator=compensator, camera_arrays=self._cam_arrays)
            self._track_rig(rois, masks)
            if self.feed_masks is not None:
                masks = self.feed_masks
            elif self.seam_masks is not None:
                masks = SeamFinder.resize_all(self.seam_masks, masks)
            corners = self.corners
            for roi, corner in zip(rois, self.corners):
                if roi[0:2] != tuple(corner):
                    raise StitchingError("warp roi changed between plan() and run()")
            rects = [(cx, cy, w, h) for (cx, cy), (w, h) in zip(self.corners, self.warped_sizes)]
        g.rects, g.crop = [tuple(int(v) for v in r) for r in rects], crop
        g.prep_corners, g.prep_sizes, g.blend_strength = list(self.corners), list(self.warped_sizes), self.blend_strength
        g.feed_corners, g.feed_masks = list(corners), list(masks)
        return g, imgs

    def _track_rig(self, rects, masks):
        """right behind the warp that returned masks: a tracker's lattice grids of these rectangles and warped masks"""
        if self.exposure_tracker is not None:
            self.exposure_tracker._create(self.ctx, [tuple(int(v) for v in r) for r in rects], masks)

    def _geometry_pass_cropped(self, g, compensator):
        """_geometry_pass with a cropper (device residency is on): the ROI pass first, then only the cropper's rectangle of every image —
        and inside it, with host seam masks and the multi-band blender, only what the seam cell can reach (view_rects)."""
        self.plan()
        cuts = [clip_rectangle(r.times(self.crop_aspect), w, h) for r, (w, h) in zip(self.cropper.intersection_rectangles, self.warped_sizes)]
        cut_sizes = [(x1 - x0, y1 - y0) for x0, x1, y0, y1 in cuts]
        if any(w <= 0 or h <= 0 for w, h in cut_sizes):
            raise StitchingError(f"the cropper leaves nothing of a warped image (sizes {cut_sizes}): it was prepared for another panorama")
        # what the reference prepares its blender on (crop_rois); the images it feeds are the slices above, which rounding may leave a
        # pixel larger or smaller
        corners, sizes = self.cropper.crop_rois(self.corners, self.warped_sizes, self.crop_aspect)
        corners, sizes = [tuple(c) for c in corners], [tuple(z) for z in sizes]
        roi = Blender.result_roi(corners, sizes)
        if self.num_bands is not None:
            self.blend_strength = blend_strength_for_bands(self.num_bands, roi[2], roi[3])
        # the reference's order: warp, then Blender.prepare (stitching/stitcher.py:118-126).  What the seam-cell crops need of the
        # blender beforehand is its geometry alone: a blender without a device (view_rects)
        crop = None
        kind, bands, _ = Blender.plan(self.blender_type, self.blend_strength, roi)
        if self._mask_cols is not None and kind == _lib.BLEND_MULTIBAND and cut_sizes == sizes:
            from .distributed import make_shard_blender

            crop = self._crop_rects(make_shard_blender(None, roi, bands), corners, sizes)
        box = [c if crop is not None and c is not None else (0, w, 0, h) for c, (w, h) in zip(crop or [None] * len(cuts), cut_sizes)]
        rects = [(cx + c[0] + x0, cy + c[2] + y0, x1 - x0, y1 - y0) for (x0, x1, y0, y1), c, (cx, cy) in zip(box, cuts, self.corners)]
        imgs, masks, _ = self.warper.warp_images_and_masks(self.frames, self.cameras, self.camera_aspect, rects=rects,
                                                           camera_arrays=self._cam_arrays)
        self._track_rig(rects, masks)
        sub = None if crop is None else [(w, h, x0, y0) for (x0, x1, y0, y1), (w, h) in zip(box, cut_sizes)]
        if compensator is not None:  # over the CROPPED image (apply on a crop); a seam-cell rectangle carries its offset in it
            imgs = compensator.apply_all(corners, imgs, None, sub=sub, ctx=self.ctx)
        if self.feed_masks is not None:
            masks = [m if b == (0, m.width, 0, m.height) else m[b[2]:b[3], b[0]:b[1]] for m, b in zip(self.feed_masks, box)]
        elif self.seam_masks is not None:
            masks = SeamFinder.resize_all(self.seam_masks, masks, sub=sub)
        g.rects, g.crop = [tuple(int(v) for v in r) for r in rects], crop
        g.gain_in_warp, g.gain_corners, g.gain_sub = False, corners, sub
        g.prep_corners, g.prep_sizes, g.blend_strength = corners, sizes, self.blend_strength
        g.feed_corners, g.feed_masks = [(cx + b[0], cy + b[2]) for (cx, cy), b in zip(corners, box)], list(masks)
        return g, imgs


def _seam_mask_input(m):
    """A low-resolution seam mask as StitchJob takes it: a foreign device array as it is (as_device copies it on the device), anything
    else as a host array."""
    return m if is_foreign_device_array(m) else np.asarray(m.get() if hasattr(m, "get") else m)


LENS_MODES = ("rectify", "fused")


def check_lens_mode(lens_mode, lenses):
    """lens_mode= of compose and Composer -> True for "fused"; any other string than LENS_MODES, and "fused" without lenses, is refused"""
    if lens_mode not in LENS_MODES:
        raise StitchingError(f"lens_mode {lens_mode!r}: one of {list(LENS_MODES)}")
    if lens_mode == "fused" and lenses is None:
        raise StitchingError("lens_mode=\"fused\" needs lenses: it warps distorted frames through them")
    return lens_mode == "fused"


def check_final_size(final_megapix, sizes):
    """lens_mode="fused": a final_megapix that resizes the (rectified) frames of `sizes` is refused — the lens belongs to the frame's
    own size.  The scale is the first frame's, as Images sets it."""
    scaler = MegapixDownscaler(final_megapix)
    scaler.set_scale_by_img_size(sizes[0])
    scaled = [scaler.get_scaled_img_size(z) for z in sizes]
    if scaled != [tuple(z) for z in sizes]:
        raise StitchingError(f"lens_mode=\"fused\" with final_megapix={final_megapix}: the frames would be resized to {scaled}, and a "
                             "lens belongs to the frame's own size")


def compose(frames, cameras, warper_type="spherical", blender_type="multiband", blend_strength=Blender.DEFAULT_BLEND_STRENGTH,
            compensator=None, seam_masks=None, ctx=None, cropper=None, crop_aspect=1, camera_aspect=1, source_masks=None, lenses=None,
            lens_mode="rectify"):
    """The final-resolution half of Stitcher.stitch (stitching/stitcher.py:117-128) with every intermediate in HBM:

        warp_final_resolution_imgs / masks   (:119-121, Warper)            -> one batched warp
        compensate_exposure_errors           (:123, ExposureErrorCompensator.apply; gains from the low-res pass)
        resize_seam_masks                    (:124, SeamFinder.resize; seam masks from the low-res pass)
        blend_images + create_final_panorama (:126-128, Blender)

    `compensator`: an ExposureErrorCompensator with set_gains() done, or None; `seam_masks`: low-resolution seam
    masks (one per image, e.g. from cv2's seam finder), or None for the full warped masks.
    `cropper`: a prepared Cropper with `crop_aspect` its lir_aspect (or the pair of both): crop_final_resolution (:119-121) — only the
    cropper's rectangles are warped (StitchJob); compensator gains and seam masks then belong to the cropped images.
    `camera_aspect`: the size of the frames relative to the images the cameras were estimated on.
    `source_masks`: one validity mask per frame (or None entries), see StitchJob.
    `lenses`: one LensMap per frame, or one for all: the frames are distorted.  `lens_mode` "rectify" (the default) rectifies them first
    (rectify_all); "fused" takes them to the panorama in one resampling (StitchJob(lenses=)) — other pixels than
    "rectify", the same masks.  Cameras and source_masks belong to the rectified frames either way.
    Returns device-resident (panorama u8x3, mask u8)."""
    fused = check_lens_mode(lens_mode, lenses)
    ctx = ctx or get_context()
    cropper, crop_aspect = _split_cropper(cropper, crop_aspect)
    if fused:
        if seam_masks is not None and blender_type == "multiband":
            seam_masks = [_seam_mask_input(m) for m in seam_masks]
        return StitchJob(frames, cameras, warper_type=warper_type, blender_type=blender_type, blend_strength=blend_strength, ctx=ctx,
                         seam_masks=seam_masks, compensator=compensator, cropper=cropper, crop_aspect=crop_aspect,
                         camera_aspect=camera_aspect, source_masks=source_masks, lenses=lenses).run()
    if lenses is not None:
        frames = rectify_all(frames, lenses, ctx=ctx)
    if cropper is not None:
        if seam_masks is not None and blender_type == "multiband":
            seam_masks = [_seam_mask_input(m) for m in seam_masks]
        return StitchJob(frames, cameras, warper_type=warper_type, blender_type=blender_type, blend_strength=blend_strength, ctx=ctx,
                         seam_masks=seam_masks, compensator=compensator, cropper=cropper, crop_aspect=crop_aspect,
                         camera_aspect=camera_aspect, source_masks=source_masks).run()
    if seam_masks is not None and blender_type == "multiband":
        # nothing between the warp and the blender needs whole images (the gain of a pixel depends on its position alone): warp,
        # compensate and feed only what the seam cells can reach
        return StitchJob(frames, cameras, warper_type=warper_type, blender_type=blender_type, blend_strength=blend_strength, ctx=ctx,
                         seam_masks=[_seam_mask_input(m) for m in seam_masks], compensator=compensator,
                         camera_aspect=camera_aspect, source_masks=source_masks).run()
    prev = config.device_resident()
    config.set_device_resident(True)
    try:
        warper = Warper(warper_type, ctx=ctx)
        warper.set_scale(cameras)
        imgs, masks, rois = warper.warp_images_and_masks([as_device(f, ctx) for f in frames], cameras, camera_aspect, compensator=compensator,
                                                         source_masks=source_masks)
        corners, sizes = [r[0:2] for r in rois], [r[2:4] for r in rois]
        if seam_masks is not None:
            masks = SeamFinder.resize_all(seam_masks, masks)
        blender = Blender(blender_type, blend_strength, ctx=ctx)
        blender.prepare(corners, sizes)
        for img, mask, corner in zip(imgs, masks, corners):
            blender.feed(img, mask, corner)
        return blender.blend()
    finally:
        config.set_device_resident(prev)


class ComposePlan:
    """What the low-resolution half of a composition leaves (Composer.prepare), device-resident: the prepared cropper, the compensator
    with its gains, the low-resolution seam masks and the scales.  Valid for every set of frames of the same rig (same sizes, same
    cameras): Composer.run(plan, images=new_frames).  The plan also carries the StitchJob of its final-resolution half, which keeps the
    rig's masks and weight pyramids between runs (StitchJob's memory note; `plan.job.release_geometry()` gives them back)."""

    def __init__(self, images, frames, cameras, warper_scale, cropper, compensator, seam_masks, seam_masks_host, low_corners, low_sizes,
                 source_masks=None, distorted=None, lenses=None, exposure_tracker=None):
        self.exposure_tracker = exposure_tracker  # Composer.prepare(exposure_tracker=): handed to the plan's StitchJob
        self.images, self.frames, self.cameras, self.warper_scale = images, frames, list(cameras), warper_scale
        # lens_mode="fused": the distorted frames the plan was prepared from and their lenses (`frames` are their rectified forms, which
        # the low-resolution pass read); None, None otherwise
        self.distorted, self.lenses = distorted, lenses
        self.source_masks = source_masks  # the frames' validity masks at the frames' size (device; OwnedMasks where they are the plan's own), or None
        self.cropper, self.compensator, self.seam_masks, self.seam_masks_host = cropper, compensator, seam_masks, seam_masks_host
        self.low_corners, self.low_sizes = low_corners, low_sizes
        self.frame_sizes = images.sizes
        self.job = self.job_key = None  # Composer.run's StitchJob for this plan: the rig's geometry is made once (StitchJob)
        R = Images.Resolution
        self.camera_aspect = images.get_ratio(R.MEDIUM, R.FINAL)
        self.lir_aspect = images.get_ratio(R.LOW, R.FINAL)

    def check_frames(self, frames, lenses=None):
        """frames: what the final-resolution half is given.  With lenses (one LensMap per frame) they are distorted frames: each must
        have its lens's source size, and each lens must rectify to the size the plan was prepared for."""
        if lenses is not None:
            got = [Images.get_image_size(f) for f in frames]
            if got != [lens.src_size for lens in lenses]:
                raise StitchingError(f"the lenses were made for frames of sizes {[lens.src_size for lens in lenses]}, got {got}")
            if [lens.dst_size for lens in lenses] != [tuple(z) for z in self.frame_sizes]:
                raise StitchingError(f"the plan was prepared for frames of sizes {self.frame_sizes}, the lenses rectify to "
                                     f"{[lens.dst_size for lens in lenses]}: same rig, same sizes")
            return
        got = [Images.get_image_size(f) for f in frames]
        if got != [tuple(z) for z in self.frame_sizes]:
            raise StitchingError(f"the plan was prepared for frames of sizes {self.frame_sizes}, got {got}: same rig, same sizes")


class Composer:
    """Cameras in, panorama out: both halves of Stitcher.stitch after estimate_scale (stitching/stitcher.py:106-128) with every
    intermediate in HBM.  `prepare` is the low-resolution half (:108-115: resize to LOW, warp, Cropper.prepare and crop,
    ExposureErrorCompensator.feed, SeamFinder.find), `run` the final one (:117-128, a StitchJob), `compose` both.  The keywords are the
    reference's Stitcher.DEFAULT_SETTINGS where they apply; `cameras` are at MEDIUM scale, as the reference's registration leaves them.
    Exposure gains and the "voronoi" / "no" seams are estimated on the device whatever the process-wide estimator settings are (nothing
    imports cv2); the "dp_*" and "gc_*" finders are cv2's, through SeamFinder; a finder object given as seam_estimator= (the project's
    own colour-aware ColorSeamEstimator, say) takes their place without cv2.  The subset step (Images.subset) is the caller's: pass
    the images registration kept.  `stitch` starts from the frames alone: it registers them with the project's own estimators
    (FeatureEstimator, MatchEstimator, CameraSolver) and composes the images those kept."""

    DEFAULT_SETTINGS = {
        "medium_megapix": Images.Resolution.MEDIUM.value,
        "warper_type": Warper.DEFAULT_WARP_TYPE,
        "low_megapix": Images.Resolution.LOW.value,
        "crop": Cropper.DEFAULT_CROP,
        "compensator": ExposureErrorCompensator.DEFAULT_COMPENSATOR,
        "nr_feeds": ExposureErrorCompensator.DEFAULT_NR_FEEDS,
        "block_size": ExposureErrorCompensator.DEFAULT_BLOCK_SIZE,
        "finder": SeamFinder.DEFAULT_SEAM_FINDER,
        "final_megapix": Images.Resolution.FINAL.value,
        "blender_type": Blender.DEFAULT_BLENDER,
        "blend_strength": Blender.DEFAULT_BLEND_STRENGTH,
    }

    REGISTRATION_MODELS = ("homography", "rotation")  # of the MatchEstimator and the CameraSolver that stitch() makes where none is given

    def __init__(self, ctx=None, seam_estimator=None, **kwargs):
        """seam_estimator (not a setting): a finder object with find(imgs, corners, masks), e.g. a ColorSeamEstimator — `prepare` then finds
        its seams with it whatever "finder" names, and never looks for cv2."""
        self.seam_estimator = seam_estimator
        self.registration = None  # of the last stitch(): indices of the images kept, their cameras, the solver's info
        for arg in kwargs:
            if arg not in self.DEFAULT_SETTINGS:
                raise StitchingError("Invalid Argument: " + arg)
        self.settings = dict(self.DEFAULT_SETTINGS, **kwargs)
        self.ctx = ctx
        st = self.settings
        if st["finder"] not in SeamFinder.SEAM_FINDER_CHOICES:
            raise StitchingError(f"unknown seam finder {st['finder']!r}")
        if st["compensator"] not in ExposureErrorCompensator.COMPENSATOR_CHOICES:
            raise StitchingError(f"unknown compensator {st['compensator']!r}")
        if st["warper_type"] not in Warper.WARP_TYPE_CHOICES:
            raise StitchingError(f"unknown warper type {st['warper_type']!r}")
        if st["blender_type"] not in Blender.BLENDER_CHOICES:
            raise StitchingError(f"unknown blender type {st['blender_type']!r}")
        if st["medium_megapix"] < st["low_megapix"]:
            raise StitchingError("Medium resolution megapix need to be greater or equal than low resolution megapix")

    def _ctx(self):
        return self.ctx or get_context()

    @staticmethod
    def _source_masks(source_masks, n, ctx, lens_masks=None):
        """source_masks= of prepare / stitch -> None, or the device masks (None entries: no mask): OwnedMasks where they are the
        library's own copies (host arrays uploaded here, a lens's masks), a plain list where a caller's device array is among them"""
        if source_masks is None:
            return None
        if isinstance(source_masks, str):
            if source_masks != "lens":
                raise StitchingError(f"source_masks={source_masks!r}: a list of masks, or \"lens\"")
            if lens_masks is None:
                raise StitchingError("source_masks=\"lens\" needs lenses: the masks are those of the rectification")
            return OwnedMasks(lens_masks)
        source_masks = list(source_masks)
        if len(source_masks) != n:
            raise StitchingError(f"{len(source_masks)} source masks for {n} images")
        own = masks_belong_to_job(None, None, source_masks)
        dev = [None if m is None else as_device(m, ctx) for m in source_masks]
        return OwnedMasks(dev) if own else dev

    @staticmethod
    def _shrunk(source_masks, sizes):
        """the masks at `sizes` (w, h): conservatively shrunk where a size is smaller than its mask, the mask itself where it is equal"""
        todo = [i for i, (m, z) in enumerate(zip(source_masks, sizes)) if m is not None and (m.width, m.height) != tuple(z)]
        out = list(source_masks)
        if todo:
            for i, m in zip(todo, shrink_masks_all([source_masks[i] for i in todo], [sizes[i] for i in todo])):
                out[i] = m
        return OwnedMasks(out) if isinstance(source_masks, OwnedMasks) else out

    def prepare(self, images, cameras, lenses=None, source_masks=None, lens_mode="rectify", exposure_tracker=None):
        """The low-resolution half -> ComposePlan.  The host waits for the device where a result decides what is launched next: the ROI
        pass of the warp, the cropper's rectangle, the gain solve (and the read-back of the seam masks for the multi-band blender's
        seam-cell crops).  lenses: one LensMap per image, or one for all — the images are then distorted frames and are rectified
        first (stitching_amd.rectify); the plan is prepared from, and keeps, the rectified frames.
        source_masks: one validity mask per image at the image's size (of the RECTIFIED image with lenses; None entries: none), or
        "lens" (needs lenses): the masks of the rectification itself, which keep a lens's black wedges out of the panorama.  The
        masks are shrunk conservatively to the LOW size and ride on the low-resolution frames, so that the cropper, the gain
        estimation and the seam finder see them through the warped masks; the plan keeps them for the final-resolution half.  A user's
        masks and a lens's are not combined.
        lens_mode: "rectify" (the default): as above.  "fused" (needs lenses): the low-resolution pass still reads rectified frames —
        it runs once per rig — but the plan keeps the DISTORTED frames and the lenses, and `run` warps through the lens (StitchJob with
        lenses).  Refused with a final_megapix that resizes the frames: a lens belongs to the frame's own size.
        exposure_tracker: an ExposureTracker kept on the plan: `run` gives it to the plan's StitchJob, whose runs then follow the
        cameras' exposure from frame to frame on top of the gains estimated here.  `compose` and `stitch` make
        one panorama and take none."""
        if exposure_tracker is not None:
            from .exposure_tracking import ExposureTracker

            if not isinstance(exposure_tracker, ExposureTracker):
                raise StitchingError(f"exposure_tracker= takes an ExposureTracker, got {type(exposure_tracker).__name__}")
        frames, cameras = list(images), list(cameras)
        fused = check_lens_mode(lens_mode, lenses)
        distorted = frames if fused else None
        if lenses is not None:
            lenses = lens_list(lenses, len(frames))
        if fused:
            check_final_size(self.settings["final_megapix"], [lens.dst_size for lens in lenses])
        st, ctx = self.settings, self._ctx()
        if len(frames) != len(cameras):
            raise StitchingError("need one camera per image")
        lens_masks = None
        if isinstance(source_masks, str) and source_masks == "lens" and lenses is not None:
            frames, lens_masks = rectify_all(frames, lenses, masks=True, ctx=ctx)
        elif lenses is not None:
            frames = rectify_all(frames, lenses, ctx=ctx)
        frames = [as_device(f, ctx) for f in frames]  # on THIS context: every later stage follows its images' context
        source_masks = self._source_masks(source_masks, len(frames), ctx, lens_masks)
        imgs_obj = Images.of(frames, st["medium_megapix"], st["low_megapix"], st["final_megapix"])
        R = Images.Resolution
        prev = config.device_resident()
        config.set_device_resident(True)
        try:
            medium = list(imgs_obj.resize(R.MEDIUM))
            low = list(imgs_obj.resize(R.LOW, medium))  # from the MEDIUM images, as stitcher.py:108 does
            warper = Warper(st["warper_type"], ctx=ctx)
            warper.set_scale(cameras)
            aspect = imgs_obj.get_ratio(R.MEDIUM, R.LOW)
            low_masks = None if source_masks is None else self._shrunk(source_masks, [(f.width, f.height) for f in low])
            imgs, masks, rois = warper.warp_images_and_masks(low, cameras, aspect, source_masks=low_masks)
            corners, sizes = [r[0:2] for r in rois], [r[2:4] for r in rois]
            cropper = Cropper(st["crop"])
            cropper.prepare(imgs, masks, corners, sizes)
            masks = list(cropper.crop_images(masks))
            imgs = list(cropper.crop_images(imgs))
            corners, sizes = cropper.crop_rois(corners, sizes)
            estimator = ExposureErrorCompensator._device_estimator(st["compensator"], st["nr_feeds"], st["block_size"])
            compensator = ExposureErrorCompensator(st["compensator"], st["nr_feeds"], st["block_size"], estimator=estimator)
            compensator.feed(corners, imgs, masks)
            if self.seam_estimator is not None:
                finder = SeamFinder(st["finder"], estimator=self.seam_estimator)
            else:
                device_finder = st["finder"] in DEVICE_SEAM_FINDERS
                finder = SeamFinder(st["finder"], estimator=SeamEstimator(st["finder"]) if device_finder else None)
            seam_masks = [as_device(m, ctx) for m in finder.find(imgs, corners, masks)]
            host = None
            if st["blender_type"] == "multiband":  # StitchJob's seam-cell crops read the masks' extents on the host
                host = [m.numpy() for m in seam_masks]
        finally:
            config.set_device_resident(prev)
        return ComposePlan(imgs_obj, frames, cameras, warper.scale, cropper, compensator, seam_masks, host, corners, sizes,
                           source_masks=source_masks, distorted=distorted, lenses=lenses if fused else None, exposure_tracker=exposure_tracker)

    def run(self, plan, images=None, lenses=None):
        """The final-resolution half on a plan: `images` None -> the frames the plan was prepared from, else new frames of the same rig
        (no low-resolution pass).  lenses: the LensMaps of new, distorted `images`, which are rectified first (the plan's own frames
        are rectified already).  A plan of lens_mode="fused" warps through the lens: its own distorted frames, or new distorted `images`
        with their `lenses`.  Returns device-resident (panorama u8x3, mask u8)."""
        if getattr(plan, "lenses", None) is not None:
            return self._run_fused(plan, images, lenses)
        if lenses is not None:
            if images is None:
                raise StitchingError("lenses go with new images: the frames the plan was prepared from are rectified already")
            images = list(images)
            lenses = lens_list(lenses, len(images))
            plan.check_frames(images, lenses)
            images = rectify_all(images, lenses, ctx=self._ctx())
        frames = plan.frames if images is None else list(images)
        plan.check_frames(frames)
        st, ctx = self.settings, self._ctx()
        frames = [as_device(f, ctx) for f in frames]
        prev = config.device_resident()
        config.set_device_resident(True)
        try:
            final = list(plan.images.resize(Images.Resolution.FINAL, frames))
        finally:
            config.set_device_resident(prev)
        # one job per plan: its second run warps pixels only (same rig, new frames)
        job_key = (id(ctx), st["warper_type"], st["blender_type"], st["blend_strength"])
        if plan.job is None or plan.job_key != job_key:
            if getattr(plan, "exposure_tracker", None) is not None:
                plan.job = None  # a tracker follows one job at a time: the old one goes first
            plan.job = StitchJob(final, plan.cameras, warper_type=st["warper_type"], blender_type=st["blender_type"],
                                 blend_strength=st["blend_strength"], ctx=ctx,
                                 seam_masks=plan.seam_masks_host if plan.seam_masks_host is not None else plan.seam_masks,
                                 compensator=plan.compensator, cropper=plan.cropper, crop_aspect=plan.lir_aspect,
                                 camera_aspect=plan.camera_aspect,
                                 source_masks=None if plan.source_masks is None else
                                 self._shrunk(plan.source_masks, [(f.width, f.height) for f in final]),
                                 exposure_tracker=getattr(plan, "exposure_tracker", None))
            plan.job_key = job_key
            return plan.job.run()
        return plan.job.run(frames=final)

    def _run_fused(self, plan, images, lenses):
        """`run` on a plan of lens_mode="fused": one StitchJob with lenses per plan and set of lenses"""
        if images is None:
            if lenses is not None:
                raise StitchingError("lenses go with new images: the plan has the lenses of its own frames")
            frames, lenses = plan.distorted, plan.lenses
        else:
            if lenses is None:
                raise StitchingError("a plan of lens_mode=\"fused\" takes distorted images with their lenses")
            frames = list(images)
            lenses = lens_list(lenses, len(frames))
            plan.check_frames(frames, lenses)
        st, ctx = self.settings, self._ctx()
        job_key = (id(ctx), st["warper_type"], st["blender_type"], st["blend_strength"], "fused", tuple(id(lens) for lens in lenses))
        if plan.job is None or plan.job_key != job_key:
            if getattr(plan, "exposure_tracker", None) is not None:
                plan.job = None  # a tracker follows one job at a time: the old one goes first
            plan.job = StitchJob(frames, plan.cameras, warper_type=st["warper_type"], blender_type=st["blender_type"],
                                 blend_strength=st["blend_strength"], ctx=ctx,
                                 seam_masks=plan.seam_masks_host if plan.seam_masks_host is not None else plan.seam_masks,
                                 compensator=plan.compensator, cropper=plan.cropper, crop_aspect=plan.lir_aspect,
                                 camera_aspect=plan.camera_aspect, source_masks=plan.source_masks, lenses=lenses,
                                 exposure_tracker=getattr(plan, "exposure_tracker", None))
            plan.job_key = job_key
            return plan.job.run()
        return plan.job.run(frames=frames)

    def compose(self, images, cameras, lenses=None, source_masks=None, lens_mode="rectify"):
        """prepare + run -> the panorama (device-resident u8x3), as Stitcher.stitch returns it; lenses, source_masks, lens_mode: see
        `prepare`"""
        pano, _ = self.run(self.prepare(images, cameras, lenses=lenses, source_masks=source_masks, lens_mode=lens_mode))
        return pano

    def stitch(self, images, feature_estimator=None, match_estimator=None, camera_solver=None, lenses=None, source_masks=None,
               lens_mode="rectify"):
        """Frames in, panorama out (device-resident u8x3), with no cv2 and no cameras supplied: the registration half of Stitcher.stitch
        (stitching/stitcher.py:99-105) by the project's own estimators — resize to MEDIUM on the device, FeatureEstimator.detect,
        MatchEstimator.match, CameraSolver.register — then `compose` on the images registration kept.  The three objects default to
        their classes' defaults.  `self.registration` keeps the indices of the images kept, their cameras and the solver's info.
        lenses: one LensMap per image, or one for all: registration and composition then see the rectified frames.
        source_masks: as in `prepare`; shrunk to the MEDIUM size they also keep the feature detector off what is not picture.
        lens_mode: as in `prepare`; registration reads the rectified frames either way."""
        from .camera_estimation import CameraSolver
        from .feature_estimation import FeatureEstimator
        from .match_estimation import MatchEstimator

        fused = check_lens_mode(lens_mode, lenses)
        distorted = list(images) if fused else None
        if lenses is not None:
            images = list(images)
            lenses = lens_list(lenses, len(images))
        st, ctx = self.settings, self._ctx()
        lens_masks = None
        if isinstance(source_masks, str) and source_masks == "lens" and lenses is not None:
            images, lens_masks = rectify_all(images, lenses, masks=True, ctx=ctx)
        elif lenses is not None:
            images = rectify_all(images, lenses, ctx=ctx)
        frames = [as_device(f, ctx) for f in images]
        source_masks = self._source_masks(source_masks, len(frames), ctx, lens_masks)
        if len(frames) < 2:
            raise StitchingError("stitching needs at least two images")
        feature_estimator = feature_estimator or FeatureEstimator()
        match_estimator = match_estimator or MatchEstimator(model=self.REGISTRATION_MODELS[0])
        camera_solver = camera_solver or CameraSolver(model=self.REGISTRATION_MODELS[1])
        imgs_obj = Images.of(frames, st["medium_megapix"], st["low_megapix"], st["final_megapix"])
        prev = config.device_resident()
        config.set_device_resident(True)
        try:
            medium = list(imgs_obj.resize(Images.Resolution.MEDIUM))
        finally:
            config.set_device_resident(prev)
        if source_masks is None:
            features = feature_estimator.detect(medium)
        else:
            features = feature_estimator.detect(medium, self._shrunk(source_masks, [(f.width, f.height) for f in medium]))
        matches = match_estimator.match(features, ctx=ctx)
        indices, cameras = camera_solver.register(features, matches, ctx=ctx)
        self.registration = {"indices": list(indices), "cameras": cameras, "info": camera_solver.info}
        kept = None if source_masks is None else type(source_masks)(source_masks[i] for i in indices)
        if fused:  # the distorted frames registration kept, with their lenses (prepare rectifies them for its low-resolution pass)
            return self.compose([distorted[i] for i in indices], cameras, lenses=[lenses[i] for i in indices], source_masks=kept,
                                lens_mode="fused")
        return self.compose([frames[i] for i in indices], cameras, source_masks=kept)


class AffineComposer(Composer):
    """Composer for scans and flat tiles, as the reference's AffineStitcher is its Stitcher (stitching/stitcher.py:267-287): the affine
    warper and no exposure compensation by default, and `stitch` registers with the affine models of the project's own estimators —
    MatchEstimator(model="affine") and CameraSolver(model="affine"), whose cameras carry the 3 x 3 map from image pixels to the panorama
    plane in R (focal = 1, ppx = ppy = 0), with no wave correction.  DESIGN.md section 18."""

    # the reference's AFFINE_DEFAULTS that are settings of Composer (its matcher, estimator, adjuster and wave correction are
    # REGISTRATION_MODELS here)
    AFFINE_DEFAULTS = {"warper_type": "affine", "compensator": "no"}
    DEFAULT_SETTINGS = dict(Composer.DEFAULT_SETTINGS, **AFFINE_DEFAULTS)
    REGISTRATION_MODELS = ("affine", "affine")

    def __init__(self, ctx=None, seam_estimator=None, **kwargs):
        for key, value in kwargs.items():
            if key in self.AFFINE_DEFAULTS and value != self.AFFINE_DEFAULTS[key]:
                warnings.warn(f"You are overwriting an affine default ({key}={self.AFFINE_DEFAULTS[key]}) with another value ({value}). "
                              "Make sure this is intended", StitchingWarning)
        super().__init__(ctx=ctx, seam_estimator=seam_estimator, **kwargs)


def stitch(frames, cameras, **kw):
    """Convenience: numpy frames in, numpy panorama out (PCIe-inclusive path)."""
    job = StitchJob(frames, cameras, **kw)
    pano, mask = job.run()
    return np.asarray(pano), np.asarray(mask)
