"""Device context and device-resident images (host side of include/stitching_amd.h).

`DeviceImage` stands where the reference hands numpy arrays / cv.UMat across the cv2
boundary (stitching/blender.py:41, stitching/warper.py:45-51): it exposes `.shape`,
`.dtype`, `__array__` (host copy on demand) and rectangular slicing
(stitching/cropper.py:150-151) while the pixels stay in HBM.
"""
import ctypes as C
import os
import threading

import numpy as np

from . import _lib
from .stitching_error import StitchingError

_DTYPES = {_lib.U8: np.uint8, _lib.S16: np.int16, _lib.F32: np.float32}
_ELEMS = {np.dtype(np.uint8): _lib.U8, np.dtype(np.int16): _lib.S16, np.dtype(np.float32): _lib.F32}


class Context:
    """One per (process, GPU): owns the HIP stream and the caching allocator."""

    def __init__(self, device=0):
        self._lib = _lib.lib()
        h = C.c_void_p()
        _lib.check(self._lib.stx_ctx_create(int(device), C.byref(h)))
        self.handle = h
        self.device = int(device)

    def sync(self):
        _lib.check(self._lib.stx_ctx_sync(self.handle))

    # ---- measurement hooks (bench.py)
    def prof_enable(self, on=True):
        _lib.check(self._lib.stx_prof_enable(self.handle, 1 if on else 0))

    def prof_reset(self):
        _lib.check(self._lib.stx_prof_reset(self.handle))

    def prof_results(self):
        n = C.c_int()
        _lib.check(self._lib.stx_prof_count(self.handle, C.byref(n)))
        out = []
        for i in range(n.value):
            name = C.create_string_buffer(64)
            calls, ms, by = C.c_int64(), C.c_double(), C.c_double()
            _lib.check(self._lib.stx_prof_get(self.handle, i, name, 64, C.byref(calls), C.byref(ms), C.byref(by)))
            out.append({"kernel": name.value.decode(), "calls": calls.value, "total_ms": ms.value,
                        "algo_bytes": by.value})
        return out

    def mark(self, slot):
        _lib.check(self._lib.stx_mark(self.handle, int(slot)))

    def elapsed_ms(self, a, b):
        ms = C.c_double()
        _lib.check(self._lib.stx_mark_elapsed_ms(self.handle, int(a), int(b), C.byref(ms)))
        return ms.value

    def close(self):
        if self.handle:
            self._lib.stx_ctx_destroy(self.handle)
            self.handle = None


_ctx_lock = threading.Lock()
_contexts = {}
_default_device = None


def device_count():
    n = C.c_int()
    _lib.check(_lib.lib().stx_device_count(C.byref(n)))
    return n.value


def set_default_device(device):
    global _default_device
    _default_device = int(device)


def get_context(device=None):
    """Process-wide context for `device` (default: STITCHING_AMD_DEVICE, else LOCAL_RANK, else 0)."""
    global _default_device
    if device is None:
        if _default_device is None:
            _default_device = int(os.environ.get("STITCHING_AMD_DEVICE", os.environ.get("LOCAL_RANK", "0")))
        device = _default_device
    with _ctx_lock:
        ctx = _contexts.get(device)
        if ctx is None:
            ctx = _contexts[device] = Context(device)
        return ctx


class _PinnedBlock:
    """Owns one page-locked host allocation and exposes it through the array interface: numpy arrays made from it
    keep it alive as their .base."""

    def __init__(self, nbytes):
        self._lib = _lib.lib()
        p = C.c_void_p()
        _lib.check(self._lib.stx_host_alloc(int(nbytes), C.byref(p)))
        self.ptr = p
        self.__array_interface__ = {"shape": (int(nbytes),), "typestr": "|u1", "data": (p.value, False), "version": 3}

    def __del__(self):
        try:
            if self.ptr:
                self._lib.stx_host_free(self.ptr)
                self.ptr = None
        except Exception:
            pass


def pinned_empty(shape, dtype=np.uint8):
    """numpy array in page-locked host memory: decode frames into it (or np.copyto) and the upload in
    Warper.warp_image / DeviceImage.from_numpy runs at PCIe rate; DeviceImage.numpy(out=such an array) likewise."""
    dt = np.dtype(dtype)
    count = int(np.prod(shape))
    raw = np.asarray(_PinnedBlock(max(count * dt.itemsize, 1)))
    return raw[:count * dt.itemsize].view(dt).reshape(shape)


class DeviceImage:
    """A 2-D image in HBM (u8 / int16 / fp32, 1..4 interleaved channels)."""

    __array_priority__ = 100

    def __init__(self, ctx, handle):
        self.ctx = ctx
        self._h = handle
        info = (C.c_int64 * 6)()
        _lib.check(ctx._lib.stx_buf_info(handle, info))
        self.width, self.height, self.channels, self._elem = int(info[0]), int(info[1]), int(info[2]), int(info[3])
        self.stride_bytes = int(info[4])

    # ---- construction
    @classmethod
    def from_numpy(cls, arr, ctx=None, wait=True):
        """Upload.  wait=False: `arr` is page-locked (pinned_empty) and stays untouched until ctx.sync(); the copy is only
        queued (pageable arrays are copied synchronously either way)."""
        ctx = ctx or get_context()
        a = np.asarray(arr)
        if a.ndim == 2:
            h, w, c = a.shape[0], a.shape[1], 1
        elif a.ndim == 3:
            h, w, c = a.shape
        else:
            raise StitchingError(f"expected an HxW or HxWxC image, got shape {a.shape}")
        if a.dtype not in _ELEMS:
            raise StitchingError(f"unsupported image dtype {a.dtype}")
        if h == 0 or w == 0:
            raise StitchingError("empty image")
        if not a.flags["C_CONTIGUOUS"]:
            a = np.ascontiguousarray(a)
        out = C.c_void_p()
        if not wait and a is not arr and not np.shares_memory(a, arr):
            wait = True  # a temporary copy was made above: it must not be freed under the queued transfer
        fn = ctx._lib.stx_buf_from_host if wait else ctx._lib.stx_buf_from_host_async
        _lib.check(fn(ctx.handle, a.ctypes.data_as(C.c_void_p), a.strides[0], w, h, c, _ELEMS[a.dtype], C.byref(out)))
        return cls(ctx, out)

    @classmethod
    def from_device(cls, obj, format=None, matrix="bt709", range="limited", stream=None, wait=True, ctx=None):
        """A foreign device frame (an object with `__cuda_array_interface__`, or the tuple of planes of nv12 / i420) -> a new image of
        the library's own, copied or converted on the device: `stitching_amd.ingest.ingest`."""
        from .ingest import ingest

        return ingest(obj, format=format, matrix=matrix, range=range, stream=stream, wait=wait, ctx=ctx)

    # ---- numpy-like surface
    @property
    def shape(self):
        return (self.height, self.width) if self.channels == 1 else (self.height, self.width, self.channels)

    @property
    def dtype(self):
        return np.dtype(_DTYPES[self._elem])

    @property
    def ndim(self):
        return 2 if self.channels == 1 else 3

    @property
    def size(self):
        return self.height * self.width * self.channels

    def numpy(self, out=None, wait=True):
        """Host copy; `out`: a C-contiguous array of this shape / dtype to copy into (e.g. from pinned_empty).
        wait=False (needs a page-locked `out`): the read-back is only queued; `out` is valid after ctx.sync()."""
        if out is None:
            out = np.empty(self.shape, self.dtype)
            wait = True
        elif out.shape != self.shape or out.dtype != self.dtype or not out.flags.c_contiguous:
            raise StitchingError(f"out must be a C-contiguous {self.dtype} array of shape {self.shape}")
        fn = self.ctx._lib.stx_buf_to_host if wait else self.ctx._lib.stx_buf_to_host_async
        _lib.check(fn(self._h, out.ctypes.data_as(C.c_void_p), out.strides[0]))
        return out

    def __array__(self, dtype=None, copy=None):
        a = self.numpy()
        return a if dtype is None else a.astype(dtype, copy=False)

    def __len__(self):
        return self.height

    def __getitem__(self, key):
        """Rectangular, unit-step slicing on (y, x) returns a device view (no copy)."""
        if not isinstance(key, tuple):
            key = (key,)
        if len(key) > 2 and not (len(key) == 3 and key[2] == slice(None)):
            return self.numpy()[key]
        ys = key[0] if len(key) > 0 else slice(None)
        xs = key[1] if len(key) > 1 else slice(None)
        if not isinstance(ys, slice) or not isinstance(xs, slice):
            return self.numpy()[key]
        y0, y1, ystep = ys.indices(self.height)
        x0, x1, xstep = xs.indices(self.width)
        if ystep != 1 or xstep != 1 or y1 <= y0 or x1 <= x0:
            return self.numpy()[key]
        out = C.c_void_p()
        _lib.check(self.ctx._lib.stx_buf_view(self._h, x0, y0, x1 - x0, y1 - y0, C.byref(out)))
        return DeviceImage(self.ctx, out)

    @property
    def validity(self):
        """The validity mask this frame carries (with_validity), as a DeviceImage on the same bytes, or None."""
        out = C.c_void_p()
        _lib.check(self.ctx._lib.stx_buf_validity(self._h, C.byref(out)))
        return DeviceImage(self.ctx, out) if out.value else None

    def device_ptr(self):
        p = C.c_void_p()
        _lib.check(self.ctx._lib.stx_buf_device_ptr(self._h, C.byref(p)))
        return p.value

    @property
    def __cuda_array_interface__(self):
        """The image's memory for a GPU encoder or another framework (version 3), without a copy.  Shape and strides are the image's
        own: rows are padded, and a crop view is exported with its parent's pitch.  The getter syncs the context, so the bytes are
        complete and `stream` is None.  This object stays the owner: the consumer must keep it alive for as long as it uses the
        memory.  The memory is handed out writable because some consumers refuse read-only arrays — but an image may be shared: the
        panorama mask of a known rig is one buffer handed out by every run, and must be copied before it is written."""
        self.ctx.sync()
        size = self.dtype.itemsize
        strides = (self.stride_bytes, size) if self.channels == 1 else (self.stride_bytes, self.channels * size, size)
        return {"version": 3, "shape": self.shape, "typestr": self.dtype.str if size > 1 else "|u1", "strides": strides,
                "data": (self.device_ptr(), False), "stream": None}

    def free(self):
        if self._h is not None:
            if self.ctx.handle:  # a closed context has already returned all of its device memory
                self.ctx._lib.stx_buf_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def __repr__(self):
        return f"DeviceImage(shape={self.shape}, dtype={self.dtype}, device={self.ctx.device})"


def with_validity(frame, mask, ctx=None):
    """`frame` (HxWx3 uint8) with the validity mask `mask` (HxW uint8: non-zero = picture) attached: a new DeviceImage onto the same
    pixels (stx_buf_with_validity) whose `.validity` is the mask.  Warper.warp_images_and_masks / warp_image_and_mask, StitchJob and
    Composer then produce warped masks that are the nearest-neighbour warp of `mask` instead of a warped rectangle; everything else
    reads the pixels and ignores the mask.  Host arrays are uploaded (masks of 0 / 255 are recognised as binary on the way), foreign
    device arrays are copied on the device (as_device); slicing the result keeps the matching slice of the mask.  `frame` itself is
    not changed."""
    f = as_device(frame, ctx)
    m = as_device(mask, f.ctx)
    out = C.c_void_p()
    _lib.check(f.ctx._lib.stx_buf_with_validity(f._h, m._h, C.byref(out)))
    return DeviceImage(f.ctx, out)


def shrink_masks_all(masks, sizes, ctx=None):
    """Validity masks at a lower resolution, conservatively: pixel (x, y) of a (w, h) result is 255 where EVERY pixel of the mask in
    columns [x sw // w, ((x + 1) sw + w - 1) // w) and the rows likewise is non-zero, else 0 (stx_mask_shrink_batch: one launch for the
    list).  sizes: (w, h) per mask, none larger than its mask; equal sizes binarise.  Returns DeviceImages."""
    masks = [as_device(m, ctx) for m in masks]
    sizes = [(int(s[0]), int(s[1])) for s in sizes]
    if len(masks) != len(sizes):
        raise StitchingError(f"{len(masks)} masks and {len(sizes)} sizes")
    n = len(masks)
    if n == 0:
        return []
    c = masks[0].ctx
    wh = (C.c_int * (2 * n))(*[v for s in sizes for v in s])
    h_src, h_out = (C.c_void_p * n)(*[m._h for m in masks]), (C.c_void_p * n)()
    _lib.check(c._lib.stx_mask_shrink_batch(c.handle, n, h_src, wh, h_out))
    return [DeviceImage(c, C.c_void_p(h_out[i])) for i in range(n)]


def is_foreign_device_array(a):
    """An object of another framework that holds device memory (`__cuda_array_interface__`): as_device copies it on the device, so
    it must not be passed through np.asarray first."""
    return not isinstance(a, DeviceImage) and hasattr(a, "__cuda_array_interface__")


def as_device(img, ctx=None, wait=True):
    """numpy array, cv.UMat, DeviceImage or foreign device array -> DeviceImage on `ctx` (uploads when needed; wait: see
    DeviceImage.from_numpy).  An object with `__cuda_array_interface__` (a u8 BGR frame or a u8 mask of another framework) is copied on
    the device, layout and bytes as they are (stitching_amd.ingest).
    A cv.UMat is what the reference's own classes hand on where cv2 produced one — the seam masks of `SeamFinder.resize`
    (stitching/seam_finder.py:37-43) reach `Blender.feed` that way when only Warper and Blender are switched — its array comes out of
    `.get()`."""
    if isinstance(img, DeviceImage):
        return img
    if hasattr(img, "__cuda_array_interface__"):
        from .ingest import ingest

        return ingest(img, ctx=ctx, wait=wait)
    if not isinstance(img, np.ndarray) and hasattr(img, "get"):
        img = img.get()
    return DeviceImage.from_numpy(img, ctx, wait)

