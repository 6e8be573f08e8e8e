"""Lens rectification on the device: frames of a Brown or fisheye lens become the pinhole frames every other stage assumes.

A `LensMap` is made once per camera on the host (numpy only: no device, no library): the source coordinate of every 16th destination
pixel in Q6.  `rectify_all` turns a list of distorted frames into pinhole `DeviceImage`s with ONE launch (`stx_rectify`): the kernel
interpolates the nodes and samples the source bilinearly, all in integers.  tests/numpy_rectify.py is the contract, byte for byte;
DESIGN.md section 22.
"""
import ctypes as C

import numpy as np

from . import _lib
from .stitching_error import StitchingError

CELL = _lib.LENS_CELL
_Q6_MIN, _Q6_MAX = -16384 * 64, 32767 * 64
_INSIDE_MARGIN = 1.0  # px that fit="inside" keeps between a border pixel's coordinate and the source's edge: covers error() < 1


def _size(size, what):
    try:
        w, h = (int(v) for v in size)
    except (TypeError, ValueError):
        raise StitchingError(f"{what} is (width, height), got {size!r}") from None
    if w < 1 or h < 1 or w > _lib.RECTIFY_MAX_SIDE or h > _lib.RECTIFY_MAX_SIDE:
        raise StitchingError(f"{what} {w}x{h}: sides are 1 .. {_lib.RECTIFY_MAX_SIDE}")
    return (w, h)


def _matrix(K, what):
    K = np.asarray(K, np.float64)
    if K.shape != (3, 3) or not np.all(np.isfinite(K)) or K[0, 0] == 0 or K[1, 1] == 0:
        raise StitchingError(f"{what} is a finite 3 x 3 camera matrix with non-zero focal lengths")
    return K


def node_counts(size):
    w, h = size
    return ((w + CELL - 1) // CELL + 1, (h + CELL - 1) // CELL + 1)


def _brown(K, dist, new_K):
    d = np.zeros(8)
    d[:dist.size] = dist
    k1, k2, p1, p2, k3, k4, k5, k6 = d

    def model(u, v):
        x, y = (u - new_K[0, 2]) / new_K[0, 0], (v - new_K[1, 2]) / new_K[1, 1]
        r2 = x * x + y * y
        radial = (1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))) / (1.0 + r2 * (k4 + r2 * (k5 + r2 * k6)))
        xd = x * radial + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
        yd = y * radial + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
        return K[0, 0] * xd + K[0, 2], K[1, 1] * yd + K[1, 2]

    return model


def _fisheye(K, D, new_K):
    k1, k2, k3, k4 = D

    def model(u, v):
        x, y = (u - new_K[0, 2]) / new_K[0, 0], (v - new_K[1, 2]) / new_K[1, 1]
        r = np.sqrt(x * x + y * y)
        theta = np.arctan(r)
        t2 = theta * theta
        theta_d = theta * (1.0 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4))))
        scale = np.where(r > 1e-12, theta_d / np.maximum(r, 1e-12), 1.0)
        return K[0, 0] * x * scale + K[0, 2], K[1, 1] * y * scale + K[1, 2]

    return model


def _border_pixels(size):
    w, h = size
    xs, ys = np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64)
    u = np.concatenate([xs, xs, np.zeros(h), np.full(h, w - 1.0)])
    v = np.concatenate([np.zeros(w), np.full(w, h - 1.0), ys, ys])
    return u, v


class LensMap:
    """The lens of one camera as a grid: `.nodes`, int32 [ny, nx, 2], holds the source coordinate (x, y) in Q6 of every 16th destination
    pixel, the nodes past the right and bottom edge included (nx = (W + 15) // 16 + 1).  `.src_size` / `.dst_size` are (width, height) of
    the distorted and of the rectified frame, `.new_K` the pinhole camera matrix of the rectified frame (None for `from_maps`).

    Made by `brown`, `fisheye` or `from_maps`; the plain constructor takes ready nodes.  Everything up to `error()` is numpy on the
    host; the device copy of the nodes is made at the first `rectify` on a context and kept."""

    def __init__(self, nodes, src_size, dst_size, new_K=None, model=None):
        self.src_size, self.dst_size = _size(src_size, "src_size"), _size(dst_size, "dst_size")
        nodes = np.asarray(nodes)
        nx, ny = node_counts(self.dst_size)
        if nodes.shape != (ny, nx, 2) or nodes.dtype.kind not in "iu":
            raise StitchingError(f"a {self.dst_size[0]}x{self.dst_size[1]} destination takes integer nodes of shape {(ny, nx, 2)} "
                                 f"(one every {CELL} pixels, the edges included), got {nodes.dtype} of shape {nodes.shape}")
        if nodes.size and (nodes.min() < _Q6_MIN or nodes.max() > _Q6_MAX):
            raise StitchingError(f"nodes are Q6 coordinates within [{_Q6_MIN}, {_Q6_MAX}]")
        self.nodes = np.ascontiguousarray(nodes, dtype=np.int32)
        self.nodes.setflags(write=False)
        self.new_K = None if new_K is None else np.array(new_K, np.float64)
        self._model = model  # (u, v) float64 arrays -> exact (sx, sy): what error() measures the grid against
        self._handles = {}   # id(ctx) -> (ctx, stx_lens_map*)

    # ---- constructors
    @classmethod
    def _from_model(cls, make, K, src_size, new_K, dst_size, fit):
        K, src_size = _matrix(K, "K"), _size(src_size, "src_size")
        dst_size = src_size if dst_size is None else _size(dst_size, "dst_size")
        if fit not in ("same", "inside"):
            raise StitchingError(f"fit {fit!r}: 'same' or 'inside'")
        if new_K is None:  # the source's camera, its focal lengths and centre scaled with the size
            new_K = K.copy()
            new_K[0] *= dst_size[0] / src_size[0]
            new_K[1] *= dst_size[1] / src_size[1]
        new_K = _matrix(new_K, "new_K").copy()
        if fit == "inside":
            new_K = cls._fit_inside(make, new_K, src_size, dst_size)
        model = make(new_K)
        nx, ny = node_counts(dst_size)
        u, v = np.meshgrid(np.arange(nx, dtype=np.float64) * CELL, np.arange(ny, dtype=np.float64) * CELL)
        return cls(_quantise(*model(u, v)), src_size, dst_size, new_K, model)

    @staticmethod
    def _fit_inside(make, new_K, src_size, dst_size):
        """The smallest factor on the focal lengths (the widest view) at which every border pixel of the destination samples inside the
        source, by bisection on the exact model: a factor passes when all coordinates lie _INSIDE_MARGIN inside the source's edges."""
        u, v = _border_pixels(dst_size)

        def scaled(s):
            k = new_K.copy()
            k[0, 0] *= s
            k[1, 1] *= s
            return k

        def passes(s):
            sx, sy = make(scaled(s))(u, v)
            return bool(np.all(np.isfinite(sx)) and np.all(np.isfinite(sy)) and sx.min() >= _INSIDE_MARGIN and sy.min() >= _INSIDE_MARGIN
                        and sx.max() <= src_size[0] - 1 - _INSIDE_MARGIN and sy.max() <= src_size[1] - 1 - _INSIDE_MARGIN)

        hi = 1.0
        while not passes(hi):
            hi *= 2.0
            if hi > 1024.0:
                raise StitchingError("fit='inside': no focal length up to 1024 times the given one keeps the destination inside the source")
        lo = hi / 2.0
        while passes(lo) and lo > 1.0 / 1024.0:
            hi, lo = lo, lo / 2.0
        if passes(lo):
            return scaled(lo)
        for _ in range(48):
            mid = 0.5 * (lo + hi)
            if passes(mid):
                hi = mid
            else:
                lo = mid
        return scaled(hi)

    @classmethod
    def brown(cls, K, dist, src_size, new_K=None, dst_size=None, fit="same"):
        """The Brown model in OpenCV's parameter order: dist = k1, k2, p1, p2[, k3[, k4, k5, k6]] (the rational model included; no tilt,
        no thin prism).  new_K: the pinhole camera of the rectified frame (default: K, scaled with dst_size); dst_size: default
        src_size.  fit="inside" scales new_K's focal lengths so that every destination pixel samples inside the source."""
        dist = np.asarray(dist, np.float64).ravel()
        if dist.size not in (4, 5, 8) or not np.all(np.isfinite(dist)):
            raise StitchingError(f"dist holds 4, 5 or 8 finite coefficients (k1, k2, p1, p2[, k3[, k4, k5, k6]]), got {dist.size}")
        K = _matrix(K, "K")
        return cls._from_model(lambda nk: _brown(K, dist, nk), K, src_size, new_K, dst_size, fit)

    @classmethod
    def fisheye(cls, K, D, src_size, new_K=None, dst_size=None, fit="same"):
        """The Kannala-Brandt model of cv2.fisheye: theta_d = theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8) with
        theta = atan(r); D = k1, k2, k3, k4.  The other arguments as `brown`."""
        D = np.asarray(D, np.float64).ravel()
        if D.size != 4 or not np.all(np.isfinite(D)):
            raise StitchingError(f"D holds the four finite coefficients k1, k2, k3, k4, got {D.size}")
        K = _matrix(K, "K")
        return cls._from_model(lambda nk: _fisheye(K, D, nk), K, src_size, new_K, dst_size, fit)

    @classmethod
    def from_maps(cls, map_x, map_y, src_size):
        """A full-resolution float map of any calibration, as cv2.initUndistortRectifyMap returns it: map_x, map_y [H, W] hold the source
        coordinate of every destination pixel.  Sampled at the nodes; a node past the last column extrapolates linearly from the last
        two (m[W-1] + (c - (W-1)) (m[W-1] - m[W-2])), rows likewise; a single column or row is repeated."""
        mx, my = np.asarray(map_x, np.float64), np.asarray(map_y, np.float64)
        if mx.ndim != 2 or mx.shape != my.shape or mx.size == 0:
            raise StitchingError(f"map_x and map_y are H x W arrays of one shape, got {mx.shape} and {my.shape}")
        if not (np.all(np.isfinite(mx)) and np.all(np.isfinite(my))):
            raise StitchingError("the maps hold a coordinate that is not finite")
        dst_size = _size((mx.shape[1], mx.shape[0]), "the maps' size")
        nx, ny = node_counts(dst_size)
        cx, cy = np.arange(nx) * CELL, np.arange(ny) * CELL

        def model(u, v):  # exact at the destination's own pixels, which is where error() asks
            ui, vi = np.asarray(u).astype(np.intp), np.asarray(v).astype(np.intp)
            return mx[vi, ui], my[vi, ui]

        return cls(_quantise(_extrapolated(mx, cx, cy), _extrapolated(my, cx, cy)), src_size, dst_size, None, model)

    # ---- the grid on the host
    def coordinates(self):
        """The Q5 source coordinates the device computes for every destination pixel: int32 [H, W, 2], value / 32 in pixels."""
        w, h = self.dst_size
        y, x = np.arange(h, dtype=np.int32)[:, None], np.arange(w, dtype=np.int32)[None, :]
        ax, ay, i, j = (x & 15)[..., None], (y & 15)[..., None], x >> 4, y >> 4
        n = self.nodes
        s = (16 - ay) * ((16 - ax) * n[j, i] + ax * n[j, i + 1]) + ay * ((16 - ax) * n[j + 1, i] + ax * n[j + 1, i + 1])
        return (s + 256) >> 9

    def error(self):
        """What the 16-pixel grid costs on this lens: the largest distance, in source pixels, between the coordinate the device uses
        (`coordinates() / 32`) and the exact model, over every destination pixel.  Host only."""
        if self._model is None:
            raise StitchingError("this LensMap was made from nodes alone: there is no exact model to measure it against")
        w, h = self.dst_size
        u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
        sx, sy = self._model(u, v)
        q = self.coordinates().astype(np.float64) / 32.0
        return float(np.max(np.hypot(q[..., 0] - sx, q[..., 1] - sy)))

    # ---- the nodes on the device
    def handle(self, ctx):
        """stx_lens_map* of this map on `ctx`, made at the first call"""
        entry = self._handles.get(id(ctx))
        if entry is None:
            nx, ny = node_counts(self.dst_size)
            h = C.c_void_p()
            _lib.check(ctx._lib.stx_lens_map_create(ctx.handle, self.dst_size[0], self.dst_size[1], self.src_size[0], self.src_size[1], nx, ny,
                                                    self.nodes.ctypes.data_as(C.POINTER(C.c_int)), C.byref(h)))
            entry = self._handles[id(ctx)] = (ctx, h)
        return entry[1]

    def release(self):
        for ctx, h in self._handles.values():
            if ctx.handle:  # a closed context has already returned all of its device memory
                ctx._lib.stx_lens_map_free(h)
        self._handles = {}

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass

    def __repr__(self):
        return f"LensMap({self.src_size[0]}x{self.src_size[1]} -> {self.dst_size[0]}x{self.dst_size[1]})"


def _quantise(sx, sy):
    s = np.stack([np.asarray(sx, np.float64), np.asarray(sy, np.float64)], axis=-1)
    if not np.all(np.isfinite(s)):
        raise StitchingError("the lens maps a node to a coordinate that is not finite")
    return np.clip(np.rint(s * 64.0), _Q6_MIN, _Q6_MAX).astype(np.int32)


def _extrapolated(m, cx, cy):
    """m [H, W] at the integer coordinates cy x cx, linearly continued past the last row and column"""
    def along(a, c, axis):
        n = a.shape[axis]
        inside = np.take(a, np.minimum(c, n - 1), axis=axis)
        if n == 1:
            return inside
        last = np.take(a, [n - 1], axis=axis)
        step = last - np.take(a, [n - 2], axis=axis)
        shape = [1, 1]
        shape[axis] = c.size
        over = np.maximum(c - (n - 1), 0).astype(np.float64).reshape(shape)
        return np.where(over > 0, last + over * step, inside)

    return along(along(m, cx, 1), cy, 0)


def lens_list(lenses, n):
    """`lenses` for n frames: one LensMap for all of them, or a sequence of n"""
    if isinstance(lenses, LensMap):
        return [lenses] * n
    try:
        lenses = list(lenses)
    except TypeError:
        raise StitchingError(f"lenses is a LensMap or a sequence of them, got {type(lenses).__name__}") from None
    if len(lenses) != n:
        raise StitchingError(f"{len(lenses)} lenses for {n} frames: one per frame, or one LensMap for all")
    for i, lens in enumerate(lenses):
        if not isinstance(lens, LensMap):
            raise StitchingError(f"lens {i} is a {type(lens).__name__}, not a LensMap")
    return lenses


def _layout(frame):
    """(width, height, channels, is_u8) of a frame before it is uploaded, or None where only the upload tells"""
    from .device import DeviceImage
    from .ingest import parse_cuda_array_interface

    if isinstance(frame, DeviceImage):
        return frame.width, frame.height, frame.channels, frame.dtype == np.uint8
    if hasattr(frame, "__cuda_array_interface__"):
        _, h, w, c, elem, _, _ = parse_cuda_array_interface(frame)
        return w, h, c, elem == _lib.U8
    if isinstance(frame, np.ndarray) and frame.ndim in (2, 3):
        return frame.shape[1], frame.shape[0], frame.shape[2] if frame.ndim == 3 else 1, frame.dtype == np.uint8
    return None


def check_layout(i, layout, lens):
    w, h, c, u8 = layout
    if not u8 or c not in (1, 3):
        raise StitchingError(f"rectify: frame {i} has {c} channel(s){'' if u8 else ' of another element type'}: u8 with 1 or 3 channels is taken")
    if (w, h) != lens.src_size:
        raise StitchingError(f"rectify: frame {i} is {w}x{h}, its lens was made for {lens.src_size[0]}x{lens.src_size[1]}")


def rectify_all(frames, lenses, border="constant", masks=False, ctx=None):
    """A list of distorted frames -> the list of rectified DeviceImages, by one launch; with masks=True (images, masks), the masks u8
    with 255 where all four taps of a pixel lie inside the source.

    frames: numpy arrays, DeviceImages (crop views included) or foreign device arrays, u8 with 1 or 3 channels; sizes may differ.
    lenses: one LensMap per frame, or one for all.  border: "constant" (a tap outside the source reads 0) or "replicate".
    The results are new images of the sizes the lenses were made for; a source is never written."""
    from .device import DeviceImage, as_device, get_context

    frames = list(frames)
    lenses = lens_list(lenses, len(frames))
    if border not in _lib.RECTIFY_BORDERS:
        raise StitchingError(f"border {border!r}: one of {list(_lib.RECTIFY_BORDERS)}")
    if not frames:
        return ([], []) if masks else []
    layouts = [_layout(f) for f in frames]
    for i, (layout, lens) in enumerate(zip(layouts, lenses)):
        if layout is not None:
            check_layout(i, layout, lens)
    ctx = ctx or get_context()
    dev = [as_device(f, ctx) for f in frames]
    for i, (layout, d, lens) in enumerate(zip(layouts, dev, lenses)):
        if layout is None:
            check_layout(i, _layout(d), lens)
    n = len(dev)
    srcs = (C.c_void_p * n)(*[d._h.value for d in dev])
    maps = (C.c_void_p * n)(*[lens.handle(ctx).value for lens in lenses])
    outs, mouts = (C.c_void_p * n)(), (C.c_void_p * n)()
    _lib.check(ctx._lib.stx_rectify(ctx.handle, n, srcs, maps, _lib.RECTIFY_BORDERS[border], 1 if masks else 0, outs, mouts if masks else None))
    imgs = [DeviceImage(ctx, C.c_void_p(h)) for h in outs]
    if masks:
        return imgs, [DeviceImage(ctx, C.c_void_p(h)) for h in mouts]
    return imgs


def rectify(frame, lens, border="constant", masks=False, ctx=None):
    """One distorted frame -> its rectified DeviceImage, or (image, mask) with masks=True (see rectify_all)."""
    out = rectify_all([frame], [lens], border=border, masks=masks, ctx=ctx)
    return (out[0][0], out[1][0]) if masks else out[0]
