"""Exposure-gain estimation on the device: ExposureCompensator::feed for "gain", "gain_blocks", "channel" and "channel_blocks".

`ExposureEstimator` is duck-typed like the cv.detail compensators the reference builds (stitching/exposure_error_compensator.py:25-41):
`feed(corners, imgs, masks)` on the low-resolution warped images, then `getMatGains()`.  The overlap statistics of every feed are one
HIP launch over a table of unit pairs (csrc/stx_exposure.hip); the linear system is assembled on the host and solved there
(csrc/stx_exposure_host.cpp, the default) or by a dense fp64 LU on the device (csrc/stx_solve.hip, solver="device": the same bits).  The algorithm restates OpenCV 4.x from recollection; tests/numpy_exposure.py is the contract and fidelity to
real OpenCV is unpinned.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._marshal import count_then_fill, handles, image_spec, info_dict, int_pairs, one_context, ptr
from .device import as_device, get_context
from .stitching_error import StitchingError


def _image(a, what, i):
    """The array (numpy or DeviceImage) and its (w, h): u8 with 3 channels for an image, 1 for a mask, not empty."""
    a, wh, ch, dt = image_spec(a, what, i)
    want = 3 if what == "image" else 1
    if dt != np.uint8 or ch != want:
        raise StitchingError(f"{what} {i}: exposure estimation needs u8 with {want} channel(s), got {dt} with {ch}")
    if wh[0] == 0 or wh[1] == 0:
        raise StitchingError(f"{what} {i}: empty image")
    return a, wh


class ExposureEstimator:
    """ExposureCompensator::feed on the device.  kind: "gain" | "gain_blocks" | "channel" | "channel_blocks"; nr_feeds and
    block_size as cv.detail_ChannelsCompensator(nr_feeds) / cv.detail_BlocksChannelsCompensator(bl, bl, nr_feeds) take them.
    solver: "host" | "device" — where the gain systems are solved; None: config.exposure_solver() at every feed."""

    def __init__(self, kind, nr_feeds=1, block_size=32, solver=None):
        if kind not in _lib.EXPOSURE_KINDS:
            raise StitchingError(f"unknown exposure estimator kind {kind!r}: one of {sorted(_lib.EXPOSURE_KINDS)}")
        if int(nr_feeds) < 1 or int(block_size) < 1:
            raise StitchingError("nr_feeds and block_size must be >= 1")
        if solver is not None and solver not in _lib.EXPOSURE_SOLVERS:
            raise StitchingError(f"unknown exposure solver {solver!r}: one of {sorted(_lib.EXPOSURE_SOLVERS)}")
        self.kind, self.nr_feeds, self.block_size, self.solver = kind, int(nr_feeds), int(block_size), solver
        self.gains = []
        # of the last feed: units, pair jobs, device statistics ms, assembly + solve + filter ms (wall clock, whichever solver), the solver
        # used and, of the device solver, elimination ms / compaction + copy + back substitution ms / non-zeros of U
        self.info = None

    def _prepare(self, corners, imgs, masks):
        """-> (ctx, the leading arguments of stx_exposure_feed_ex and stx_exposure_stats, the images' (w, h), what those arguments
        point into: to be held until the calls are made)"""
        imgs, masks, corners = list(imgs), list(masks), [tuple(int(v) for v in c) for c in corners]
        if not (len(imgs) == len(masks) == len(corners)):
            raise StitchingError("feed needs as many corners, images and masks")
        sizes = []
        for i, (im, mk) in enumerate(zip(imgs, masks)):
            imgs[i], wh = _image(im, "image", i)
            masks[i], mwh = _image(mk, "mask", i)
            if wh != mwh:
                raise StitchingError(f"mask {i} is {mwh[0]}x{mwh[1]}, its image {wh[0]}x{wh[1]}")
            sizes.append(wh)
        ctx = one_context(imgs + masks)
        d_imgs, d_masks, cs = [as_device(a, ctx) for a in imgs], [as_device(a, ctx) for a in masks], int_pairs(corners, len(imgs))
        args = (ctx.handle, _lib.EXPOSURE_KINDS[self.kind], len(imgs), handles(d_imgs), handles(d_masks), ptr(cs), self.block_size)
        return ctx, args, sizes, (d_imgs, d_masks, cs)  # args holds raw handles and addresses: these keep what they name alive

    def feed(self, corners, imgs, masks):
        """Estimate the gains (numpy arrays, cv.UMat-likes or DeviceImages of one context; the images are not modified)."""
        corners, imgs, masks = list(corners), list(imgs), list(masks)
        if not corners and not imgs and not masks:
            return
        ctx, args, sizes, alive = self._prepare(corners, imgs, masks)
        solver = -1 if self.solver is None else _lib.EXPOSURE_SOLVERS[self.solver]
        info = np.zeros(8, np.float64)

        def call(count, out):
            o, i = (None, None) if out is None else (ptr(out), ptr(info))
            _lib.check(ctx._lib.stx_exposure_feed_ex(*args, self.nr_feeds, solver, o, count, i))

        out, _ = count_then_fill(call, C.c_longlong, lambda k: np.zeros(k, np.float64))
        del alive  # both calls are made
        names = {v: k for k, v in _lib.EXPOSURE_SOLVERS.items()}
        self.info = info_dict(info, [("units", int), ("pair_jobs", int), ("stats_ms", float), ("solve_ms", float),
                                     ("solver", lambda v: names[int(v)]), ("device_lu_ms", float), ("host_tail_ms", float),
                                     ("u_nonzeros", int)])
        gains, o = [], 0
        for w, h in sizes:
            if self.kind == "gain":
                gains.append(out[o:o + 1].reshape(1, 1).copy())
                o += 1
            elif self.kind == "channel":
                gains.append(out[o:o + 3].reshape(3, 1).copy())
                o += 3
            else:
                bpw, bph = -(-w // self.block_size), -(-h // self.block_size)
                k = bpw * bph * (3 if self.kind == "channel_blocks" else 1)
                g = out[o:o + k].astype(np.float32)
                gains.append(g.reshape(bph, bpw, 3) if self.kind == "channel_blocks" else g.reshape(bph, bpw))
                o += k
        self.gains = gains

    def getMatGains(self):  # noqa: N802 - the cv.detail name
        """Per image: "gain" (1, 1) float64, "channel" (3, 1) float64 BGR, the block kinds their filtered float32 gain maps."""
        return [g.copy() for g in self.gains]

    def stats(self, corners, imgs, masks):
        """The first feed's overlap statistics per pair job: (ab (J, 2) int, c (J,) int64, sums (J, 6) float64) — sums are
        {sum_a, sum_b, 0...} for the gain kinds and {B, G, R of a, B, G, R of b} for the channel kinds."""
        ctx, args, _, alive = self._prepare(corners, imgs, masks)

        def call(count, out):
            _lib.check(ctx._lib.stx_exposure_stats(*args, count, *([None] * 3 if out is None else [ptr(a) for a in out])))

        (ab, c, s), k = count_then_fill(call, C.c_longlong, lambda J: (np.zeros((J, 2), np.int32), np.zeros(J, np.int64),
                                                                       np.zeros((J, 6), np.float64)))
        del alive  # both calls are made
        return ab[:k], c[:k], s[:k]


def solve_gains(m, pairs, n_iij_iji, skip, solver="host", ctx=None):
    """GainCompensator::singleFeed's assembly + cv::solve from given statistics.  pairs (P, 2) with i <= j,
    n_iij_iji (P, 3) = N(i,j), I(i,j), I(j,i); skip (m,) bool.  -> gains (m,) float64.  solver "host": no GPU; "device": the
    elimination on ctx's device (the default context when None), the same bits."""
    if solver not in _lib.EXPOSURE_SOLVERS:
        raise StitchingError(f"unknown exposure solver {solver!r}: one of {sorted(_lib.EXPOSURE_SOLVERS)}")
    pairs = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
    vals = np.ascontiguousarray(np.asarray(n_iij_iji, np.float64).reshape(-1, 3))
    sk = np.ascontiguousarray(np.asarray(skip, bool).astype(np.uint8).reshape(-1))
    if sk.size != m or vals.shape[0] != pairs.shape[0]:
        raise StitchingError("solve_gains: skip must hold m values and n_iij_iji one row per pair")
    out = np.zeros(max(1, m), np.float64)
    L = _lib.lib()
    if solver == "device":
        ctx = ctx or get_context()
        _lib.check(L.stx_exposure_solve_device(ctx.handle, int(m), pairs.shape[0], ptr(pairs), ptr(vals), ptr(sk), ptr(out), None))
        return out[:m]
    _lib.check(L.stx_exposure_solve(int(m), pairs.shape[0], ptr(pairs), ptr(vals), ptr(sk), ptr(out)))
    return out[:m]


def lu_solve_device(A, b, ctx=None, want_info=False):
    """A x = b by the device LU alone (stx_lu_solve_device; tests and tools): the bits of cv::solve(DECOMP_LU)'s dense loop for every
    n >= 1.  -> x (n,) float64, with want_info also {"device_lu_ms", "host_tail_ms", "u_nonzeros"}."""
    A = np.ascontiguousarray(np.asarray(A, np.float64))
    b = np.ascontiguousarray(np.asarray(b, np.float64).reshape(-1))
    if A.ndim != 2 or A.shape[0] != A.shape[1] or A.shape[0] < 1 or b.size != A.shape[0]:
        raise StitchingError("lu_solve_device: A must be n x n with n >= 1 and b hold n values")
    ctx = ctx or get_context()
    x, info = np.zeros(A.shape[0], np.float64), np.zeros(4, np.float64)
    _lib.check(ctx._lib.stx_lu_solve_device(ctx.handle, A.shape[0], ptr(A), ptr(b), ptr(x), ptr(info)))
    if want_info:
        return x, info_dict(info, [("device_lu_ms", float), ("host_tail_ms", float), ("u_nonzeros", int)])
    return x
