"""Exposure gains tracked from frame to frame on a known rig (tests/numpy_exposure_track.py is the contract).

`Composer.prepare` estimates the exposure gains once, on the low-resolution pass, and every later panorama of the rig applies them.
The cameras of a real rig go on exposing on their own.  An `ExposureTracker` given to a `StitchJob` (or to `Composer.prepare`) measures
the warped, compensated images every run makes anyway — integer sums over a lattice of the overlaps, one small HIP launch
(csrc/stx_exposure_track.hip) whose result is picked up one run later — and lays a residual gain per camera over the plan's gains:

    tracker = S.ExposureTracker(kind="gain", rate=0.25, stride=8)
    job = StitchJob(frames, cameras, compensator=compensator, exposure_tracker=tracker)
    for frames in stream:
        pano, mask = job.run(frames=frames)      # run k applies what run k - 1 measured

The plan's own compensator is never written.  Without a tracker nothing here runs.
"""
import ctypes as C
import time
import weakref

import numpy as np

from . import _lib
from ._marshal import handles, ptr
from .device import DeviceImage, as_device, get_context
from .exposure_error_compensator import ExposureErrorCompensator
from .exposure_estimation import solve_gains
from .stitching_error import StitchingError

KINDS = ("gain", "channel")
DEFAULT_RATE, DEFAULT_STRIDE, DEFAULT_LIMITS = 0.25, 8, (0.25, 4.0)


def track_update(kind, r, pairs, self_counts, stats, rate=DEFAULT_RATE, limits=DEFAULT_LIMITS):
    """One update of the residual gains, on the host, in float64 without fused operations (tests/numpy_exposure_track.py::track_update
    is the contract, equal in every bit).  r (n, planes): the residuals the measured images were made with; pairs (J, 2); self_counts
    (n,); stats (J, 8) = c, aB, aG, aR, bB, bG, bR, rej per pair.  Per plane: the means of both sides of every pair with c > 0
    ("gain": over the three channels), divided by the side's own residual — which makes the estimate absolute instead of a feedback
    product —, GainCompensator::singleFeed's system over them (solve_gains, host), and r + rate * (r* - r) clipped to limits.  A
    plane whose solve fails or returns a non-finite value keeps its residuals.  -> (r_next, {"solve_failures", "rejected_share"})"""
    if kind not in KINDS:
        raise StitchingError(f"unknown tracker kind {kind!r}: one of {list(KINDS)}")
    r = np.array(r, np.float64)
    if r.ndim != 2 or r.shape[1] != (3 if kind == "channel" else 1):
        raise StitchingError(f"track_update: r must be (n, {3 if kind == 'channel' else 1}) for kind {kind!r}, got {r.shape}")
    n, planes = r.shape
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    stats = np.asarray(stats, np.int64).reshape(-1, 8)
    counts = np.asarray(self_counts, np.int64).reshape(-1)
    if len(stats) != len(pairs) or counts.size != n:
        raise StitchingError("track_update: one row of statistics per pair and one self count per image")
    lo, hi = float(limits[0]), float(limits[1])
    out, failures = r.copy(), 0
    # the system's pairs: every image with itself (N = max(1, c_ii)), then the pair jobs (N = max(1, c))
    ij = np.concatenate([np.repeat(np.arange(n, dtype=np.int64)[:, None], 2, axis=1), pairs]).astype(np.int32)
    skip = np.ones(n, bool)
    for (a, b), st in zip(pairs.tolist(), stats):
        if int(st[0]) > 0:
            skip[a] = skip[b] = False
    for p in range(planes):
        vals = np.zeros((n + len(pairs), 3), np.float64)
        vals[:n, 0] = np.maximum(1, counts)
        for j, ((a, b), st) in enumerate(zip(pairs.tolist(), stats.tolist())):
            c = st[0]
            vals[n + j, 0] = max(1, c)
            if c <= 0:
                continue
            if kind == "channel":
                ia, ib = float(st[1 + p]) / float(c), float(st[4 + p]) / float(c)
            else:
                ia, ib = float(st[1] + st[2] + st[3]) / (3.0 * float(c)), float(st[4] + st[5] + st[6]) / (3.0 * float(c))
            vals[n + j, 1], vals[n + j, 2] = ia / r[a, p], ib / r[b, p]
        try:
            star = solve_gains(n, ij, vals, skip, solver="host")
            ok = bool(np.isfinite(star).all())
        except StitchingError:
            ok = False
        if not ok:
            failures += 1
            continue
        out[:, p] = np.minimum(np.maximum(r[:, p] + rate * (star - r[:, p]), lo), hi)
    rej = int(stats[:, 7].sum()) if len(stats) else 0
    total = rej + (int(stats[:, 0].sum()) if len(stats) else 0)
    return out, {"solve_failures": failures, "rejected_share": float(rej) / float(total) if total > 0 else 0.0}


class TrackHandle:
    """The device side of a tracker for one rig (stx_exposure_track_*): the lattice grids of the warped masks, made once, and the
    measure / collect pair.  rects: (x, y, w, h) per image in panorama coordinates; masks: the warped u8 masks of those rectangles (host
    arrays are uploaded; device views are taken as they are).  `pairs` (J, 2) and `self_counts` (n,) are those of the contract."""

    def __init__(self, rects, masks, stride=DEFAULT_STRIDE, ctx=None):
        masks = list(masks)
        ctx = ctx or next((m.ctx for m in masks if isinstance(m, DeviceImage)), None) or get_context()
        self.ctx, self._h = ctx, None
        r = np.ascontiguousarray(np.asarray(rects, np.int32).reshape(-1, 4))
        if len(masks) != len(r):
            raise StitchingError(f"{len(masks)} masks for {len(r)} rectangles")
        d = [as_device(m, ctx) for m in masks]
        h = C.c_void_p()
        _lib.check(ctx._lib.stx_exposure_track_create(ctx.handle, len(r), ptr(r.reshape(-1)), handles(d), int(stride), C.byref(h)))
        self._h, self.n, self.stride = h, len(r), int(stride)
        count = C.c_int(0)
        _lib.check(ctx._lib.stx_exposure_track_pairs(h, C.byref(count), None, None))
        ab, self.self_counts = np.zeros((max(1, count.value), 2), np.int32), np.zeros(self.n, np.int64)
        count = C.c_int(len(ab))
        _lib.check(ctx._lib.stx_exposure_track_pairs(h, C.byref(count), ptr(ab.reshape(-1)), ptr(self.self_counts)))
        self.pairs = ab[:count.value].copy()

    def measure(self, imgs):
        """Queue the statistics of the warped, compensated u8x3 images of the rectangles: no host wait.  At most two may be pending."""
        d = [as_device(i, self.ctx) for i in imgs]
        if len(d) != self.n:
            raise StitchingError(f"{len(d)} images for a tracker of {self.n}")
        _lib.check(self.ctx._lib.stx_exposure_track_measure(self._h, handles(d)))

    def collect(self):
        """The (J, 8) int64 statistics of the oldest pending measure; waits for its event alone.  Refused when none is pending."""
        out = np.zeros((max(1, len(self.pairs)), 8), np.int64)
        _lib.check(self.ctx._lib.stx_exposure_track_collect(self._h, ptr(out.reshape(-1))))
        return out[:len(self.pairs)]

    def info(self):
        v = np.zeros(6, np.float64)
        _lib.check(self.ctx._lib.stx_exposure_track_info(self._h, ptr(v)))
        return {"pairs": int(v[0]), "tile_jobs": int(v[1]), "grid_bytes": int(v[2]), "stats_ms": float(v[3]), "wait_ms": float(v[4]),
                "measures": int(v[5])}

    def free(self):
        if self._h is not None:
            if self.ctx.handle:  # a closed context has already returned its device memory
                self.ctx._lib.stx_exposure_track_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def scale_gain_maps(maps, factors, ctx=None):
    """maps[i] * factors[i] in fp32 on the device, all maps in one launch (stx_gain_maps_scale).  maps: f32x1 or f32x3 gain maps
    (DeviceImages or host arrays); factors: (n,) or (n, 1) — one per map — or (n, 3), BGR: f32x1 maps then come back f32x3.
    -> DeviceImages."""
    maps = list(maps)
    ctx = ctx or next((m.ctx for m in maps if isinstance(m, DeviceImage)), None) or get_context()
    d = [as_device(m, ctx) for m in maps]
    f = np.ascontiguousarray(np.asarray(factors, np.float64).reshape(len(d), -1), np.float32)
    outs = (C.c_void_p * max(1, len(d)))()
    _lib.check(ctx._lib.stx_gain_maps_scale(ctx.handle, len(d), handles(d), ptr(f.reshape(-1)), f.shape[1], outs))
    return [DeviceImage(ctx, C.c_void_p(outs[i])) for i in range(len(d))]


class _TrackedCompensator(ExposureErrorCompensator):
    """The compensator a tracked job applies: the plan's gains times the tracker's residuals, served through `_gain_map` / `apply`.
    It reads the plan's compensator and never writes it (`gains_version` does not move).  Its kind is the plan's, with three planes
    where either side has three; a plan without a compensator, or of kind "no", counts as gain 1."""

    def __init__(self, plan, tracker):
        self._plan_kind = "no" if plan is None else plan.compensator_type
        self._blocks = self._plan_kind.endswith("_blocks")
        three = self._plan_kind.startswith("channel") or tracker.planes == 3
        kind = ("channel_blocks" if three else "gain_blocks") if self._blocks else ("channel" if three else "gain")
        super().__init__(kind, estimator=tracker)  # estimates nothing: the gains are derived
        self._plan, self._three, self._hi = plan, three, float(tracker.limits[1])
        self._r = self._version = None
        self._plan_maps = {}  # context -> (the plan's gains_version, its maps on the device, their STX_GAIN_MAP_BOUNDED flags)
        self._scaled = {}     # context -> [(scaled map, flag)] of the residuals of `refresh`

    def set_gains(self, gains):
        raise StitchingError("the gains of a tracked job are derived: set the plan's compensator, or reset the tracker")

    def feed(self, corners, imgs, masks):
        raise StitchingError("the gains of a tracked job are derived: feed the plan's compensator")

    def refresh(self, r):
        """the effective gains of the next run, from the plan's gains as they are now and the residuals r (n, planes)"""
        plan = self._plan
        if self._plan_kind != "no" and plan.gains is None:
            raise StitchingError("ExposureErrorCompensator.set_gains(gains) must be called before apply")
        r, version = np.array(r, np.float64), None if plan is None else plan.gains_version
        if self._r is None or r.tobytes() != self._r.tobytes() or version != self._version:
            self._scaled = {}  # (residuals that did not move keep their maps: no launch)
        self._r, self._version = r, version
        if self._blocks:
            self.gains = plan.gains  # (what says "set": the maps themselves come from _gain_map)
            return
        gains = []
        for i in range(len(self._r)):
            ri = self._r[i]
            if ri.size == 1 and self._three:
                ri = np.full(3, ri[0])
            p = np.ones(1) if self._plan_kind == "no" else plan.gains[i]
            p = p[:3] if p.size >= 3 else np.full(ri.size, p[0])
            gains.append(p * ri)  # float64; `apply` demotes to float32
        self.gains = gains

    def _bounded_flags(self):
        """STX_GAIN_MAP_BOUNDED per map, for the products: every |P| * hi finite and below 2^31 / 255 (the residuals never exceed hi)"""
        return [_lib.GAIN_MAP_BOUNDED if bool(np.isfinite(g).all() and np.abs(g).max(initial=0.0) * self._hi < 8.0e6) else 0
                for g in self._plan.gains]

    def _plan_device_maps(self, ctx):
        plan = self._plan
        hit = self._plan_maps.get(id(ctx))
        if hit is None or hit[0] != plan.gains_version:
            hit = self._plan_maps[id(ctx)] = (plan.gains_version, [as_device(g, ctx) for g in plan.gains], self._bounded_flags())
        return hit[1], hit[2]

    def _gain_map(self, idx, ctx):
        hit = self._scaled.get(id(ctx))
        if hit is None:
            maps, flags = self._plan_device_maps(ctx)
            hit = self._scaled[id(ctx)] = list(zip(scale_gain_maps(maps, self._r[:len(maps)], ctx), flags))
        return hit[idx]


class ExposureTracker:
    """Residual exposure gains of the cameras of a known rig, followed from run to run.

    kind: "gain" (one residual per camera) or "channel" (one per camera and BGR channel).  rate: the share of the way to the newly
    solved gains a run goes (0 < rate <= 1).  stride: the lattice — every stride-th panorama pixel both ways is a sample (1 .. 64).
    limits: (lo, hi) the residuals are clipped to.

    Give it to one StitchJob (`exposure_tracker=`) or to Composer.prepare.  Run k applies plan gains x residuals, the residuals being
    a function of run k - 1's statistics alone (run 0: 1); the only host wait the tracker adds is the one for the previous run's
    statistics, at the start of a run.
    `factors`: a copy of the residuals the last run applied (n, planes), None before a job has bound the tracker.  `last_stats`: (pairs
    (J, 2), self counts (n,), statistics (J, 8)) of the last run, or None.  `info`: the rejected share of the samples and the failed solves of
    the last update, the failed solves so far, the updates so far, `wait_ms` of the last collect (host clock), `stats_ms` of the
    statistics launch it collected (HIP events), `update_ms` of the last collect + update on the host (it sits in front of the run's first
    launch), pair and tile jobs and the bytes of the lattice grids."""

    def __init__(self, kind="gain", rate=DEFAULT_RATE, stride=DEFAULT_STRIDE, limits=DEFAULT_LIMITS):
        if kind not in KINDS:
            raise StitchingError(f"unknown tracker kind {kind!r}: one of {list(KINDS)}")
        try:
            rate, lo, hi = float(rate), float(limits[0]), float(limits[1])
            bad_stride = int(stride) != stride
        except (TypeError, ValueError, IndexError):
            raise StitchingError("ExposureTracker: rate and stride are numbers, limits a pair (lo, hi)") from None
        if not (0.0 < rate <= 1.0):
            raise StitchingError(f"ExposureTracker: rate {rate} outside (0, 1]")
        if bad_stride or not (1 <= int(stride) <= _lib.TRACK_STRIDE_MAX):
            raise StitchingError(f"ExposureTracker: stride {stride!r} outside 1 .. {_lib.TRACK_STRIDE_MAX}")
        if len(limits) != 2 or not (0.0 < lo <= 1.0 <= hi) or not np.isfinite(hi):
            raise StitchingError(f"ExposureTracker: limits {limits!r}: a pair 0 < lo <= 1 <= hi")
        self.kind, self.rate, self.stride, self.limits = kind, rate, int(stride), (lo, hi)
        self.planes = 3 if kind == "channel" else 1
        self._r = self._job = self._handle = None
        self._pending = self._discard = self._fresh = False
        self._last_stats = None
        self.info = {"rejected_share": 0.0, "solve_failures": 0, "solve_failures_total": 0, "updates": 0, "wait_ms": 0.0, "stats_ms": 0.0,
                     "update_ms": 0.0, "pairs": 0, "tile_jobs": 0, "grid_bytes": 0}

    @property
    def factors(self):
        return None if self._r is None else self._r.copy()

    @property
    def last_stats(self):
        """(pairs (J, 2), self counts (n,), statistics (J, 8)) of the last run, or None before any: reading it right after a run waits for
        that run's statistics (the next run would, at its start)"""
        self._collect()
        return self._last_stats

    def reset(self):
        """Residuals back to 1; what a run has measured and no update has used yet is dropped."""
        if self._r is not None:
            self._r = np.ones_like(self._r)
        self._discard, self._fresh = self._pending, False
        self._last_stats = None

    # ---- what StitchJob calls ----------------------------------------------------------------------------------------------------
    def _bind(self, job, n):
        """one tracker, one job: the residuals belong to that job's cameras"""
        other = self._job() if self._job is not None else None
        if other is not None and other is not job:
            raise StitchingError("this ExposureTracker belongs to another StitchJob: one tracker per job")
        self._job = weakref.ref(job)
        if self._r is None or len(self._r) != n:
            self._r = np.ones((n, self.planes), np.float64)

    def _create(self, ctx, rects, masks):
        """a first run of a rig: the lattice grids of its warped masks (the masks themselves are not kept)"""
        self._release()
        self._handle = TrackHandle(rects, masks, self.stride, ctx)
        i = self._handle.info()
        self.info.update(pairs=i["pairs"], tile_jobs=i["tile_jobs"], grid_bytes=i["grid_bytes"])

    def _release(self):
        """the job drops its geometry: the handle goes (with what it has measured), the residuals stay"""
        if self._handle is not None:
            self._handle.free()
        self._handle = None
        self._pending = self._discard = False  # (statistics already collected stay: they belong to the residuals, not to the handle)

    def _collect(self):
        """what the last run measured, if nobody has picked it up yet: the one host wait of the tracker (on that run's event)"""
        if not self._pending:
            return
        h = self._handle
        stats = h.collect()
        self._pending = False
        i = h.info()
        self.info.update(wait_ms=i["wait_ms"], stats_ms=i["stats_ms"])
        if self._discard:
            self._discard = False
            return
        self._last_stats = (h.pairs.copy(), h.self_counts.copy(), stats)
        self._fresh = True

    def _begin_run(self):
        """collect + update for the previous run -> the residuals this run applies"""
        t0 = time.perf_counter()
        self._collect()
        if self._fresh:
            self._fresh = False
            pairs, self_counts, stats = self._last_stats
            self._r, u = track_update(self.kind, self._r, pairs, self_counts, stats, self.rate, self.limits)
            self.info.update(rejected_share=u["rejected_share"], solve_failures=u["solve_failures"], updates=self.info["updates"] + 1,
                             solve_failures_total=self.info["solve_failures_total"] + u["solve_failures"])
        self.info["update_ms"] = (time.perf_counter() - t0) * 1e3
        return self._r

    def _measure(self, imgs):
        """the run's images are final: queue their statistics (no wait)"""
        if self._handle is None:
            raise StitchingError("internal: the tracker has no grids: the geometry pass did not make them")
        self._handle.measure(imgs)
        self._pending = True
