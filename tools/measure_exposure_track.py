#!/usr/bin/env python
"""Exposure tracking (stitching_amd.ExposureTracker) in the steady state of a known rig: BASELINE config 2's rig
(eight 4000 x 3000 frames in device memory, one ring, spherical warper, 5 bands) with a "gain_blocks" compensator.  A tracked and an
untracked StitchJob alternate call by call in one process, so they share whatever else the machine is doing; the yardstick is the
untracked job of the same run.
usage: python tools/measure_exposure_track.py [--steps 60] [--warmup 5] [--strides 4,8,16] [--out profiles/exposure_track.json]
One JSON line per stride:
  device_ms_tracked / device_ms_untracked  device time of one panorama between two events of the context's stream (median, min, max)
  host_call_ms_tracked / _untracked        host time of the job.run() call that queues the panorama
  host_update_ms                           of it, collect + update for the previous run: it precedes the run's first launch
  stats_kernel_ms                          the statistics launch alone, by the HIP events the library records around it
  wait_ms                                  host time `collect` waited for the previous run's event — (a) `synced`: the caller waits for
                                           every panorama before it starts the next (as the timing above does), (b) `back_to_back`:
                                           the caller queues panoramas without waiting, so the host runs ahead of the device
  rejected_share                           samples with a byte at 0 or 255, of all samples where both masks are 255
and a summary line.  Not measured here: other rigs, hardware counters, a "channel" tracker over gain_blocks (its gains are a second
pass over f32x3 maps instead of the warp's epilogue)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import stitching_amd as S  # noqa: E402
from stitching_amd import synthetic  # noqa: E402
from stitching_amd.pipeline import StitchJob  # noqa: E402


def q(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def timed_run(ctx, job):
    """(device ms of one panorama: events around everything the run queues — host time in front of a launch included, the device
    idles through it —, host ms of the call that queues it)"""
    ctx.mark(0)
    t0 = time.perf_counter()
    out = job.run()
    host = (time.perf_counter() - t0) * 1e3
    ctx.mark(1)
    ctx.sync()
    del out
    return ctx.elapsed_ms(0, 1), host


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--strides", default="4,8,16")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--size", default="4000x3000")
    ap.add_argument("--bands", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()
    import bench

    ctx = S.get_context()
    w, h = (int(v) for v in args.size.split("x"))
    n, lines = args.frames, []
    base = {"frames": n, "frame_size": [w, h], "bands": args.bands, "compensator": "gain_blocks", "tracker_kind": "gain",
            "kernel_source_hash": bench.kernel_source_hash(), "runs": args.steps, "warmup": args.warmup}

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    frames = [S.DeviceImage.from_numpy(f, ctx) for f in synthetic.make_frames(range(n), w, h)]
    cams = synthetic.ring_cameras(n, w, h, focal_factor=0.75)
    rng = np.random.default_rng(7)
    comp = S.ExposureErrorCompensator("gain_blocks", estimator=object())
    comp.set_gains([rng.uniform(0.9, 1.1, (24, 32)).astype(np.float32) for _ in range(n)])
    kw = dict(warper_type="spherical", blender_type="multiband", num_bands=args.bands, ctx=ctx, compensator=comp)
    plain = StitchJob(frames, cams, **kw)
    for _ in range(args.warmup):
        timed_run(ctx, plain)
    medians = {}
    for stride in (int(s) for s in args.strides.split(",")):
        tracker = S.ExposureTracker("gain", rate=0.25, stride=stride)
        job = StitchJob(frames, cams, exposure_tracker=tracker, **kw)
        for _ in range(args.warmup):
            timed_run(ctx, job)
            timed_run(ctx, plain)
        assert job.last_reused and plain.last_reused
        t_tracked, t_plain, h_tracked, h_plain, stats_ms, wait_ms, update_ms, rejected = [], [], [], [], [], [], [], []
        for _ in range(args.steps):  # alternating: both jobs see the same stretch of the machine's time
            d, hm = timed_run(ctx, job)
            t_tracked.append(d)
            h_tracked.append(hm)
            wait_ms.append(tracker.info["wait_ms"])      # of this run's collect: the previous run's event
            stats_ms.append(tracker.info["stats_ms"])    # of the launch that collect picked up
            update_ms.append(tracker.info["update_ms"])  # collect + update on the host, in front of the run's first launch
            rejected.append(tracker.info["rejected_share"])
            d, hm = timed_run(ctx, plain)
            t_plain.append(d)
            h_plain.append(hm)
        ahead = []
        for _ in range(args.steps):  # nobody waits: the host queues the next panorama while the device works on this one
            out = job.run()
            ahead.append(tracker.info["wait_ms"])
            del out
        ctx.sync()
        info = tracker.info
        rec = dict(base, case=f"stride_{stride}", stride=stride, pairs=info["pairs"], tile_jobs=info["tile_jobs"], grid_bytes=info["grid_bytes"],
                   device_ms_tracked=q(t_tracked), device_ms_untracked=q(t_plain), host_call_ms_tracked=q(h_tracked),
                   host_call_ms_untracked=q(h_plain), host_update_ms=q(update_ms), stats_kernel_ms=q(stats_ms),
                   wait_ms={"synced": q(wait_ms), "back_to_back": q(ahead)}, rejected_share=round(statistics.median(rejected), 6),
                   ranges_overlap=bool(min(t_tracked) <= max(t_plain) and min(t_plain) <= max(t_tracked)),
                   solve_failures=info["solve_failures_total"], factors=[round(float(v), 6) for v in tracker.factors[:, 0]])
        emit(rec)
        medians[stride] = (rec["device_ms_tracked"]["median"], rec["device_ms_untracked"]["median"], rec["stats_kernel_ms"]["median"])
        job.release_geometry()
        del job, tracker
    emit(dict(base, case="summary", tracked_minus_untracked_ms={str(s): round(m[0] - m[1], 4) for s, m in medians.items()},
              stats_kernel_ms={str(s): m[2] for s, m in medians.items()}))
    if args.out:
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
