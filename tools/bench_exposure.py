#!/usr/bin/env python
"""Exposure-gain estimation (stitching_amd.ExposureEstimator.feed) at the reference's low resolution (0.1 Mpx: 365 x 274 frames of
4000 x 3000 or 8000 x 6000 sources) on two cases: BASELINE config 2 (8 frames, one spherical ring) and config 4's 64 frames (16 x 4
cylindrical grid).  Device-resident warped inputs, default parameters (block size 32, one feed).
usage: python tools/bench_exposure.py [--steps 20] [--out profiles/exposure_feed.json] [--kinds gain,gain_blocks,...]
One JSON line per (case, kind): units, pair jobs, device statistics time (HIP events around the launch, median), host assembly + solve +
filter time (median), whole feed wall time (median), the restatement's CPU time (tests/numpy_exposure.py, one run), kernel_source_hash.
--solver host|device|both (profiles/exposure_solve.json): one line per (case, kind, solver) with the solver's name, the assembly + solve +
filter time (wall clock: with the device solver the elimination on the device and the host tail), and of the device solver the elimination
time (HIP events), the compaction + copy + back substitution time and the non-zeros of U; `both` also checks that the two solvers return
the same gain maps byte for byte and adds the ratio host / device.  At least 3 runs of --steps (the host solve of config 4 takes seconds);
the restatement is not run."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import stitching_amd as S  # noqa: E402
from stitching_amd import config, synthetic  # noqa: E402

LW, LH = 365, 274  # 0.1 Mpx of a 4:3 frame


def case(name):
    if name == "config2_low":
        return _warped(synthetic.ring_cameras(8, LW, LH, focal_factor=0.75), "spherical")
    return grid_case(16, 4)


def grid_case(n_yaw, n_pitch):
    """n_yaw of config 4's 16 columns, n_pitch rows (16 x 4: config 4's low-resolution layout itself)."""
    return _warped(synthetic.grid_cameras(n_yaw, n_pitch, LW, LH, max_edge_lat_deg=50.0, layout_yaw=16), "cylindrical")


def _warped(cams, wtype):
    frames = synthetic.make_frames(range(len(cams)), LW, LH)
    frames = [np.clip(np.rint(f.astype(np.float32) * np.float32(0.75 + 0.5 * ((7 * i) % 11) / 10)), 0, 255).astype(np.uint8)
              for i, f in enumerate(frames)]  # a different exposure per frame
    prev = config.device_resident()
    config.set_device_resident(True)
    try:
        wp = S.Warper(wtype)
        wp.set_scale(cams)
        sizes = [(LW, LH)] * len(cams)
        imgs = list(wp.warp_images(frames, cams))
        masks = list(wp.create_and_warp_masks(sizes, cams))
        corners, _ = wp.warp_rois(sizes, cams)
    finally:
        config.set_device_resident(prev)
    return wtype, [tuple(int(v) for v in c) for c in corners], imgs, masks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--kinds", default="gain,gain_blocks,channel,channel_blocks")
    ap.add_argument("--cases", default="config2_low,config4_low")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    ap.add_argument("--solver", default=None, choices=("host", "device", "both"), help="compare the solvers of the gain systems")
    args = ap.parse_args()
    if args.solver:
        return solver_lines(args)
    import bench
    from tests import numpy_exposure as X

    khash = bench.kernel_source_hash()
    ctx = S.get_context()
    lines = []
    for cname in args.cases.split(","):
        wtype, corners, imgs, masks = case(cname)
        h_imgs, h_masks = [i.numpy() for i in imgs], [m.numpy() for m in masks]
        for kind in args.kinds.split(","):
            est = S.ExposureEstimator(kind)
            est.feed(corners, imgs, masks)  # warm-up: sqrt table, allocator, code objects
            ctx.sync()
            wall, dev, host = [], [], []
            for _ in range(max(20, args.steps)):
                t = time.perf_counter()
                est.feed(corners, imgs, masks)
                wall.append((time.perf_counter() - t) * 1e3)
                dev.append(est.info["stats_ms"])
                host.append(est.info["solve_ms"])
            t = time.perf_counter()
            X.feed(kind, corners, h_imgs, h_masks)
            ref_ms = (time.perf_counter() - t) * 1e3
            rec = {"case": cname, "warper": wtype, "frames": len(imgs), "frame_size": [LW, LH], "kind": kind,
                   "units": est.info["units"], "pair_jobs": est.info["pair_jobs"], "runs": len(wall),
                   "device_stats_ms_median": round(statistics.median(dev), 4),
                   "host_solve_filter_ms_median": round(statistics.median(host), 4),
                   "feed_wall_ms_median": round(statistics.median(wall), 4),
                   "feed_wall_ms_min": round(min(wall), 4),
                   "restatement_cpu_ms": round(ref_ms, 1),
                   "kernel_source_hash": khash}
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    if args.out:
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


def solver_lines(args):
    import bench

    khash = bench.kernel_source_hash()
    ctx = S.get_context()
    lines = []
    for cname in args.cases.split(","):
        wtype, corners, imgs, masks = case(cname)
        for kind in args.kinds.split(","):
            recs, maps = {}, {}
            for solver in (("host", "device") if args.solver == "both" else (args.solver,)):
                est = S.ExposureEstimator(kind, solver=solver)
                est.feed(corners, imgs, masks)  # warm-up: sqrt table, allocator (the dense matrix), code objects
                ctx.sync()
                maps[solver] = est.getMatGains()
                wall, solve, lu, tail = [], [], [], []
                for _ in range(max(3, args.steps)):
                    t = time.perf_counter()
                    est.feed(corners, imgs, masks)
                    wall.append((time.perf_counter() - t) * 1e3)
                    solve.append(est.info["solve_ms"])
                    lu.append(est.info["device_lu_ms"])
                    tail.append(est.info["host_tail_ms"])
                recs[solver] = {"case": cname, "warper": wtype, "frames": len(imgs), "frame_size": [LW, LH], "kind": kind,
                                "solver": est.info["solver"], "units": est.info["units"], "pair_jobs": est.info["pair_jobs"],
                                "runs": len(wall), "solve_filter_ms_median": round(statistics.median(solve), 4),
                                "device_lu_ms_median": round(statistics.median(lu), 4),
                                "host_tail_ms_median": round(statistics.median(tail), 4), "u_nonzeros": est.info["u_nonzeros"],
                                "feed_wall_ms_median": round(statistics.median(wall), 4), "kernel_source_hash": khash}
            if args.solver == "both":
                same = all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(maps["host"], maps["device"]))
                recs["device"]["same_bits_as_host"] = bool(same)
                recs["device"]["host_over_device"] = round(recs["host"]["solve_filter_ms_median"] /
                                                           max(1e-9, recs["device"]["solve_filter_ms_median"]), 3)
            for rec in recs.values():
                print(json.dumps(rec), flush=True)
                lines.append(rec)
    if args.out:
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
