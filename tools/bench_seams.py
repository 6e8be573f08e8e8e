#!/usr/bin/env python
"""Seam finding (stitching_amd.SeamEstimator("voronoi").find) on three cases: BASELINE config 2 (8 frames, one spherical ring) and config 4's
64 frames (16 x 4 cylindrical grid) at the reference's low resolution (0.1 Mpx: 365 x 274 frames), and config 2 at full resolution
(4000 x 3000 frames).  Device-resident warped masks (the images are read for their sizes only, so the masks stand in for them).
usage: python tools/bench_seams.py [--steps 20] [--out profiles/seam_find.json] [--cases config2_low,config4_low,config2_full]
One JSON line per case: pairs, dependency levels, device time of the levels (HIP events, median), the same with the copy of the inputs
into the result buffers (median), whole call wall time (median), the restatement's CPU time (tests/numpy_seams.py, one run; host masks),
whether the results are equal byte for byte, kernel_source_hash."""
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
        w, h, wtype = LW, LH, "spherical"
        cams = synthetic.ring_cameras(8, w, h, focal_factor=0.75)
    elif name == "config4_low":
        w, h, wtype = LW, LH, "cylindrical"
        cams = synthetic.grid_cameras(16, 4, w, h, max_edge_lat_deg=50.0, layout_yaw=16)
    elif name == "config2_full":
        w, h, wtype = 4000, 3000, "spherical"
        cams = synthetic.ring_cameras(8, w, h, focal_factor=0.75)
    else:
        raise SystemExit(f"unknown case {name}")
    prev = config.device_resident()
    config.set_device_resident(True)
    try:
        wp = S.Warper(wtype)
        wp.set_scale(cams)
        sizes = [(w, h)] * len(cams)
        masks = list(wp.create_and_warp_masks(sizes, cams))
        corners, _ = wp.warp_rois(sizes, cams)
    finally:
        config.set_device_resident(prev)
    return wtype, (w, h), [tuple(int(v) for v in c) for c in corners], masks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--cases", default="config2_low,config4_low,config2_full")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()
    import bench
    from tests import numpy_seams as Z

    khash = bench.kernel_source_hash()
    ctx = S.get_context()
    lines = []
    for cname in args.cases.split(","):
        wtype, fsize, corners, masks = case(cname)
        est = S.SeamEstimator("voronoi")
        out = est.find(masks, corners, masks)  # warm-up: allocator, code objects
        ctx.sync()
        wall, dev, dev_copy = [], [], []
        for _ in range(max(5, args.steps)):
            t = time.perf_counter()
            out = est.find(masks, corners, masks)
            wall.append((time.perf_counter() - t) * 1e3)
            dev.append(est.info["device_ms"])
            dev_copy.append(est.info["device_ms_with_copy"])
        h_masks = [m.numpy() for m in masks]
        t = time.perf_counter()
        want = Z.find("voronoi", corners, h_masks)
        ref_ms = (time.perf_counter() - t) * 1e3
        equal = all(np.array_equal(o.numpy(), w) for o, w in zip(out, want))
        rec = {"case": cname, "warper": wtype, "frames": len(masks), "frame_size": list(fsize),
               "warped_mask_px": int(sum(m.width * m.height for m in masks)),
               "pairs": est.info["pairs"], "levels": est.info["levels"], "runs": len(wall),
               "device_ms_median": round(statistics.median(dev), 4),
               "device_ms_with_copy_median": round(statistics.median(dev_copy), 4),
               "call_wall_ms_median": round(statistics.median(wall), 4),
               "call_wall_ms_min": round(min(wall), 4),
               "restatement_cpu_ms": round(ref_ms, 1),
               "equal_to_restatement": equal,
               "kernel_source_hash": khash}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if args.out:
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
