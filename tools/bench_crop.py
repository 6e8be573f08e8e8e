#!/usr/bin/env python
"""The largest interior rectangle (stx_crop_lir: contour counts + rectangle) on the panorama masks of three cases: BASELINE config 2
(8 frames, one spherical ring) and config 4's 64 frames (16 x 4 cylindrical grid) at the reference's low resolution (0.1 Mpx: 365 x 274
frames), and config 2 at full resolution (4000 x 3000 frames).  The masks come from Blender.create_panorama with device residency on,
so they are DeviceImages.
usage: python tools/bench_crop.py [--steps 20] [--out profiles/crop_lir.json] [--cases config2_low,config4_low,config2_full]
One JSON line per case: the mask size, the device time of the launches (HIP events, median), the per-kernel split (profiler, one extra
run), the whole call's wall time (median), the restatement's CPU time (tests/numpy_lir.py lir + single_contour, one run), whether the
rectangle and both counts equal the restatement's, kernel_source_hash."""
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
from stitching_amd.cropper import largest_interior_rectangle  # noqa: E402

LW, LH = 365, 274  # 0.1 Mpx of a 4:3 frame


def case(name):
    if name == "config2_low":
        cams, wtype, w, h = synthetic.ring_cameras(8, LW, LH, focal_factor=0.75), "spherical", LW, LH
    elif name == "config4_low":
        cams, wtype, w, h = synthetic.grid_cameras(16, 4, LW, LH, max_edge_lat_deg=50.0, layout_yaw=16), "cylindrical", LW, LH
    elif name == "config2_full":
        cams, wtype, w, h = synthetic.ring_cameras(8, 4000, 3000, focal_factor=0.75), "spherical", 4000, 3000
    else:
        raise SystemExit(f"unknown case {name}")
    frames = synthetic.make_frames(range(len(cams)), w, h)
    prev = config.device_resident()
    config.set_device_resident(True)
    try:
        wp = S.Warper(wtype)
        wp.set_scale(cams)
        sizes = [(w, h)] * len(cams)
        imgs = list(wp.warp_images(frames, cams))
        masks = list(wp.create_and_warp_masks(sizes, cams))
        corners, wsizes = wp.warp_rois(sizes, cams)
        mask = S.Cropper.estimate_panorama_mask(imgs, masks, corners, wsizes)
    finally:
        config.set_device_resident(prev)
    return wtype, len(cams), (w, h), mask


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--cases", default="config2_low,config4_low,config2_full")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()
    import bench
    from tests import numpy_lir as Z

    khash = bench.kernel_source_hash()
    ctx = S.get_context()
    lines = []
    for cname in args.cases.split(","):
        wtype, n, fsize, mask = case(cname)
        got = largest_interior_rectangle(mask)  # warm-up: allocator, code objects
        wall, dev = [], []
        for _ in range(max(5, args.steps)):
            t = time.perf_counter()
            got = largest_interior_rectangle(mask)
            wall.append((time.perf_counter() - t) * 1e3)
            dev.append(got[2])
        ctx.prof_reset()
        ctx.prof_enable(True)
        largest_interior_rectangle(mask)
        ctx.sync()
        prof = {e["kernel"]: round(e["total_ms"], 4) for e in ctx.prof_results() if e["kernel"].startswith("crop_")}
        ctx.prof_enable(False)
        host = mask.numpy()
        t = time.perf_counter()
        want = (Z.lir(host), Z.single_contour(host))
        ref_ms = (time.perf_counter() - t) * 1e3
        rec = {"case": cname, "warper": wtype, "frames": n, "frame_size": list(fsize), "mask_size": [mask.width, mask.height],
               "rect_xywh": list(got[0]), "contours": list(got[1]), "runs": len(wall),
               "device_ms_median": round(statistics.median(dev), 4),
               "kernel_ms": prof,
               "call_wall_ms_median": round(statistics.median(wall), 4),
               "call_wall_ms_min": round(min(wall), 4),
               "restatement_cpu_ms": round(ref_ms, 1),
               "equal_to_restatement": (got[0], got[1]) == want,
               "kernel_source_hash": khash}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if args.out:
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
