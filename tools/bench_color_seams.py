#!/usr/bin/env python
"""ColorSeamEstimator (the project's own colour-aware seams: csrc/stx_color_seams.hip) on BASELINE config 2's eight frames (one spherical
ring) and config 4's 64 frames (16 x 4 cylindrical grid) at the reference's low resolution (0.1 Mpx: 365 x 274 frames), with
SeamEstimator("voronoi") on the same device-resident inputs beside it as context, and one pair of equal roi area as a vertical and as a
horizontal seam (the horizontal one reads its images with strided loads).
usage: python tools/bench_color_seams.py [--steps 20] [--out profiles/color_seams.json] [--cases config2_low,config4_low,orientation]
One JSON line per case.  device_ms is info["device_ms"] of a find() call: HIP events on the stream around the launches of all levels,
after the copy of the input masks (device_ms_with_copy includes it); inputs are DeviceImages, one warm-up call, then `steps` calls, median /
min / max.  kernel_ms: the profiler's per-kernel split of one extra call.  equal_to_contract: the result against
tests/numpy_color_seams.py."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import stitching_amd as S  # noqa: E402
from stitching_amd import config, synthetic  # noqa: E402

LW, LH = 365, 274  # 0.1 Mpx of a 4:3 frame


def warped(cams, wtype):
    frames = synthetic.make_frames(range(len(cams)), LW, LH)
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
    return [tuple(int(v) for v in c) for c in corners], imgs, masks


def pair(transpose, ctx):
    """two 365 x 274 images 65 apart (a 300 x 274 roi, vertical seam) or the same transposed (horizontal)"""
    rng = np.random.default_rng(0)
    imgs = [rng.integers(0, 256, (LH, LW, 3), dtype=np.uint8) for _ in range(2)]
    masks = [np.full((LH, LW), 255, np.uint8) for _ in range(2)]
    corners = [(0, 0), (65, 0)]
    if transpose:
        imgs, masks = [np.ascontiguousarray(a.transpose(1, 0, 2)) for a in imgs], [m.T.copy() for m in masks]
        corners = [(y, x) for x, y in corners]
    return corners, [S.DeviceImage.from_numpy(a, ctx) for a in imgs], [S.DeviceImage.from_numpy(m, ctx) for m in masks]


def stats(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def measure(est, imgs, corners, masks, steps, ctx, prefix):
    est.find(imgs, corners, masks)  # warm-up: allocator, code objects
    dev, with_copy = [], []
    for _ in range(steps):
        est.find(imgs, corners, masks)
        dev.append(est.info["device_ms"])
        with_copy.append(est.info["device_ms_with_copy"])
    ctx.prof_reset()
    ctx.prof_enable(True)
    out = est.find(imgs, corners, masks)
    ctx.sync()
    prof = {e["kernel"]: {"calls": e["calls"], "total_ms": round(e["total_ms"], 4)} for e in ctx.prof_results() if e["kernel"].startswith(prefix)}
    ctx.prof_enable(False)
    return {"device_ms": stats(dev), "device_ms_with_copy": stats(with_copy), "kernel_ms": prof, "pairs": est.info["pairs"],
            "levels": est.info["levels"], "runs": steps}, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--cases", default="config2_low,config4_low,orientation")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()
    import bench
    from tests import numpy_color_seams as Z

    khash = bench.kernel_source_hash()
    ctx = S.get_context()
    steps = max(5, args.steps)
    lines = []

    def equal(out, imgs, corners, masks):
        want = Z.find([a.numpy() for a in imgs], corners, [m.numpy() for m in masks])
        return all(np.array_equal(o.numpy(), w) for o, w in zip(out, want))

    for cname in args.cases.split(","):
        if cname == "orientation":
            rec = {"case": cname, "roi": [300, 274]}
            for label, transpose in (("vertical", False), ("horizontal", True)):
                corners, imgs, masks = pair(transpose, ctx)
                rec[label], out = measure(S.ColorSeamEstimator(), imgs, corners, masks, steps, ctx, "color_seam_")
                rec[label]["equal_to_contract"] = equal(out, imgs, corners, masks)
            rec["device_ratio_horizontal_over_vertical"] = round(rec["horizontal"]["device_ms"]["median"] / rec["vertical"]["device_ms"]["median"], 3)
        else:
            if cname == "config2_low":
                cams, wtype = synthetic.ring_cameras(8, LW, LH, focal_factor=0.75), "spherical"
            elif cname == "config4_low":
                cams, wtype = synthetic.grid_cameras(16, 4, LW, LH, max_edge_lat_deg=50.0, layout_yaw=16), "cylindrical"
            else:
                raise SystemExit(f"unknown case {cname}")
            corners, imgs, masks = warped(cams, wtype)
            rec = {"case": cname, "warper": wtype, "frames": len(cams), "frame_size": [LW, LH]}
            rec["color"], out = measure(S.ColorSeamEstimator(), imgs, corners, masks, steps, ctx, "color_seam_")
            rec["color"]["equal_to_contract"] = equal(out, imgs, corners, masks)
            rec["voronoi"], _ = measure(S.SeamEstimator("voronoi"), imgs, corners, masks, steps, ctx, "seam_")
        rec["how"] = ("device_ms: HIP events around the launches of all levels of one find() on device-resident inputs, after one warm-up "
                      "call; kernel_ms: the context profiler's per-kernel events of one extra call")
        rec["kernel_source_hash"] = khash
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if args.out:
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
