#!/usr/bin/env python
"""The low-resolution pass and the cropped composition (stitching_amd.Composer) on BASELINE config 2 (8 frames of 4000 x 3000, one
spherical ring) and config 4 (64 frames of 8000 x 6000, 16 x 4 cylindrical grid).
usage: python tools/bench_low_pass.py [--steps 20] [--out profiles/low_pass.json] [--cases resize,prepare,run] [--configs 2,4]
One JSON line per measurement, medians of --steps calls with the run-to-run spread (min, max); device time by HIP events on the
context's stream (from the first launch of a call to its last: host gaps inside a call count).
  resize  : the LOW resize (frames -> 0.1 Mpx) as one stx_resize_linear_exact_batch launch against the loop over
            stx_resize_linear_exact, the same device-resident frames, in the same run
  prepare : Composer.prepare (finder "voronoi", the other settings at their defaults)
  run     : Composer.run at config 2 with the cropper and with crop=False, and the ratio of the warped pixels
Frame contents do not matter to any timing here: config 4 uploads 8 distinct synthetic frames 8 times each (64 separate buffers)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import stitching_amd as S  # noqa: E402
from stitching_amd import synthetic  # noqa: E402
from stitching_amd.pipeline import clip_rectangle  # noqa: E402
from stitching_amd.seam_finder import resize_linear_exact, resize_linear_exact_all  # noqa: E402

R = S.Images.Resolution


def rig(cfg, ctx):
    """device-resident frames and the cameras at MEDIUM scale"""
    n, (w, h), wtype = (8, (4000, 3000), "spherical") if cfg == 2 else (64, (8000, 6000), "cylindrical")
    host = synthetic.make_frames(range(min(n, 8)), w, h)
    frames = [S.DeviceImage.from_numpy(host[i % len(host)], ctx) for i in range(n)]
    images = S.Images.of(frames)
    mw, mh = images.get_scaled_img_sizes(R.MEDIUM)[0]
    cams = synthetic.ring_cameras(n, mw, mh, focal_factor=0.75) if cfg == 2 else \
        synthetic.grid_cameras(16, 4, mw, mh, max_edge_lat_deg=50.0, layout_yaw=16)
    return frames, cams, wtype, images


def warped_px(ctx, wtype, plan, crop):
    """pixels of the final warps: whole, or the cropper's rectangles clipped as the job clips them (the seam-cell crops of the
    multi-band blender cut both further)"""
    wp = S.Warper(wtype, ctx=ctx)
    wp.set_scale(plan.cameras)
    _, sizes = wp.warp_rois(plan.images.get_scaled_img_sizes(R.FINAL), plan.cameras, plan.camera_aspect)
    if not crop:
        return int(sum(w * h for w, h in sizes))
    cuts = [clip_rectangle(r.times(plan.lir_aspect), w, h) for r, (w, h) in zip(plan.cropper.intersection_rectangles, sizes)]
    return int(sum((x1 - x0) * (y1 - y0) for x0, x1, y0, y1 in cuts))


def timed(ctx, fn, steps):
    fn()
    ctx.sync()
    wall, dev = [], []
    for _ in range(steps):
        ctx.sync()
        t = time.perf_counter()
        ctx.mark(0)
        out = fn()
        ctx.mark(1)
        ctx.sync()
        wall.append((time.perf_counter() - t) * 1e3)
        dev.append(ctx.elapsed_ms(0, 1))
        del out
    q = lambda v: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}  # noqa: E731
    return {"wall_ms": q(wall), "device_ms": q(dev), "runs": steps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--cases", default="resize,prepare,run")
    ap.add_argument("--configs", default="2,4")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()
    import bench

    khash = bench.kernel_source_hash()
    ctx = S.get_context()
    cases, lines = args.cases.split(","), []

    def emit(rec):
        rec["kernel_source_hash"] = khash
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    for cfg in (int(c) for c in args.configs.split(",")):
        frames, cams, wtype, images = rig(cfg, ctx)
        low = images.get_scaled_img_sizes(R.LOW)
        base = {"config": cfg, "frames": len(frames), "frame_size": [frames[0].width, frames[0].height], "low_size": list(low[0])}
        if "resize" in cases:
            loop = timed(ctx, lambda: [resize_linear_exact(f, z, ctx=ctx, device_resident=True) for f, z in zip(frames, low)], args.steps)
            batch = timed(ctx, lambda: resize_linear_exact_all(frames, low, ctx=ctx, device_resident=True), args.steps)
            emit(dict(base, case="resize_low", loop=loop, batch=batch,
                      wall_ratio_loop_over_batch=round(loop["wall_ms"]["median"] / batch["wall_ms"]["median"], 3),
                      device_ratio_loop_over_batch=round(loop["device_ms"]["median"] / batch["device_ms"]["median"], 3)))
        comp = S.Composer(ctx=ctx, warper_type=wtype, finder="voronoi")
        if "prepare" in cases:
            try:
                emit(dict(base, case="composer_prepare", warper=wtype, **timed(ctx, lambda: comp.prepare(frames, cams), max(5, args.steps // 4))))
            except S.StitchingError as e:
                emit(dict(base, case="composer_prepare", warper=wtype, error=str(e)))
        if "run" in cases and cfg == 2:
            rec = dict(base, case="composer_run", warper=wtype)
            for label, crop in (("cropped", True), ("whole", False)):
                c = S.Composer(ctx=ctx, warper_type=wtype, finder="voronoi", crop=crop)
                plan = c.prepare(frames, cams)
                rec[label] = timed(ctx, lambda: c.run(plan), args.steps)
                rec[label]["warped_px"] = warped_px(ctx, wtype, plan, crop)
            rec["device_ratio_cropped_over_whole"] = round(rec["cropped"]["device_ms"]["median"] / rec["whole"]["device_ms"]["median"], 3)
            rec["pixel_ratio_cropped_over_whole"] = round(rec["cropped"]["warped_px"] / rec["whole"]["warped_px"], 3)
            emit(rec)
        del frames
    if args.out:
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
