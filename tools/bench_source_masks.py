#!/usr/bin/env python
"""Source validity masks (stitching_amd.with_validity) on the frames of BASELINE config 2: 8 BGR frames of
4000 x 3000 in device memory, spherical warper.  The first-run warp launch of a rig (image + mask into the ROIs, one launch of the tuned
kernel) WITHOUT masks, with binary disc masks and with grey masks — the three alternate call by call in one process, so they share
whatever else the machine is doing; the yardstick is the unmasked launch of the same run.  Then stx_mask_shrink_batch of the eight
masks to the LOW size of the pipeline (0.1 megapixels).
usage: python tools/bench_source_masks.py [--steps 50] [--warmup 5] [--out profiles/source_masks.json] [--frames 8] [--size 4000x3000]
One JSON line per case: kernel_ms is the launch's own begin / end stamps (the context's profiler, stx_prof_*), median with the
run-to-run spread (min, max) of --steps calls; algo_bytes: what the launch has to move (the source once, image and mask once, a
validity mask once: at most sw x sh more bytes per image); the summary line holds the ratios to the unmasked launch."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import stitching_amd as S  # noqa: E402
from stitching_amd import synthetic  # noqa: E402

PEAK_BYTES_PER_MS = 8.0e9  # 8 TB/s
LOW_MEGAPIX = 0.1


def q(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def one_kernel(ctx, fn, name):
    """(kernel ms, declared algorithmic bytes) of the one launch called `name` that fn() makes"""
    ctx.prof_reset()
    out = fn()
    ctx.sync()
    res = {r["kernel"]: r for r in ctx.prof_results() if r["calls"]}
    del out
    assert name in res and res[name]["calls"] == 1, res
    return res[name]["total_ms"], res[name]["algo_bytes"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--size", default="4000x3000")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()
    import bench

    khash = bench.kernel_source_hash()
    ctx = S.get_context()
    w, h = (int(v) for v in args.size.split("x"))
    n, lines = args.frames, []
    base = {"frames": n, "frame_size": [w, h], "kernel_source_hash": khash, "runs": args.steps, "warmup": args.warmup}

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    rng = np.random.default_rng(1)
    host = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(2)]
    frames = [S.DeviceImage.from_numpy(host[i % 2], ctx) for i in range(n)]
    del host
    cams = synthetic.ring_cameras(n, w, h, focal_factor=0.75)
    yy, xx = np.mgrid[0:h, 0:w]
    disc = np.where((xx - w / 2.0) ** 2 + (yy - h / 2.0) ** 2 <= (0.58 * w) ** 2, 255, 0).astype(np.uint8)  # a circular image: corners cut
    grey = (1 + (7 * xx + 13 * yy) % 251).astype(np.uint8)
    del yy, xx
    d_disc, d_grey = S.DeviceImage.from_numpy(disc, ctx), S.DeviceImage.from_numpy(grey, ctx)
    variants = {"none": frames, "binary_disc": [S.with_validity(f, d_disc) for f in frames], "grey": [S.with_validity(f, d_grey) for f in frames]}
    warper = S.Warper("spherical", ctx=ctx)
    warper.set_scale(cams)
    arrays = warper.camera_arrays(cams)
    corners, sizes = warper.warp_rois([(w, h)] * n, cams, camera_arrays=arrays)
    rects = [tuple(c) + tuple(z) for c, z in zip(corners, sizes)]
    prev = S.device_resident()
    S.set_device_resident(True)
    ctx.prof_enable()
    try:
        def warp(srcs):
            return warper.warp_images_and_masks(srcs, cams, rects=rects, camera_arrays=arrays)

        for _ in range(args.warmup):
            for srcs in variants.values():
                one_kernel(ctx, lambda: warp(srcs), "warp_img_mask")
        ms = {k: [] for k in variants}
        declared = {}
        for _ in range(args.steps):
            for k, srcs in variants.items():  # alternating: every variant sees the same stretch of the machine's time
                t, declared[k] = one_kernel(ctx, lambda: warp(srcs), "warp_img_mask")
                ms[k].append(t)
        out_px = float(sum(r[2] * r[3] for r in rects))
        recs = {}
        for k in variants:
            algo = n * 3.0 * w * h + 4.0 * out_px + (0.0 if k == "none" else n * 1.0 * w * h)
            med = statistics.median(ms[k])
            recs[k] = dict(base, case=f"warp_img_mask_{k}", kernel="warp_img_mask", kernel_ms=q(ms[k]), algo_bytes=algo,
                           declared_algo_bytes=declared[k], tb_per_s=round(algo / med / 1e9, 3),
                           fraction_of_peak=round(algo / med / PEAK_BYTES_PER_MS, 4))
            emit(recs[k])
        # the eight masks to the LOW size
        scale = min(1.0, (LOW_MEGAPIX * 1e6 / (w * h)) ** 0.5)
        low = (int(round(w * scale)), int(round(h * scale)))
        for _ in range(args.warmup):
            one_kernel(ctx, lambda: S.shrink_masks_all([d_disc] * n, [low] * n), "mask_shrink_batch")
        sm = [one_kernel(ctx, lambda: S.shrink_masks_all([d_disc] * n, [low] * n), "mask_shrink_batch") for _ in range(args.steps)]
        algo = n * (1.0 * w * h + 1.0 * low[0] * low[1])
        med = statistics.median([t for t, _ in sm])
        emit(dict(base, case="mask_shrink_batch_to_low", kernel="mask_shrink_batch", low_size=list(low), kernel_ms=q([t for t, _ in sm]),
                  algo_bytes=algo, declared_algo_bytes=sm[0][1], tb_per_s=round(algo / med / 1e9, 3),
                  fraction_of_peak=round(algo / med / PEAK_BYTES_PER_MS, 4)))
        none = recs["none"]["kernel_ms"]["median"]
        emit(dict(base, case="summary", unmasked_kernel_ms=none,
                  binary_disc_over_unmasked=round(recs["binary_disc"]["kernel_ms"]["median"] / none, 4),
                  grey_over_unmasked=round(recs["grey"]["kernel_ms"]["median"] / none, 4),
                  extra_bytes_per_image=w * h, mask_shrink_kernel_ms=round(med, 4)))
    finally:
        ctx.prof_enable(False)
        S.set_device_resident(prev)
    if args.out:
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
