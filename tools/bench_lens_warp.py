#!/usr/bin/env python
"""The warp through the lens (StitchJob with lenses, stx_warp_lens_batch) beside rectify-then-warp, as the steady state of a known rig:
BASELINE config 2 (8 BGR frames of 4000 x 3000 in device memory, one ring, spherical warper, 5-band blender), every frame through the
bench lens of tools/bench_rectify.py (fit="inside").
usage: python tools/bench_lens_warp.py [--steps 50] [--warmup 5] [--out profiles/lens_warp.json] [--frames 8] [--size 4000x3000]
Two legs, INTERLEAVED call by call in one process — the yardstick is leg (a) of the same run, never an earlier file:
  (a) rectify_then_warp: rectify_all(distorted) then job.run(frames=rectified) on a job over rectified frames;
  (b) fused:             job.run(frames=distorted) on a job with lenses.
One JSON line per leg: medians of --steps calls with the run-to-run spread (min, max).  device_ms: HIP events on the context's stream
around the whole panorama; kernels: per kernel the launch's own events per panorama (the context's profiler, a run of its own), the bytes
the pass has to move and their fraction of 8 TB/s.  The summary line holds the ratios and whether the two spreads overlap."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import stitching_amd as S  # noqa: E402
from stitching_amd import synthetic  # noqa: E402
from stitching_amd.pipeline import StitchJob  # noqa: E402
from tools.bench_rectify import PEAK_BYTES_PER_MS, bench_lens, q  # noqa: E402


def kernels(ctx, fn, steps, names):
    """per panorama: {kernel: {kernel_ms, algo_bytes, fraction_of_peak, launches}} of the named kernels, from `steps` profiled calls"""
    ctx.sync()
    ctx.prof_enable()
    ctx.prof_reset()
    for _ in range(steps):
        out = fn()
        ctx.sync()
        del out
    res = {r["kernel"]: r for r in ctx.prof_results() if r["calls"]}
    ctx.prof_enable(False)
    out = {}
    for name in names:
        r = res[name]
        ms, by = r["total_ms"] / steps, r["algo_bytes"] / steps
        out[name] = {"kernel_ms": round(ms, 4), "algo_bytes": by, "fraction_of_peak": round(by / ms / PEAK_BYTES_PER_MS, 4),
                     "launches": r["calls"] / steps}
    out["all_kernels_ms"] = round(sum(r["total_ms"] for r in res.values()) / steps, 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--size", default="4000x3000")
    ap.add_argument("--bands", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()
    import bench

    ctx = S.get_context()
    w, h = (int(v) for v in args.size.split("x"))
    n = args.frames
    rng = np.random.default_rng(1)
    host = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(2)]
    distorted = [S.DeviceImage.from_numpy(host[i % 2], ctx) for i in range(n)]
    lenses = [bench_lens(i, w, h, fit="inside") for i in range(n)]
    cams = synthetic.ring_cameras(n, w, h, focal_factor=0.75)
    kw = dict(warper_type="spherical", blender_type="multiband", num_bands=args.bands, ctx=ctx)
    job_a = StitchJob(S.rectify_all(distorted, lenses, ctx=ctx), cams, **kw)
    job_b = StitchJob(distorted, cams, lenses=lenses, **kw)

    def leg_a():
        return job_a.run(frames=S.rectify_all(distorted, lenses, ctx=ctx))

    def leg_b():
        return job_b.run(frames=distorted)

    legs = {"rectify_then_warp": leg_a, "fused": leg_b}
    for fn in legs.values():  # the first run of either rig makes its geometry
        fn()
    ctx.sync()
    assert np.array_equal(np.asarray(job_a.run()[1]), np.asarray(job_b.run()[1])), "the two jobs' panorama masks differ"
    for _ in range(args.warmup):
        for fn in legs.values():
            out = fn()
            ctx.sync()
            del out
    dev = {k: [] for k in legs}
    for _ in range(args.steps):
        for k, fn in legs.items():
            ctx.sync()
            ctx.mark(0)
            out = fn()
            ctx.mark(1)
            ctx.sync()
            dev[k].append(ctx.elapsed_ms(0, 1))
            del out
    assert job_a.last_reused and job_b.last_reused
    base = {"frames": n, "frame_size": [w, h], "bands": job_a.last_num_bands, "warper": "spherical", "runs": args.steps, "warmup": args.warmup,
            "interleaved": True, "kernel_source_hash": bench.kernel_source_hash(),
            "lens": {"model": "brown", "fit": "inside", "focal_factor": round(float(lenses[0].new_K[0, 0] / (0.6 * w)), 4)}}
    lines = [dict(base, case="rectify_then_warp", device_ms=q(dev["rectify_then_warp"]),
                  kernels=kernels(ctx, leg_a, args.steps, ["rectify", "warp_img"]),
                  intermediate_bytes=6.0 * n * w * h, note="rectified frames written once and read once between the two passes"),
             dict(base, case="fused", device_ms=q(dev["fused"]), kernels=kernels(ctx, leg_b, args.steps, ["warp_lens_img"]), intermediate_bytes=0.0)]
    a, b = lines[0], lines[1]
    resample_a = a["kernels"]["rectify"]["kernel_ms"] + a["kernels"]["warp_img"]["kernel_ms"]
    resample_b = b["kernels"]["warp_lens_img"]["kernel_ms"]
    lines.append(dict(base, case="summary",
                      fused_over_rectify_then_warp_device=round(b["device_ms"]["median"] / a["device_ms"]["median"], 3),
                      spreads_overlap=not (b["device_ms"]["max"] < a["device_ms"]["min"] or a["device_ms"]["max"] < b["device_ms"]["min"]),
                      resampling_kernels_ms={"rectify_then_warp": round(resample_a, 4), "fused": round(resample_b, 4)},
                      fused_over_rectify_then_warp_kernels=round(resample_b / resample_a, 3),
                      not_measured=["hardware counters", "strongly minifying lenses", "the per-pixel projector families", "other rigs than config 2"]))
    for rec in lines:
        print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
