#!/usr/bin/env python
"""Device frame emit (stitching_amd.emit, one stx_emit launch per call) on one panorama of the size of BASELINE config 2's
(17852 x 2984 u8 BGR, random pixels) and its mask: as NV12 and I420 into surfaces with 256-byte-aligned pitches, as BGRA with the
mask as alpha and as a plain BGR copy, all in place into device memory of the tool's own — beside DeviceImage.numpy of the same
panorama into page-locked host memory, the only way out before emit existed.
usage: python tools/bench_emit.py [--steps 20] [--out profiles/emit.json] [--size 17852x2984]
One JSON line per case: medians of --steps calls with the run-to-run spread (min, max).  device_ms: HIP events on the context's
stream around the call; kernel_ms: the launch's own events (the context's profiler, a run of its own); algo_bytes: what the
conversion has to move (the source and the alpha image once, the target planes once); fraction_of_peak: algo_bytes / kernel time
over 8 TB/s."""
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

PEAK_BYTES_PER_MS = 8.0e9  # 8 TB/s


class Surface:
    """device memory of the tool's own behind `__cuda_array_interface__`: `rows` rows of `shape[1:]` u8, `pitch` bytes apart"""

    def __init__(self, ctx, shape, pitch):
        self.owner = S.DeviceImage.from_numpy(np.zeros((1, shape[0] * pitch), np.uint8), ctx)
        packed = np.empty((1,) + tuple(shape[1:]), np.uint8).strides[1:]
        self.__cuda_array_interface__ = {"version": 3, "shape": tuple(shape), "typestr": "|u1", "data": (self.owner.device_ptr(), False),
                                         "strides": (pitch,) + packed}


def q(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def timed(ctx, fn, steps):
    """wall and device time of fn() (which only queues work)"""
    fn()
    ctx.sync()
    wall, dev = [], []
    for _ in range(steps):
        ctx.sync()
        t = time.perf_counter()
        ctx.mark(0)
        fn()
        ctx.mark(1)
        ctx.sync()
        wall.append((time.perf_counter() - t) * 1e3)
        dev.append(ctx.elapsed_ms(0, 1))
    return {"wall_ms": q(wall), "device_ms": q(dev), "runs": steps}


def kernel_time(ctx, fn, steps):
    ctx.sync()
    ctx.prof_enable()
    ctx.prof_reset()
    for _ in range(steps):
        fn()
        ctx.sync()
    res = {r["kernel"]: r for r in ctx.prof_results() if r["calls"]}
    ctx.prof_enable(False)
    return res


def up256(v):
    return (v + 255) // 256 * 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--size", default="17852x2984")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()
    import bench

    khash = bench.kernel_source_hash()
    ctx = S.get_context()
    w, h = (int(v) for v in args.size.split("x"))
    cw, ch = (w + 1) // 2, (h + 1) // 2
    lines = []
    rng = np.random.default_rng(1)
    px = float(w) * h
    base = {"panorama_size": [w, h], "kernel_source_hash": khash}
    host = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    pano = S.DeviceImage.from_numpy(host, ctx)
    mask = S.DeviceImage.from_numpy(rng.integers(0, 2, (h, w), dtype=np.uint8) * 255, ctx)

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    def case(name, fmt, target, algo_bytes, alpha=None, **more):
        fn = lambda: S.emit(pano, fmt, out=target, alpha=alpha, wait=False, ctx=ctx)  # noqa: E731
        rec = dict(base, case=name, format=fmt, algo_bytes=algo_bytes, **more, **timed(ctx, fn, args.steps))
        k = kernel_time(ctx, fn, args.steps)
        assert list(k) == ["emit"] and k["emit"]["calls"] == args.steps, k  # one launch per call
        ms = k["emit"]["total_ms"] / args.steps
        rec["kernel_ms"] = round(ms, 4)
        rec["declared_algo_bytes"] = k["emit"]["algo_bytes"] / args.steps
        rec["fraction_of_peak"] = round(algo_bytes / ms / PEAK_BYTES_PER_MS, 4)
        rec["tb_per_s"] = round(algo_bytes / ms / 1e9, 3)
        emit(rec)
        return rec

    yuv_bytes = px * 4.0 + 2.0 * cw * ch
    ypitch, uvpitch, cpitch = up256(w), up256(2 * cw), up256(cw)
    r_nv12 = case("nv12_pitch256", "nv12", (Surface(ctx, (h, w), ypitch), Surface(ctx, (ch, cw, 2), uvpitch)), yuv_bytes, y_pitch=ypitch,
                  uv_pitch=uvpitch)
    case("i420_pitch256", "i420", (Surface(ctx, (h, w), ypitch), Surface(ctx, (ch, cw), cpitch), Surface(ctx, (ch, cw), cpitch)), yuv_bytes,
         y_pitch=ypitch, uv_pitch=cpitch)
    case("bgra_mask_alpha", "bgra", Surface(ctx, (h, w, 4), 4 * w), px * 8.0, alpha=mask)
    r_bgr = case("bgr", "bgr", Surface(ctx, (h, w, 3), up256(3 * w)), px * 6.0, pitch=up256(3 * w))
    # the way out before emit: the panorama read back into page-locked host memory
    pinned = S.pinned_empty((h, w, 3))
    down = timed(ctx, lambda: pano.numpy(out=pinned, wait=False), args.steps)
    emit(dict(base, case="numpy_pinned", bytes=px * 3.0, **down, gb_per_s=round(px * 3.0 / down["device_ms"]["median"] / 1e6, 2)))
    emit(dict(base, case="summary", nv12_over_bgr_fraction=round(r_nv12["fraction_of_peak"] / r_bgr["fraction_of_peak"], 3),
              numpy_over_nv12_emit=round(down["device_ms"]["median"] / r_nv12["device_ms"]["median"], 1)))
    if args.out:
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
