#!/usr/bin/env python
"""Lens rectification (stitching_amd.rectify_all, one stx_rectify launch per list) on the frames of BASELINE config 2: 8 BGR frames of
4000 x 3000 in device memory, each through the Brown lens of its own camera (fit="inside") — beside ingest_all of the same frames as
packed BGR in the same process: the plain copy, the project's own yardstick for one pass over the same bytes.
usage: python tools/bench_rectify.py [--steps 50] [--warmup 5] [--out profiles/rectify.json] [--frames 8] [--size 4000x3000]
One JSON line per case: medians of --steps calls with the run-to-run spread (min, max).  device_ms: HIP events on the context's
stream around the call; kernel_ms: the launch's own events (the context's profiler, a run of its own); algo_bytes: what the pass has
to move (the source once, the destination once); fraction_of_peak: algo_bytes / kernel time over 8 TB/s.  The summary line holds the
ratio of the two and LensMap.error() — what the 16-pixel grid costs, in pixels — of the bench lens and of the two lenses of
tests/test_rectify_contract.py."""
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
# the lenses of tests/test_rectify_contract.py (K, WIDE, FISH on 96 x 72 frames)
TEST_K = np.array([[70.0, 0.0, 47.3], [0.0, 70.0, 35.6], [0.0, 0.0, 1.0]])
TEST_BROWN, TEST_FISHEYE, TEST_SIZE = (-0.25, 0.06, 0.001, -0.0008, -0.01), (-0.03, 0.01, -0.004, 0.001), (96, 72)
BENCH_DIST = (-0.22, 0.05, 0.0004, -0.0003, -0.006)


class Surface:
    """device memory of the tool's own behind `__cuda_array_interface__` (tools/bench_ingest.py)"""

    def __init__(self, ctx, arr):
        self.owner = S.DeviceImage.from_numpy(arr.reshape(1, -1), ctx)
        self.__cuda_array_interface__ = {"version": 3, "shape": arr.shape, "typestr": "|u1", "data": (self.owner.device_ptr(), False),
                                         "strides": None}


def q(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def timed(ctx, fn, steps, warmup):
    for _ in range(warmup):
        out = fn()
        ctx.sync()
        del out
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
    return {"wall_ms": q(wall), "device_ms": q(dev), "runs": steps, "warmup": warmup}


def kernel_time(ctx, fn, steps, name):
    ctx.sync()
    ctx.prof_enable()
    ctx.prof_reset()
    for _ in range(steps):
        out = fn()
        ctx.sync()
        del out
    res = {r["kernel"]: r for r in ctx.prof_results() if r["calls"]}
    ctx.prof_enable(False)
    assert list(res) == [name] and res[name]["calls"] == steps, res  # one launch per list
    return res[name]["total_ms"] / steps, res[name]["algo_bytes"] / steps


def bench_lens(i, w, h, **kw):
    K = np.array([[0.6 * w, 0.0, w / 2.0 - 9.5 + 3.0 * i], [0.0, 0.6 * w, h / 2.0 + 7.25 - 2.0 * i], [0.0, 0.0, 1.0]])
    return S.LensMap.brown(K, BENCH_DIST, (w, h), **kw)


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
    rng = np.random.default_rng(1)
    px = float(n) * w * h
    base = {"frames": n, "frame_size": [w, h], "kernel_source_hash": khash}

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    def case(name, kernel, fn, algo_bytes, **more):
        rec = dict(base, case=name, algo_bytes=algo_bytes, **more, **timed(ctx, fn, args.steps, args.warmup))
        ms, declared = kernel_time(ctx, fn, args.steps, kernel)
        rec["kernel_ms"] = round(ms, 4)
        rec["declared_algo_bytes"] = declared
        rec["fraction_of_peak"] = round(algo_bytes / ms / PEAK_BYTES_PER_MS, 4)
        rec["tb_per_s"] = round(algo_bytes / ms / 1e9, 3)
        emit(rec)
        return rec

    host = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(2)]
    lenses = [bench_lens(i, w, h, fit="inside") for i in range(n)]
    frames = [S.DeviceImage.from_numpy(host[i % 2], ctx) for i in range(n)]
    r_rect = case("rectify_brown_inside", "rectify", lambda: S.rectify_all(frames, lenses, ctx=ctx), px * 6.0, border="constant", masks=False,
                  focal_factor=round(float(lenses[0].new_K[0, 0] / (0.6 * w)), 4))
    r_mask = case("rectify_brown_inside_masks", "rectify", lambda: S.rectify_all(frames, lenses, masks=True, ctx=ctx), px * 7.0,
                  border="constant", masks=True)
    del frames
    surfaces = [Surface(ctx, host[i % 2]) for i in range(n)]
    r_copy = case("ingest_bgr_plain_copy", "ingest", lambda: S.ingest_all(surfaces, format="bgr", wait=False, ctx=ctx), px * 6.0)
    del surfaces
    emit(dict(base, case="summary",
              rectify_kernel_ms=r_rect["kernel_ms"], plain_copy_kernel_ms=r_copy["kernel_ms"],
              rectify_over_plain_copy=round(r_rect["kernel_ms"] / r_copy["kernel_ms"], 3),
              rectify_fraction_of_peak=r_rect["fraction_of_peak"], plain_copy_fraction_of_peak=r_copy["fraction_of_peak"],
              rectify_with_masks_kernel_ms=r_mask["kernel_ms"],
              lens_error_px={"bench_brown_inside": round(lenses[0].error(), 5),
                             "test_brown": round(S.LensMap.brown(TEST_K, TEST_BROWN, TEST_SIZE).error(), 5),
                             "test_fisheye": round(S.LensMap.fisheye(TEST_K, TEST_FISHEYE, TEST_SIZE).error(), 5)}))
    if args.out:
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
