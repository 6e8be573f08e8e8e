#!/usr/bin/env python
"""Device frame ingest (stitching_amd.ingest_all, one stx_ingest launch per list) on the frames of BASELINE config 2: 8 frames of
4000 x 3000, as NV12 surfaces with 256-byte-aligned pitches, as packed BGR and as BGRA, all in device memory of the tool's own —
beside DeviceImage.from_numpy of the same frames from page-locked host memory, the only way in before ingest existed.
usage: python tools/bench_ingest.py [--steps 20] [--out profiles/ingest.json] [--frames 8] [--size 4000x3000]
One JSON line per case: medians of --steps calls with the run-to-run spread (min, max).  device_ms: HIP events on the context's
stream around the call; kernel_ms: the launch's own events (the context's profiler, a run of its own); algo_bytes: what the
conversion has to move (source planes once, BGR once); fraction_of_peak: algo_bytes / kernel time over 8 TB/s."""
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
    """device memory of the tool's own behind `__cuda_array_interface__`: rows `pitch` bytes apart in a flat u8 DeviceImage"""

    def __init__(self, ctx, arr, pitch):
        rows, row_bytes = arr.shape[0], arr[0].nbytes
        flat = np.zeros(rows * pitch, np.uint8)
        flat.reshape(rows, pitch)[:, :row_bytes] = arr.reshape(rows, row_bytes)
        self.owner = S.DeviceImage.from_numpy(flat.reshape(1, -1), ctx)
        self.__cuda_array_interface__ = {"version": 3, "shape": arr.shape, "typestr": "|u1", "data": (self.owner.device_ptr(), False),
                                         "strides": (pitch,) + arr.strides[1:]}


def q(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def timed(ctx, fn, steps):
    """wall and device time of fn() (which only queues work), then the kernel's own time in a profiled run"""
    del_out = fn()
    ctx.sync()
    del del_out
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
    return {"wall_ms": q(wall), "device_ms": q(dev), "runs": steps}


def kernel_time(ctx, fn, steps):
    ctx.sync()
    ctx.prof_enable()
    ctx.prof_reset()
    for _ in range(steps):
        out = fn()
        ctx.sync()
        del out
    res = {r["kernel"]: r for r in ctx.prof_results() if r["calls"]}
    ctx.prof_enable(False)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
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

    def case(name, fmt, frames, algo_bytes, **more):
        fn = lambda: S.ingest_all(frames, format=fmt, wait=False, ctx=ctx)  # noqa: E731
        rec = dict(base, case=name, format=fmt, algo_bytes=algo_bytes, **more, **timed(ctx, fn, args.steps))
        k = kernel_time(ctx, fn, args.steps)
        assert list(k) == ["ingest"] and k["ingest"]["calls"] == args.steps, k  # one launch per list
        ms = k["ingest"]["total_ms"] / args.steps
        rec["kernel_ms"] = round(ms, 4)
        rec["declared_algo_bytes"] = k["ingest"]["algo_bytes"] / args.steps
        rec["fraction_of_peak"] = round(algo_bytes / ms / PEAK_BYTES_PER_MS, 4)
        rec["tb_per_s"] = round(algo_bytes / ms / 1e9, 3)
        emit(rec)
        return rec

    pitch = (w + 255) // 256 * 256
    cw, ch = (w + 1) // 2, (h + 1) // 2
    cpitch = (2 * cw + 255) // 256 * 256
    one = [(rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (ch, cw, 2), dtype=np.uint8)) for _ in range(2)]
    nv12 = [(Surface(ctx, one[i % 2][0], pitch), Surface(ctx, one[i % 2][1], cpitch)) for i in range(n)]
    r_nv12 = case("nv12_pitch256", "nv12", nv12, px * 3.0 + n * (float(w) * h + 2.0 * cw * ch), y_pitch=pitch, uv_pitch=cpitch)
    del nv12
    host3 = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(2)]
    bgr = [Surface(ctx, host3[i % 2], w * 3) for i in range(n)]
    r_bgr = case("bgr", "bgr", bgr, px * 6.0)
    del bgr
    host4 = [rng.integers(0, 256, (h, w, 4), dtype=np.uint8) for _ in range(2)]
    bgra = [Surface(ctx, host4[i % 2], w * 4) for i in range(n)]
    case("bgra", "bgra", bgra, px * 7.0)
    del bgra, host4
    # the way in before ingest: page-locked host frames over the host link, copies queued and waited for once
    pinned = [S.pinned_empty((h, w, 3)) for _ in range(n)]
    for i, p in enumerate(pinned):
        np.copyto(p, host3[i % 2])
    up = timed(ctx, lambda: [S.DeviceImage.from_numpy(p, ctx, wait=False) for p in pinned], args.steps)
    emit(dict(base, case="from_numpy_pinned", bytes=px * 3.0, **up,
              gb_per_s=round(px * 3.0 / up["device_ms"]["median"] / 1e6, 2)))
    emit(dict(base, case="summary", nv12_over_bgr_fraction=round(r_nv12["fraction_of_peak"] / r_bgr["fraction_of_peak"], 3),
              from_numpy_over_nv12_ingest=round(up["device_ms"]["median"] / r_nv12["device_ms"]["median"], 1)))
    if args.out:
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
