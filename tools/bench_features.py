#!/usr/bin/env python
"""FeatureEstimator (the project's own corner detector and binary descriptor: csrc/stx_features.hip) on eight synthetic frames at the
reference's medium resolution (0.6 Mpx: 894 x 671), the images resident on the device.
usage: python tools/bench_features.py [--steps 20] [--out profiles/features.json]
Two JSON lines: the synthetic frames ("timing": smooth, few corners) and seeded smoothed noise of the same size ("timing_textured": corners
everywhere, the selection's heavy case).  detect_ms: a host clock around one detect() of the eight frames — it ends with the copy of
the results to the host, behind a stream synchronisation — after one warm-up call, `steps` calls, median / min / max, profiler off.  kernel_ms: the context profiler's
per-kernel events of one extra call.  equal_to_contract: frame 0 against tests/numpy_features.py.  --out merges the two lines
into the JSON file, whose other entries are kept.  There is no bar and no baseline: the numpy contract is not one."""
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
from stitching_amd import synthetic  # noqa: E402

MW, MH, FRAMES = 894, 671, 8  # 0.6 Mpx of a 4:3 frame


def smooth(a):
    """seeded noise, lightly smoothed: corners everywhere, the opposite of the smooth synthetic frames"""
    a = a.astype(np.uint16)
    return ((a + np.roll(a, 1, 0) + np.roll(a, 1, 1) + np.roll(a, (1, 1), (0, 1)) + 2) // 4).astype(np.uint8)


def measure(ctx, case, frames, steps, N, khash):
    imgs = [S.DeviceImage.from_numpy(f, ctx) for f in frames]
    est = S.FeatureEstimator()
    est.detect(imgs)  # warm-up: allocator, code objects
    ms = []
    for _ in range(steps):
        ctx.sync()
        t0 = time.perf_counter()
        out = est.detect(imgs)
        ms.append((time.perf_counter() - t0) * 1e3)
    ctx.prof_reset()
    ctx.prof_enable(True)
    est.detect(imgs)
    ctx.sync()
    prof = {e["kernel"]: {"calls": e["calls"], "total_ms": round(e["total_ms"], 4)} for e in ctx.prof_results()
            if e["kernel"].startswith("feat_") or e["kernel"] == "resize_linear_exact_batch"}
    ctx.prof_enable(False)
    want = N.detect(frames[0])
    equal = all(np.array_equal(getattr(out[0], k), want[k]) for k in ("level", "x", "y", "bin", "R", "descriptors"))
    return {"case": case, "frames": len(frames), "frame_size": [MW, MH],
            "parameters": {"nfeatures": est.nfeatures, "nlevels": est.nlevels, "scale": est.scale, "fast_threshold": est.fast_threshold},
            "detect_ms": {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}, "runs": len(ms),
            "kernel_ms": prof, "kernel_ms_sum": round(sum(v["total_ms"] for v in prof.values()), 4), "levels": est.info["levels"],
            "candidates": est.info["candidates"], "keypoints": est.info["keypoints"], "equal_to_contract": bool(equal),
            "how": "detect_ms: host clock around one detect() of 8 device-resident frames (ends behind a stream synchronisation), after one "
                   "warm-up call, profiler off; kernel_ms: the context profiler's per-kernel events of one extra call",
            "kernel_source_hash": khash}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None, help="merge the lines into this JSON file as its \"timing\" and \"timing_textured\" entries")
    args = ap.parse_args()
    import bench
    from tests import numpy_features as N

    ctx = S.get_context()
    rs = np.random.RandomState(0)
    cases = {"timing": ("medium_8_frames", synthetic.make_frames(range(FRAMES), MW, MH)),
             "timing_textured": ("medium_8_frames_noise", [smooth(rs.randint(0, 256, (MH, MW, 3))) for _ in range(FRAMES)])}
    doc = {}
    if args.out and os.path.exists(args.out):
        with open(args.out) as f:
            doc = json.load(f)
    for key, (case, frames) in cases.items():
        doc[key] = measure(ctx, case, frames, max(5, args.steps), N, bench.kernel_source_hash())
        print(json.dumps(doc[key]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
