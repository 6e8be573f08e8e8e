#!/usr/bin/env python
"""MatchEstimator (the project's own descriptor matcher and homography RANSAC: csrc/stx_matches.hip) on synthetic features with planted
counterparts: 8 images x 500 features and 64 images x 2000 features, every pair matched.
usage: python tools/bench_matches.py [--steps 10] [--out profiles/matches.json]
The features: landmarks along a strip with random 256-bit descriptors; an image sees a window of them that overlaps each neighbour's by
half, through its own translation, with a pixel of position noise, 3 % of the descriptor bits flipped and 15 % of the places wrong.
Per size one JSON line: match_ms, a host clock around one match() — uploads, the four launches, the copies back, the host's refits —
after one warm-up call, `steps` calls, median / min / max, profiler off; device_ms / device_ms_with_copy: the call's own HIP events
(median); kernel_ms: the context profiler's per-kernel events of one extra call, for both ways match_2nn can take the other image's
descriptors (through LDS tiles, the default, and STX_MATCH_TRAIN=uniform: wave-uniform loads).  At the small size also the numpy
contract's seconds and whether the device equals it.  --out merges the lines into the JSON file as "timing_<size>", next to "contract"
(tests/test_matches_contract.py's cases, measured here again on the CPU).  No target is set: this is the first measurement of this code."""
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

SIZES = {"8x500": (8, 500), "64x2000": (64, 2000)}


def scene(n, nf, seed=0):
    """n ImageFeatures of nf features each"""
    rs = np.random.RandomState(seed)
    total = (n + 1) * nf // 2
    D = rs.randint(0, 256, (total, 32)).astype(np.uint8)
    P = np.stack([rs.randint(0, 600, total) + np.arange(total) * 600 // nf, rs.randint(20, 780, total)], axis=1)  # 300 px of strip per image step
    feats = []
    for i in range(n):
        pick = rs.permutation(np.arange(i * nf // 2, i * nf // 2 + nf))
        d = D[pick] ^ np.packbits(rs.random_sample((nf, 256)) < 0.03, axis=1)
        xy = P[pick] - (i * 300, 0) + rs.randint(-1, 2, (nf, 2)) + (100, 0)
        wrong = rs.random_sample(nf) < 0.15  # outliers: the descriptor matches, the place does not
        xy[wrong] = np.stack([rs.randint(100, 1300, nf), rs.randint(20, 780, nf)], axis=1)[wrong]
        feats.append(S.ImageFeatures(i, (1400, 800), [(1400, 800)], np.zeros(nf, np.int32), xy[:, 0].astype(np.int32), xy[:, 1].astype(np.int32),
                                     np.zeros(nf, np.int32), np.zeros(nf, np.int64), np.ascontiguousarray(d)))
    return feats


def box():
    """the device's name as the HIP runtime gives it (hipDeviceProp_t begins with char name[256])"""
    import ctypes

    for path in ("libamdhip64.so", "/opt/rocm/lib/libamdhip64.so"):
        try:
            hip = ctypes.CDLL(path)
            fn = getattr(hip, "hipGetDevicePropertiesR0600", None) or hip.hipGetDeviceProperties
            buf = ctypes.create_string_buffer(16384)
            if fn(buf, 0) == 0:
                return {"device": buf.raw[:256].split(b"\0")[0].decode(), "note": "one GPU of a box shared with other jobs"}
        except (OSError, AttributeError):
            continue
    return {"device": "unknown", "note": "the HIP runtime did not name the device"}


def kernels(ctx, est, feats):
    ctx.prof_reset()
    ctx.prof_enable(True)
    est.match(feats, ctx=ctx)
    ctx.sync()
    prof = {e["kernel"]: round(e["total_ms"], 4) for e in ctx.prof_results() if e["kernel"].startswith("match_")}
    ctx.prof_enable(False)
    return prof


def measure(ctx, name, steps, with_contract, khash):
    n, nf = SIZES[name]
    feats = scene(n, nf)
    est = S.MatchEstimator()
    out = {"case": name, "images": n, "features_per_image": nf,
           "parameters": {"match_conf": est.match_conf, "range_width": est.range_width, "ransac_iters": est.ransac_iters,
                          "ransac_threshold": est.ransac_threshold}}
    for train in ("lds", "uniform"):
        os.environ["STX_MATCH_TRAIN"] = train
        got = est.match(feats, ctx=ctx)  # warm-up: allocator, code objects
        ms, dev, devc = [], [], []
        for _ in range(steps):
            ctx.sync()
            t0 = time.perf_counter()
            got = est.match(feats, ctx=ctx)
            ms.append((time.perf_counter() - t0) * 1e3)
            dev.append(est.info["device_ms"])
            devc.append(est.info["device_ms_with_copy"])
        out[f"train_{train}"] = {
            "match_ms": {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)},
            "device_ms": round(statistics.median(dev), 4), "device_ms_with_copy": round(statistics.median(devc), 4),
            "kernel_ms": kernels(ctx, est, feats)}
        if train == "lds":
            first = got
        else:
            out["variants_equal"] = all(np.array_equal(a.matches, b.matches) and np.array_equal(a.inliers_mask, b.inliers_mask)
                                        and a.hypothesis == b.hypothesis for a, b in zip(first, got))
    os.environ.pop("STX_MATCH_TRAIN")
    out.update({"runs": steps, "pairs": est.info["pairs"], "matches": est.info["matches"],
                "pairs_with_homography": sum(1 for e in first if e.H is not None and e.src_img_idx < e.dst_img_idx),
                "largest_confidence": round(max(e.confidence for e in first), 4)})
    if with_contract:
        from tests import numpy_matches as N

        t0 = time.perf_counter()
        want = N.match(feats)
        out["numpy_contract_s"] = round(time.perf_counter() - t0, 3)
        out["equal_to_contract"] = all(
            np.array_equal(g.matches, w["matches"]) and np.array_equal(g.inliers_mask, w["inliers_mask"]) and g.hypothesis == w["hypothesis"]
            and ((g.H_sample is None and w["H_sample"] is None) or np.array_equal(g.H_sample.view(np.uint64), w["H_sample"].view(np.uint64)))
            for g, w in zip(first, want))
    out["how"] = ("match_ms: host clock around one match() of host-resident features (uploads, four launches, copies back, host refits), "
                  "after one warm-up call, profiler off; device_ms: HIP events around the four launches, with_copy: around uploads, launches "
                  "and copies back; kernel_ms: the context profiler's per-kernel events of one extra call")
    out["kernel_source_hash"] = khash
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None, help="merge the lines into this JSON file")
    args = ap.parse_args()
    import bench
    from tests import test_matches_contract as T

    ctx = S.get_context()
    doc = {}
    if args.out and os.path.exists(args.out):
        with open(args.out) as f:
            doc = json.load(f)
    doc["box"] = box()
    doc["contract"] = {k: T.measure(k)[1] for k in sorted(T.CASES)}
    doc["contract"]["what"] = ("tests/numpy_matches.py on tests/numpy_features.py's features (CPU, no device involved) of the two cases of "
                               "tests/test_matches_contract.py: 240 x 320 textures, default settings; the largest distance of the four image "
                               "corners under the refitted H from their true positions")
    print(json.dumps(doc["contract"]), flush=True)
    for name in SIZES:
        doc[f"timing_{name}"] = measure(ctx, name, max(3, args.steps), name == "8x500", bench.kernel_source_hash())
        print(json.dumps(doc[f"timing_{name}"]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
