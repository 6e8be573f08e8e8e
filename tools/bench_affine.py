#!/usr/bin/env python
"""The affine registration (MatchEstimator(model="affine"), CameraSolver(model="affine"); csrc/stx_matches.hip, csrc/stx_cameras.hip) on
planted inputs: 8 images x 500 features and 64 images x 2000 features.
usage: python tools/bench_affine.py [--steps 10] [--out profiles/affine.json] [--contract-only]
contract: tests/numpy_affine.py on the cases of tests/test_affine_contract.py, on the CPU (no device involved): the largest corner error
relative to the centre tile — tests/test_affine_contract.py and the GPU tests assert twice these values, so --contract-only is run again
whenever the contract or a rig changes.
timing_<size>, adjustment: tests/affine_rigs.grid_rig — tiles of 1400 x 800 in a grid of 4 x 2 or 8 x 8 at a pitch of 0.7, each through
its own similarity, 0.5 px of noise, one wrong match per three inliers.  register_ms, a host clock around one register() after one
warm-up call, `steps` calls, median / min / max; device_ms_per_evaluation: the launch's own HIP events, summed over the call and divided
by its evaluations (median over the calls), with_copy alike; numpy: the same call with the contract's vectorised evaluation in the
device's place, 3 calls — its clock holds numpy_affine.match_terms and numpy_cameras.ordered_sum over points gathered once, the variants
made outside it, which is what the device's "with copies" holds.
timing_<size>, ransac: tools/bench_matches.scene (neighbours share half their features through a translation, 15 % of them misplaced),
500 hypotheses; per model the context profiler's events of match_ransac and match_pick in one call after one warm-up call, `steps` calls,
median — the other two launches of a call do not depend on the model.
No target is set: this is the first measurement of this code."""
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

SIZES = {"8x500": (4, 2, 500), "64x2000": (8, 8, 2000)}
SIZE = (1400, 800)
MODELS = ("homography", "affine_partial", "affine_full")


def clock(solver, F, M, runs, evaluate=None):
    ms, evals, dev, devc = [], [], [], []
    for _ in range(runs):
        t0 = time.perf_counter()
        solver.register(F, M, evaluate=evaluate)
        ms.append((time.perf_counter() - t0) * 1e3)
        evals.append(solver.info["evaluations"])
        dev.append(solver.info["device_ms"] / solver.info["evaluations"])
        devc.append(solver.info["device_ms_with_copy"] / solver.info["evaluations"])
    return {"register_ms": {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)},
            "evaluations": int(statistics.median(evals))}, statistics.median(dev), statistics.median(devc)


def adjustment(ctx, name, steps):
    from tests import affine_rigs as AR
    from tests import camera_rigs as CR
    from tests import numpy_affine as NA
    from tests import numpy_cameras as NC

    cols, rows, nf = SIZES[name]
    n = cols * rows
    feats, matches, truth = AR.grid_rig(0, cols, rows, per_image=nf, size=SIZE, max_shared=None, outliers=1 / 3)
    F, M = CR.to_package(feats, matches)
    solver = S.CameraSolver(model="affine")
    idx, cams = solver.register(F, M, ctx=ctx)  # warm-up: allocator, code object
    _, centre = NC.spanning_tree(matches, n)
    out = {"images": n, "features_per_image": nf, "kept": len(idx), "edges": solver.info["edges"], "matches": solver.info["matches"],
           "accepted": solver.info["accepted"], "workgroups": solver.info["edges"],
           "corner_error_px": round(AR.corner_error([c.R for c in cams], {"T": [truth["T"][i] for i in idx]}, centre, SIZE), 4)}
    out["device"], dev, devc = clock(solver, F, M, steps)
    out["device"]["device_ms_per_evaluation"], out["device"]["device_ms_with_copy_per_evaluation"] = round(dev, 4), round(devc, 4)
    ed = NC.edges(matches, n)
    pts = [NA.uncentred(f) for f in feats]
    gathered = [NC.edge_points(feats, matches, n, i, j, pts) for i, j in ed]
    per_eval = []

    def numpy_eval(p, V):
        t0 = time.perf_counter()
        sums = np.array([NC.ordered_sum(NA.match_terms(V[i], V[j], xyuv)) for (i, j), xyuv in zip(ed, gathered)]).reshape(-1, 45)
        per_eval.append((time.perf_counter() - t0) * 1e3)
        return sums[:, 0], sums[:, 1:9], sums[:, 9:]

    ref = S.CameraSolver(model="affine")
    out["numpy"], _, _ = clock(ref, F, M, 3, numpy_eval)
    out["numpy"]["numpy_ms_per_evaluation"] = round(statistics.median(per_eval), 3)
    out["numpy"]["equal_parameters"] = bool(np.allclose(ref.info["parameters"], solver.info["parameters"], rtol=1e-9, atol=1e-6))
    out["device_over_numpy"] = {"evaluation_with_copy": round(devc / statistics.median(per_eval), 5),
                                "evaluation_launch_alone": round(dev / statistics.median(per_eval), 5)}
    return out


def ransac(ctx, name, steps):
    from tools.bench_matches import scene

    cols, rows, nf = SIZES[name]
    feats = scene(cols * rows, nf)
    out = {"hypotheses": 500}
    for model in MODELS:
        est = S.MatchEstimator(model=model.split("_")[0], full_affine=model == "affine_full", range_width=1)
        got = est.match(feats, ctx=ctx)  # warm-up
        rows_ms = {"match_ransac": [], "match_pick": []}
        for _ in range(steps):
            ctx.prof_reset()
            ctx.prof_enable(True)
            est.match(feats, ctx=ctx)
            ctx.sync()
            for e in ctx.prof_results():
                if e["kernel"] in rows_ms:
                    rows_ms[e["kernel"]].append(e["total_ms"])
            ctx.prof_enable(False)
        out[model] = {"pairs": est.info["pairs"], "matches": est.info["matches"],
                      "inliers": int(sum(e.num_inliers for e in got if 0 <= e.src_img_idx < e.dst_img_idx)),
                      "match_ransac_ms": round(statistics.median(rows_ms["match_ransac"]), 4),
                      "match_pick_ms": round(statistics.median(rows_ms["match_pick"]), 4)}
    for model in MODELS[1:]:
        out[model]["ransac_over_homography"] = round(out[model]["match_ransac_ms"] / out["homography"]["match_ransac_ms"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None, help="merge the lines into this JSON file")
    ap.add_argument("--contract-only", action="store_true", help="the CPU part alone (no device)")
    args = ap.parse_args()
    from tests import affine_rigs as AR

    doc = {}
    if args.out and os.path.exists(args.out):
        with open(args.out) as f:
            doc = json.load(f)
    doc["contract"] = {k: AR.measure(k)[1] for k in AR.CASES}
    doc["contract"]["what"] = ("tests/numpy_affine.py (CPU, no device involved) on the cases of tests/test_affine_contract.py: grids of 320 x 240 "
                               "tiles at a pitch of 0.7, turns within 2 degrees, scales within 2 %, 0.5 px of noise, and four such tiles of a "
                               "texture through the numpy detector and the affine matcher; corner_error_px: the largest distance between "
                               "where the recovered and the planted transforms, both relative to the centre tile, take a tile's corners")
    print(json.dumps(doc["contract"]), flush=True)
    if not args.contract_only:
        import bench
        from tools.bench_matches import box

        ctx = S.get_context()
        doc["box"] = box()
        if not doc["box"]["device"]:
            doc["box"] = {"device": "not available", "note": "the HIP runtime returned an empty device name; one GPU of a box shared with other jobs"}
        steps = max(3, args.steps)
        for name in SIZES:
            doc[f"timing_{name}"] = {"case": name, "adjustment": adjustment(ctx, name, steps), "ransac": ransac(ctx, name, steps), "runs": steps,
                                     "kernel_source_hash": bench.kernel_source_hash()}
            print(json.dumps(doc[f"timing_{name}"]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
