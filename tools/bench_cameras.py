#!/usr/bin/env python
"""CameraSolver (the project's own camera registration; its ray adjustment is csrc/stx_cameras.hip) on planted rigs: 8 images x 500
features and 64 images x 2000 features, one row of cameras in which only neighbours overlap (by half), as tools/bench_matches.py's
scenes do.
usage: python tools/bench_cameras.py [--steps 10] [--out profiles/cameras.json]
The rigs: tests/camera_rigs.point_rig — unit-vector landmarks seen by cameras of focal 8000 +- 5 % on 1400 x 800 images, yaw steps of
half the field of view (5 degrees), +- 0.5 degrees of pitch and roll, 0.5 px of noise, one wrong match per three inliers.
Per size one JSON line: register_ms, a host clock around one register() — subset, estimate, the upload of the edges, every evaluation
(variants on the host, one launch, one wait, the 4n x 4n solve), wave correction — after one warm-up call, `steps` calls, median / min /
max; device_ms_per_evaluation: the launch's own HIP events, summed over the call and divided by its evaluations (median over the calls),
with_copy alike; numpy: the same call with the contract's numpy evaluation in the device's place, 3 calls — its clock holds
tests/numpy_cameras.match_terms and ordered_sum over points gathered once, the variants made outside it, which is what the device's
"with copies" holds; device_over_numpy: the ratios of the two.  --out merges the lines into the JSON file as "timing_<size>", next to "contract"
(tests/test_cameras_contract.py's cases, measured here again on the CPU).  No target is set: this is the first measurement of this code.

--model reproj (usage: python tools/bench_cameras.py --model reproj --out profiles/reproj.json): CameraSolver(model="reproj") on rigs of the
same geometry with a planted principal-point offset and aspect (tests/reproj_rigs.point_rig): 8 images with about 120 matches on an edge
and 64 images with about 2000.  Per size one JSON line: register_ms and the device's time per evaluation with and without the copies as
above, evaluations per adjustment, and beside them the same figures of the ray model (CameraSolver()) on the same features and matches.
"contract" holds tests/numpy_reproj.py on the rigs and masks of tests/test_reproj_contract.py with the principal points and aspects that
came back (CPU).  No numpy clock is taken for this model."""
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
FOCAL, SIZE = 8000.0, (1400, 800)


def planted(n, nf, seed=0):
    from tests import camera_rigs as CR

    half = float(np.rad2deg(np.arctan(SIZE[0] / 2 / FOCAL)))
    return CR.point_rig(seed, n, per_image=nf, size=SIZE, focal=FOCAL, step=(0.95 * half, 1.05 * half), jitter=0.5, max_shared=None, outliers=1 / 3)


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


def measure(ctx, name, steps, khash):
    from tests import camera_rigs as CR
    from tests import numpy_cameras as NC

    n, nf = SIZES[name]
    feats, matches, truth = planted(n, nf)
    F, M = CR.to_package(feats, matches)
    solver = S.CameraSolver()
    idx, cams = solver.register(F, M, ctx=ctx)  # warm-up: allocator, code object
    _, centre = NC.spanning_tree(matches, n)
    rot, foc = CR.errors([(c.focal, c.R) for c in cams], truth, centre)
    out = {"case": name, "images": n, "features_per_image": nf, "kept": len(idx), "edges": solver.info["edges"], "matches": solver.info["matches"],
           "accepted": solver.info["accepted"], "rotation_error_deg": round(rot, 4), "focal_error_percent": round(foc, 4),
           "workgroups": solver.info["edges"]}
    out["device"], dev, devc = clock(solver, F, M, steps)
    out["device"]["device_ms_per_evaluation"], out["device"]["device_ms_with_copy_per_evaluation"] = round(dev, 4), round(devc, 4)
    # the numpy side, like for like with the device's "with copies": the variants are made outside the clock (the package makes them
    # for the device too) and the edges' points are gathered once, as the upload of the edges is; the clock holds the contract's terms
    # of every match and their ordered sums
    ed = NC.edges(matches, n)
    gathered = [NC.edge_points(feats, matches, n, i, j) for i, j in ed]
    per_eval = []

    def numpy_eval(p, V):
        t0 = time.perf_counter()
        sums = np.array([NC.ordered_sum(NC.match_terms(V[i], V[j], xyuv)) for (i, j), xyuv in zip(ed, gathered)]).reshape(-1, 45)
        per_eval.append((time.perf_counter() - t0) * 1e3)
        return sums[:, 0], sums[:, 1:9], sums[:, 9:]

    ref = S.CameraSolver()
    out["numpy"], _, _ = clock(ref, F, M, 3, numpy_eval)
    out["numpy"]["numpy_ms_per_evaluation"] = round(statistics.median(per_eval), 3)
    out["numpy"]["equal_parameters"] = bool(CR.parameters_agree(ref.info["parameters"], solver.info["parameters"], centre))
    out["device_over_numpy"] = {
        "register": round(out["device"]["register_ms"]["median"] / out["numpy"]["register_ms"]["median"], 4),
        "evaluation_with_copy": round(devc / statistics.median(per_eval), 5), "evaluation_launch_alone": round(dev / statistics.median(per_eval), 5)}
    out["runs"], out["kernel_source_hash"] = steps, khash
    out["how"] = ("register_ms: host clock around one register() of host-resident features and matches, after one warm-up call; "
                  "device_ms_per_evaluation: HIP events around the launch, with_copy: around the upload of the variants, the launch and the "
                  "copy back; numpy: the contract's match_terms + ordered_sum on points gathered once and variants made outside the clock, inside the same call")
    return out


REPROJ_SIZES = {"8x120": (8, 240), "64x2000": (64, 4000)}  # images, features per image: neighbours share about half


def measure_reproj(ctx, name, steps, khash):
    from tests import camera_rigs as CR
    from tests import numpy_cameras as NC
    from tests import reproj_rigs as RR

    n, nf = REPROJ_SIZES[name]
    half = float(np.rad2deg(np.arctan(SIZE[0] / 2 / FOCAL)))
    feats, matches, truth = RR.point_rig(0, n, per_image=nf, size=SIZE, focal=FOCAL, step=(0.95 * half, 1.05 * half), jitter=0.5, max_shared=None,
                                         outliers=1 / 3)
    F, M = CR.to_package(feats, matches)
    _, centre = NC.spanning_tree(matches, n)
    per_edge = sorted(int(matches[i * n + j]["num_inliers"]) for i, j in NC.edges(matches, n))
    out = {"case": name, "images": n, "features_per_image": nf, "planted_offset_px": list(truth["offset"]), "planted_aspect": truth["aspect"],
           "matches_per_edge": {"median": per_edge[len(per_edge) // 2], "min": per_edge[0], "max": per_edge[-1]}}
    for model in ("reproj", "rotation"):
        solver = S.CameraSolver(model=model)
        idx, cams = solver.register(F, M, ctx=ctx)  # warm-up: allocator, code object
        rot, foc = CR.errors([(c.focal, c.R) for c in cams], truth, centre)
        edges, total = solver.info["edges"], solver.info["matches"]
        rec = {"kept": len(idx), "edges": edges, "matches": total,
               "accepted": solver.info["accepted"], "rms_px_or_rays": round(float(np.sqrt(solver.info["last_E"] / max(total, 1))), 4),
               "rotation_error_deg": round(rot, 4), "focal_error_percent": round(foc, 4), "workgroups": edges * (3 if model == "reproj" else 1)}
        timing, dev, devc = clock(solver, F, M, steps)
        rec.update(timing)
        rec["device_ms_per_evaluation"], rec["device_ms_with_copy_per_evaluation"] = round(dev, 4), round(devc, 4)
        if model == "reproj":
            rec["offset_px_mean"] = [round(float(np.mean([c.ppx - SIZE[0] / 2 for c in cams])), 3), round(float(np.mean([c.ppy - SIZE[1] / 2 for c in cams])), 3)]
            rec["aspect_mean"] = round(float(np.mean([c.aspect for c in cams])), 5)
        out["ray_model_beside" if model == "rotation" else "reproj"] = rec
    out["reproj_over_ray_launch"] = round(out["reproj"]["device_ms_per_evaluation"] / out["ray_model_beside"]["device_ms_per_evaluation"], 3)
    out["runs"], out["kernel_source_hash"] = steps, khash
    out["how"] = ("register_ms: host clock around one register() of host-resident features and matches, after one warm-up call; "
                  "device_ms_per_evaluation: HIP events around the launch, with_copy: around the upload of the variants, the launch and the copy "
                  "back, both summed over a call and divided by its evaluations, median over the calls; the ray model on the same inputs")
    return out


def main_reproj(args):
    from tests import reproj_rigs as RR

    doc = {}
    if args.out and os.path.exists(args.out):
        with open(args.out) as f:
            doc = json.load(f)
    doc["contract"] = {name: {mask: RR.measure(name, mask)[1] for mask in RR.MASKS} for name in sorted(RR.RIGS)}
    doc["contract"]["what"] = ("tests/numpy_reproj.py (CPU, no device involved) on the rigs of tests/test_reproj_contract.py: 800 x 600 images at focal "
                               "700 +- 5 % with a planted offset of (12, -9) px and an aspect of 1.02, from 1.03 x the focal, no offset, aspect 1 and "
                               "rotations off by up to 1 degree; per mask the rms reprojection error and the principal points and aspects that came back")
    print(json.dumps(doc["contract"]), flush=True)
    if not args.contract_only:
        import bench
        from tools.bench_matches import box

        ctx = S.get_context()
        doc["box"] = box()
        if not doc["box"]["device"]:
            doc["box"] = {"device": "not available", "note": "the HIP runtime returned an empty device name; one GPU of a box shared with other jobs"}
        for name in REPROJ_SIZES:
            doc[f"timing_{name}"] = measure_reproj(ctx, name, max(3, args.steps), bench.kernel_source_hash())
            print(json.dumps(doc[f"timing_{name}"]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None, help="merge the lines into this JSON file")
    ap.add_argument("--contract-only", action="store_true", help="the CPU part alone (no device)")
    ap.add_argument("--model", default="rotation", choices=("rotation", "reproj"), help="reproj: the reprojection model's rigs and figures")
    args = ap.parse_args()
    if args.model == "reproj":
        return main_reproj(args)
    from tests import camera_rigs as T

    doc = {}
    if args.out and os.path.exists(args.out):
        with open(args.out) as f:
            doc = json.load(f)
    doc["contract"] = {k: T.measure(k)[1] for k in T.CASES}
    doc["contract"]["what"] = ("tests/numpy_cameras.py (CPU, no device involved) on the cases of tests/test_cameras_contract.py: point rigs of "
                               "800 x 600 images at focal 700 +- 5 % and four 320 x 240 views of a texture through the numpy detector and "
                               "matcher; the largest rotation error relative to the centre camera and the largest focal error")
    print(json.dumps(doc["contract"]), flush=True)
    if not args.contract_only:
        import bench
        from tools.bench_matches import box

        ctx = S.get_context()
        doc["box"] = box()
        if not doc["box"]["device"]:
            doc["box"] = {"device": "not available", "note": "the HIP runtime returned an empty device name; one GPU of a box shared with other jobs"}
        for name in SIZES:
            doc[f"timing_{name}"] = measure(ctx, name, max(3, args.steps), bench.kernel_source_hash())
            print(json.dumps(doc[f"timing_{name}"]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
