#!/usr/bin/env python
"""bench.py — warp + multi-band blend throughput on MI355X (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W          (N > 1 without RANK in the environment: spawns its N ranks)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A "step" is one pass of the hot path over one batch of synthetic input: every source frame (already resident in HBM) is
warped (fused image + mask), fed to the blender and the panorama is produced in HBM.

  N = 1   BASELINE.json configs[1]: 8 synthetic 4000x3000 frames, spherical warp + 5-band blend.
  N > 1   BASELINE.json configs[2] ("config 3"): 4000x3000 frames as yaw columns x 4 pitch rows (f = 0.75 W), one column
          of 4 frames per GPU — N = 8 is the 32-frame configuration itself, N = 2 / 4 are 2 / 4 of its 8 columns (same
          yaw step, same geometry per GPU: weak scaling).  --config 4: 8000x6000, cylindrical, 7 bands, two columns =
          8 frames per GPU (N = 8: configs[3], 64 frames).  --config 2 --gpus N: the tele-ring family of round 1.
  --config 3 / 4 at N = 1: one GPU's share of that configuration, unsharded (the same-family single-GPU rate).

Prints ONE JSON line on rank 0.  A plain run sets up, warms up, times exactly --steps steps and prints the headline (`value`,
`ms_per_step` = milliseconds of one timed step).  --full adds everything else, each measured after the timed steps: `timed_rounds`
(more rounds of --steps steps until --min-seconds are timed: the spread), `roofline` (dominant kernel, HIP events on the stream the
kernel runs on), `kernels[]`, `parity` (N = 1: the panorama of the timed path against the oracle's; N > 1: every rank's band against
the oracle's columns of that band — rank 0 runs the oracle once on all frames; --no-parity skips it), `cpu_baseline` (the oracle, timed
on the host cores, N = 1 only), the latency of one panorama, the PCIe-inclusive rates and the extra legs.
--dump-outputs DIR writes what the last timed step computed (see dump_outputs).  torch is imported only for N > 1 (rendezvous /
barrier); the product path is ctypes -> libstitching_amd.so.
"""
import argparse
import glob
import hashlib
import json
import os
import socket
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8 TB/s spec
MIN_TIMED_S = 3.0      # --full: `timed_rounds` repeats rounds of --steps steps until they hold at least this much work
DUMP_BYTES = 64 * 10**6  # --dump-outputs: all files of one run together stay below this


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--full", action="store_true", help="after the timed steps, also measure and check everything besides the headline: "
                   "timed_rounds, roofline / kernels, parity, cpu_baseline, latency, PCIe-inclusive rates, extra legs (N > 1: the "
                   "same-family single-GPU rate and the per-rank parity)")
    p.add_argument("--dump-outputs", default="", metavar="DIR", help="write the panorama and mask of the last timed step as float32 / "
                   "float64 .npy files under DIR (a seeded sample of the pixels where the whole would exceed 64 MB)")
    p.add_argument("--config", type=int, default=0, help="BASELINE configuration 2..5 (1-based as in DESIGN.md); default: 2 at "
                   "N = 1, 3 at N > 1")
    p.add_argument("--frames-per-gpu", type=int, default=0, help="config 2 only (default 8)")
    p.add_argument("--width", type=int, default=0)
    p.add_argument("--height", type=int, default=0)
    p.add_argument("--bands", type=int, default=0)
    p.add_argument("--warper", default="")
    p.add_argument("--blender", default="")
    p.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip cpu_baseline (and with it the N = 1 parity)")
    p.add_argument("--no-parity", action="store_true", help="--full, N > 1: skip the comparison of every rank's band with the oracle's "
                   "panorama (rank 0 runs the oracle once on all frames, outside the timed region)")
    p.add_argument("--no-extra", action="store_true", help="--full: skip the extra legs (seam masks, configs 4 / 5, modes)")
    p.add_argument("--cpu-frames", type=int, default=0, help="frames in the CPU-baseline sample (0: all frames of the step, which also gives `parity`)")
    p.add_argument("--profile-steps", type=int, default=10, help="--full: steps of the per-kernel HIP-event pass")
    p.add_argument("--min-seconds", type=float, default=MIN_TIMED_S, help="--full: seconds of work the `timed_rounds` record holds at least")
    p.add_argument("--streams", type=int, default=2, help="panoramas in flight per GPU (contexts = HIP streams); N = 1 "
                   "measured: 1 -> 93.0, 2 -> 105.9, 3 -> 99.6 Gpix/s")
    p.add_argument("--e2e-steps", type=int, default=2, help="--full: PCIe-inclusive passes (host frames in, host panorama out)")
    p.add_argument("--traffic-json", default=os.path.join(ROOT, "profiles", "r06_traffic.json"),
                   help="JSON with PMC-derived HBM bytes per launch and rocprofv3's average launch durations (tools/make_traffic_json.py)")
    args = p.parse_args()
    if args.steps < 1 or args.warmup < 0:
        p.error("--steps must be >= 1 and --warmup >= 0")
    return args


def kernel_source_hash():
    """sha256 over the device CODE (.hip files, the device headers, the Makefile's flags; comments and white space dropped, so that rewording a
    comment does not orphan a traffic profile): a profile is only quoted for the kernels it was measured on (host-side API changes
    do not move bytes)."""
    h = hashlib.sha256()
    for f in sorted(glob.glob(os.path.join(ROOT, "stitching_amd", "csrc", "*"))):
        # device code and the Makefile (per-file code-generation flags; its comments start with "#")
        if f.endswith(".hip") or os.path.basename(f) in ("stx_device_math.h", "stx_blend_kernels.h", "Makefile"):
            mk = f.endswith("Makefile")
            for line in open(f, encoding="utf-8", errors="replace"):
                if mk and not line.startswith(("FLAGS", "EXTRA", "WARP_EXTRA", "BLEND_EXTRA", "FAST_EXTRA")):
                    continue  # of the Makefile only the flag assignments
                code = "".join(line.split("#" if mk else "//", 1)[0].split())  # no "//" inside a string literal in these sources
                if code:
                    h.update(code.encode() + b"\n")
    return h.hexdigest()[:16]


def workload(args, world):
    """Cameras and shapes of the configuration (all ranks build the same description)."""
    from stitching_amd import synthetic

    cfg = args.config or (2 if world == 1 else 3)
    w = dict(cfg=cfg)
    if cfg == 2:
        w.update(width=4000, height=3000, warper="spherical", blender="multiband", bands=5, fpg=args.frames_per_gpu or 8)
    elif cfg == 3:
        w.update(width=4000, height=3000, warper="spherical", blender="multiband", bands=5, fpg=4)
    elif cfg == 4:
        w.update(width=8000, height=6000, warper="cylindrical", blender="multiband", bands=7, fpg=8)
    elif cfg == 5:
        w.update(width=4000, height=3000, warper="affine", blender="feather", bands=0, fpg=16)
    else:
        raise SystemExit(f"bench.py: unknown --config {cfg}")
    for k, v in (("width", args.width), ("height", args.height), ("bands", args.bands), ("warper", args.warper), ("blender", args.blender)):
        if v:
            w[k] = v
    W, H, fpg = w["width"], w["height"], w["fpg"]
    n_total = fpg * world
    if w["warper"] == "affine":
        if world > 1:
            raise SystemExit("bench.py: config 5 (AffineStitcher tiles) is a single-GPU configuration")
        cams = synthetic.affine_scan_cameras(n_total, W, H)
        name = f"BASELINE config 5: {n_total} scan tiles {W}x{H}, affine warp + {w['blender']} blender"
    elif cfg == 2:
        cams = synthetic.ring_cameras(n_total, W, H, focal_factor=0.75 * world)
        name = (f"BASELINE config 2: {n_total} synthetic {W}x{H} frames, one ring" if world == 1 else
                f"config-2 family: {n_total} synthetic {W}x{H} frames, one tele ring (focal 0.75 W x {world}), {fpg} per GPU")
    elif cfg == 3:
        cams = synthetic.grid_cameras(world, 4, W, H, layout_yaw=8)
        name = (f"BASELINE config 3{'' if world == 8 else ' family'}: {n_total} synthetic {W}x{H} frames = {world} of 8 yaw columns x 4 pitch "
                f"rows (f = 0.75 W, rows at +-18.6 / +-55.8 deg), one column per GPU")
    else:
        cams = synthetic.grid_cameras(2 * world, 4, W, H, max_edge_lat_deg=50.0, layout_yaw=16)
        name = (f"BASELINE config 4{'' if world == 8 else ' family'}: {n_total} synthetic {W}x{H} frames = {2 * world} of 16 yaw columns x 4 "
                f"pitch rows (f = 0.75 W), two columns per GPU")
    if w["warper"] != "affine" and len(cams) > 1:
        # the geometry in numbers (it is NOT SURVEY 8(d)'s 0.70 hfov = 47 degree step: a ring of 8 such frames, and all the more the
        # +-56 degree rows of config 3, would cross the +-180 degree seam of the parametrisation — DESIGN.md section 6)
        import math

        import numpy as np

        yaw = lambda c: math.degrees(math.atan2(float(np.asarray(c.R)[0, 2]), float(np.asarray(c.R)[2, 2])))  # noqa: E731
        rows = 1 if cfg == 2 else 4
        step = abs(yaw(cams[rows]) - yaw(cams[0])) if len(cams) > rows else 0.0
        hfov = 2.0 * math.degrees(math.atan(W / (2.0 * float(cams[0].focal))))
        if step > 0:
            name += f"; yaw step {step:.1f} deg = {step / hfov:.2f} hfov ({100 * (1 - step / hfov):.0f} % overlap; SURVEY 8(d) names 0.70 hfov)"
    w.update(cams=cams, n_total=n_total, name=name)
    return w


def survey_8d_bytes(src_sizes, corners, wsizes, bands):
    """Algorithmic HBM bytes of ONE pass by SURVEY.md §8(d)'s model (OpenCV's dataflow with the maps
    never stored): warp 3 P_s + 4 P_w; feed 4 P_w + (12 h + 8 h + 20 g) P_f; finish (10 + 6 + 12) g P_d
    + 4 P_d, with g = sum_{i<=B} 4^-i, h = g - 1, P_f the 2^B-aligned feed rectangles
    (MultiBandBlender::feed geometry) and P_d the padded panorama.  DESIGN.md §5."""
    g = sum(4.0 ** -i for i in range(bands + 1))
    h = g - 1.0
    x0 = min(c[0] for c in corners)
    y0 = min(c[1] for c in corners)
    x1 = max(c[0] + s[0] for c, s in zip(corners, wsizes))
    y1 = max(c[1] + s[1] for c, s in zip(corners, wsizes))
    al = 1 << bands
    pw, ph = -(-(x1 - x0) // al) * al, -(-(y1 - y0) // al) * al
    gap = 3 * al
    p_s = sum(w * hh for w, hh in src_sizes)
    p_w = sum(w * hh for w, hh in wsizes)
    p_f = 0
    for (cx, cy), (w, hh) in zip(corners, wsizes):
        tx, ty = max(x0, cx - gap), max(y0, cy - gap)
        bx, by = min(x0 + pw, cx + w + gap), min(y0 + ph, cy + hh + gap)
        tx, ty = x0 + (tx - x0) // al * al, y0 + (ty - y0) // al * al
        p_f += (-(-(bx - tx) // al) * al) * (-(-(by - ty) // al) * al)
    p_d = pw * ph
    warp = 3.0 * p_s + 4.0 * p_w
    feed = 4.0 * p_w + (12.0 * h + 8.0 * h + 20.0 * g) * p_f
    finish = (10.0 + 6.0 + 12.0) * g * p_d + 4.0 * p_d
    return {"warp": warp, "feed": feed, "finish": finish, "total": warp + feed + finish, "P_s": p_s, "P_w": p_w,
            "P_f": p_f, "P_d": p_d}


def cpu_baseline(wl, frames, cams, all_cams, n_frames):
    """The oracle (CPU restatement of OpenCV's algorithm — NOT OpenCV; see oracle/stx_oracle.cpp)
    on the same workload, all host cores (OpenMP).  Returns (record, panorama, mask)."""
    import numpy as np

    from oracle import oracle as O
    from stitching_amd.synthetic import blend_strength_for_bands

    O.build()
    # OpenMP thread count: all hardware threads is not the fastest choice on a 256-thread host (memory-bound
    # pyramids, SMT); calibrate on a two-frame warp + blend (both phases scale differently) and keep the best
    w0 = O.Warper(wl["warper"])
    w0.set_scale(all_cams)
    best = (None, 1)
    cand = sorted({c for c in (8, 16, 32, 64, 128, O.max_threads()) if c <= O.max_threads()})
    cal_sizes = [(f.shape[1], f.shape[0]) for f in frames[:2]]
    for c in cand:
        O.set_num_threads(c)
        t = time.perf_counter()
        cc, cs = w0.warp_rois(cal_sizes, cams[:2])
        cb = O.Blender(wl["blender"], 5)
        cb.prepare(cc, cs)
        for f, cam, sz, corner in zip(frames[:2], cams[:2], cal_sizes, cc):
            cb.feed(w0.warp_image(f, cam), w0.create_and_warp_mask(sz, cam), corner)
        cb.blend()
        dt = time.perf_counter() - t
        if best[0] is None or dt < best[0]:
            best = (dt, c)
    cores = best[1]
    O.set_num_threads(cores)
    n = min(n_frames, len(frames))
    frames, cams = frames[:n], cams[:n]
    sizes = [(f.shape[1], f.shape[0]) for f in frames]
    w = O.Warper(wl["warper"])
    w.set_scale(all_cams)
    t0 = time.perf_counter()
    corners, wsizes = w.warp_rois(sizes, cams)
    roi = O.result_roi(corners, wsizes)
    strength = blend_strength_for_bands(wl["bands"], roi[2], roi[3]) if wl["blender"] == "multiband" else 5
    b = O.Blender(wl["blender"], strength)
    b.prepare(corners, wsizes)
    for f, c, corner in zip(frames, cams, corners):
        b.feed(w.warp_image(f, c), w.create_and_warp_mask((f.shape[1], f.shape[0]), c), corner)
    pano, pmask = b.blend()
    dt = time.perf_counter() - t0
    mpix = sum(f.shape[0] * f.shape[1] for f in frames) / 1e6
    bands_txt = f"{b.blender.num_bands()}-band " if wl["blender"] == "multiband" else ""
    res = {"value": round(mpix / dt, 3), "unit": "Mpix/s", "cores": cores, "kind": "port",
           "sample": f"{n} frames {wl['width']}x{wl['height']}, {wl['warper']} warp + {bands_txt}{wl['blender']} "
                     f"blend, {dt:.2f} s wall on {cores} of {O.max_threads()} OpenMP threads (fastest of {cand} on a two-frame warp + blend); "
                     f"CPU restatement of OpenCV's algorithm (oracle/), not OpenCV"}
    # the reference's own dataflow on ONE frame (stitching/warper.py:44,59: two PyRotationWarper.warp calls, each
    # building both fp32 maps in OpenCV's serial buildMaps loop, then cv::remap), for scale against the fused port above
    t1 = time.perf_counter()
    roi = w.warp_roi(sizes[0], cams[0])
    K0 = O.Warper.get_K(cams[0])
    O.set_num_threads(1)
    xm, ym = O.build_maps(wl["warper"], w.scale, K0, cams[0].R, roi)
    xm2, ym2 = O.build_maps(wl["warper"], w.scale, K0, cams[0].R, roi)
    O.set_num_threads(cores)
    O.remap_linear(frames[0], xm, ym)
    O.remap_nearest(np.full(frames[0].shape[:2], 255, np.uint8), xm2, ym2)
    dt_ref = time.perf_counter() - t1
    res["reference_dataflow_warp"] = {"value": round(frames[0].shape[0] * frames[0].shape[1] / 1e6 / dt_ref, 3), "unit": "Mpix/s",
                                      "sample": f"1 frame, maps materialised twice by a serial buildMaps + remap x2: {dt_ref:.2f} s"}
    return res, np.asarray(pano), np.asarray(pmask)


def oracle_panorama(wl, frames, all_cams):
    """The oracle's panorama of ALL frames of the configuration (the checker of the N > 1 `parity` record; never timed)."""
    import numpy as np

    from oracle import oracle as O
    from stitching_amd.synthetic import blend_strength_for_bands

    O.build()
    O.set_num_threads(max(1, min(O.max_threads(), 64)))
    w = O.Warper(wl["warper"])
    w.set_scale(all_cams)
    sizes = [(f.shape[1], f.shape[0]) for f in frames]
    corners, wsizes = w.warp_rois(sizes, all_cams)
    roi = O.result_roi(corners, wsizes)
    strength = blend_strength_for_bands(wl["bands"], roi[2], roi[3]) if wl["blender"] == "multiband" else 5
    b = O.Blender(wl["blender"], strength)
    b.prepare(corners, wsizes)
    for f, c, corner in zip(frames, all_cams, corners):
        b.feed(w.warp_image(f, c), w.create_and_warp_mask((f.shape[1], f.shape[0]), c), corner)
    pano, pmask = b.blend()
    return np.asarray(pano), np.asarray(pmask), corners, wsizes


def oracle_chain(wl, frames, cams, all_cams, trig=None, model=None, gain_maps=None, low_seams=None, blend_strength=None):
    """The checker's panorama for an extra leg (never timed): the oracle's warp -> [block gain] -> [seam-mask resize] -> blend chain on
    host frames under the arithmetic model the leg runs the product in.  -> (panorama, mask, bands)"""
    import numpy as np

    from oracle import oracle as O
    from stitching_amd.synthetic import blend_strength_for_bands

    O.build()
    O.set_num_threads(max(1, min(O.max_threads(), 64)))
    prev = O.set_model(**model) if model else None
    try:
        w = O.Warper(wl["warper"], **({"trig": trig} if trig is not None else {}))
        w.set_scale(all_cams)
        sizes = [(f.shape[1], f.shape[0]) for f in frames]
        corners, wsizes = w.warp_rois(sizes, cams)
        roi = O.result_roi(corners, wsizes)
        strength = blend_strength if blend_strength is not None else blend_strength_for_bands(wl["bands"], roi[2], roi[3])
        b = O.Blender("multiband", strength)
        b.prepare(corners, wsizes)
        for k, (f, c, corner) in enumerate(zip(frames, cams, corners)):
            img = w.warp_image(f, c)
            mask = w.create_and_warp_mask((f.shape[1], f.shape[0]), c)
            if gain_maps is not None:
                img = O.block_gain_apply(img, gain_maps[k])
            if low_seams is not None:
                mask = O.seam_resize(low_seams[k], mask)
            b.feed(img, mask, corner)
        pano, pmask = b.blend()
        return np.asarray(pano), np.asarray(pmask), b.blender.num_bands()
    finally:
        if prev:
            O.set_model(**prev)


def parity_record(job, o_pano, o_mask, vs):
    import numpy as np

    g_pano, g_mask = (np.asarray(a) for a in job.run())
    if g_pano.shape != o_pano.shape:
        return {"vs": vs, "shape_mismatch": [list(g_pano.shape), list(o_pano.shape)]}
    d = np.abs(g_pano.astype(np.int16) - o_pano.astype(np.int16))
    return {"vs": vs, "max_abs_diff": int(d.max()), "differing_bytes": int(np.count_nonzero(d)),
            "mask_equal": bool(np.array_equal(g_mask, o_mask)), "panorama_shape": list(g_pano.shape)}


def sharded_parity(job, dist, rank, world, wl, all_cams):
    """N > 1: every rank produces one more band with the job object that was timed; rank 0 runs the oracle on all frames of
    the configuration and compares each rank's band with the oracle's columns of that band, byte for byte."""
    import numpy as np

    from stitching_amd import synthetic

    band, bmask = (np.asarray(a) for a in job.run())
    parts = dist.gather((band, bmask), 0)
    if rank != 0:
        return None
    t0 = time.perf_counter()
    frames = [synthetic.make_frame(i, wl["width"], wl["height"]) for i in range(wl["n_total"])]
    o_pano, o_mask, o_corners, o_sizes = oracle_panorama(wl, frames, all_cams)
    p = job.plan_
    rec = {"vs": "oracle (oracle/stx_oracle.cpp, default model) on all %d frames, compared per rank with the columns of its band" % wl["n_total"],
           "ranks": world, "oracle_seconds": round(time.perf_counter() - t0, 1)}
    if [tuple(c) for c in o_corners] != p.corners or [tuple(s) for s in o_sizes] != p.sizes:
        rec["roi_mismatch"] = True
        return rec
    diffs, nbytes, masks_ok = [], 0, True
    for g, (bp, bm) in enumerate(parts):
        x0, x1 = p.band(g)
        op, om = o_pano[:, x0:x1], o_mask[:, x0:x1]
        if bp.shape != op.shape or bm.shape != om.shape:
            rec["shape_mismatch"] = [g, list(bp.shape), list(op.shape)]
            return rec
        d = np.abs(bp.astype(np.int16) - op.astype(np.int16))
        diffs.append(int(d.max()) if d.size else 0)
        nbytes += int(np.count_nonzero(d))
        masks_ok = masks_ok and bool(np.array_equal(bm, om))
    rec.update(max_abs_diff=max(diffs), differing_bytes=nbytes, mask_equal=masks_ok, per_rank_max_abs_diff=diffs,
               panorama_shape=list(o_pano.shape), band_edges=list(p.edges))
    return rec


def timed_steps(run_step, barrier, steps, warmup, n_inflight, reduce_max):
    """W warm-up steps per panorama in flight, then exactly `steps` timed steps between barriers + stream syncs (max over ranks).
    Returns (seconds, what the last timed step returned); the earlier steps' outputs are dropped as they come back."""
    for i in range(warmup * n_inflight):
        run_step(i)
    barrier()
    t0 = time.perf_counter()
    for i in range(steps - 1):
        run_step(i)
    last = run_step(steps - 1)
    barrier()
    return reduce_max(time.perf_counter() - t0), last


def dump_outputs(out_dir, outputs, rank, world):
    """--dump-outputs: what the last timed step handed its caller — the panorama (u8 x3) and its mask (u8); at N > 1 this rank's
    band, files suffixed _rank<r> — as .npy files: `panorama` / `mask` in float32, whole where they fit this rank's share of
    DUMP_BYTES, else the same seeded sample of pixel positions of both (flattened; the sample depends on the shape alone), and always
    `panorama_row_sums` / `panorama_col_sums` / `mask_row_sums` / `mask_col_sums` over every pixel in float64."""
    import numpy as np

    pano, mask = (np.asarray(a) for a in outputs)
    h, w = mask.shape
    c = pano.shape[2]
    sfx = f"_rank{rank}" if world > 1 else ""
    sums = {"panorama_row_sums": pano.sum(axis=1, dtype=np.float64), "panorama_col_sums": pano.sum(axis=0, dtype=np.float64),
            "mask_row_sums": mask.sum(axis=1, dtype=np.float64), "mask_col_sums": mask.sum(axis=0, dtype=np.float64)}
    room = DUMP_BYTES // world - sum(a.nbytes for a in sums.values()) - 6 * 4096  # .npy headers
    n_px = max(0, room // (4 * (c + 1)))
    if n_px >= h * w:
        arrays = {"panorama": pano.astype(np.float32), "mask": mask.astype(np.float32)}
    else:
        idx = np.unique(np.random.default_rng(20251016).integers(0, h * w, n_px))
        arrays = {"panorama": pano.reshape(-1, c)[idx].astype(np.float32), "mask": mask.reshape(-1)[idx].astype(np.float32)}
    arrays.update(sums)
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, f"{name}{sfx}.npy"), a)


def timed_rounds(run_step, barrier, steps, warmup, n_inflight, min_seconds, reduce_max):
    """W warm-up steps, then rounds of exactly K timed steps (barrier + stream sync on both sides, max over ranks) until
    the rounds hold >= min_seconds of work.  Returns (seconds per round list)."""
    for i in range(warmup * n_inflight):
        run_step(i)
    rounds = []
    total = 0.0
    while True:
        barrier()
        t0 = time.perf_counter()
        for i in range(steps):
            run_step(i)
        barrier()
        dt = reduce_max(time.perf_counter() - t0)
        rounds.append(dt)
        total += dt
        if total >= min_seconds or len(rounds) >= 2000:
            return rounds


def spawn_ranks(args):
    """`python bench.py --gpus N` without a launcher: become `torch.distributed.run` with N ranks on this node."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    os.execv(sys.executable, cmd)


def main():
    args = parse()
    if "RANK" not in os.environ and args.gpus > 1:
        spawn_ranks(args)
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}", file=sys.stderr)
        sys.exit(2)
    dist = None
    if world > 1:
        # Control plane = the product's own TCP rendezvous (stitching_amd/rendezvous.py).  Its port: STITCHING_AMD_RDZV_PORT when the
        # launcher exports one; under torch.distributed.run (the driver's launcher — MASTER_PORT belongs to its store) rank 0 picks a
        # free port and the launcher's gloo group carries that one integer, then torch is out of the picture.
        from stitching_amd.rendezvous import TcpGroup, bound_listener

        port, listener = os.environ.get("STITCHING_AMD_RDZV_PORT"), None
        if port is None:
            import torch.distributed as tdist

            if os.environ.get("MASTER_ADDR", "127.0.0.1") in ("127.0.0.1", "localhost"):
                os.environ.setdefault("GLOO_SOCKET_IFNAME", "lo")  # one node: do not make gloo resolve the container's host name
            # gloo prints "[Gloo] Rank 0 is connected to ..." on STDOUT: this process's stdout carries ONE JSON line and nothing else, so
            # file descriptor 1 points at stderr while the launcher's group is up
            sys.stdout.flush()
            saved_fd = os.dup(1)
            os.dup2(2, 1)
            try:
                tdist.init_process_group(backend="gloo", rank=rank, world_size=world)
                if rank == 0:  # rank 0 binds its listening socket NOW and keeps it: nobody can take the port in between
                    listener, lport = bound_listener(os.environ.get("MASTER_ADDR", "127.0.0.1"))
                box = [lport if rank == 0 else None]
                tdist.broadcast_object_list(box, src=0)
                tdist.barrier()
                tdist.destroy_process_group()
            finally:
                sys.stdout.flush()
                os.dup2(saved_fd, 1)
                os.close(saved_fd)
            port = box[0]
        dist = TcpGroup(rank, world, os.environ.get("MASTER_ADDR", "127.0.0.1"), int(port), listener=listener)

    import numpy as np

    import stitching_amd as S
    from stitching_amd import synthetic
    from stitching_amd.pipeline import StitchJob

    # One process per GPU.  A box with fewer GPUs than ranks (the 1-GPU harness; STITCHING_AMD_FORCE_DEVICE pins it
    # explicitly) puts several ranks on one device: the sharded path then runs with the host-staged transport
    # (RCCL refuses two ranks on one device) and the line says so.
    ndev = S.device_count()
    if "STITCHING_AMD_FORCE_DEVICE" in os.environ:
        dev = int(os.environ["STITCHING_AMD_FORCE_DEVICE"])
        shared = world > 1
    else:
        dev = local_rank % max(1, ndev)
        shared = world > ndev
    if shared and world > 1:
        os.environ.setdefault("STITCHING_AMD_TRANSPORT", "host")
    S.set_default_device(dev)
    ctx = S.get_context()

    wl = workload(args, world)
    W, H, fpg, n_total, all_cams = wl["width"], wl["height"], wl["fpg"], wl["n_total"], wl["cams"]
    my = range(rank * fpg, (rank + 1) * fpg)
    frames = [synthetic.make_frame(i, W, H) for i in my]
    cams = [all_cams[i] for i in my]
    nb = wl["bands"] if wl["blender"] == "multiband" else None

    def make_job(c, frames_):
        if world > 1:
            from stitching_amd.distributed import ShardedStitchJob

            # split: the pyramids of the rank's own images are built while its strips travel (measured on one rank of the
            # 8-rank config-3 job, tools/sim_rank.py: 1.03 ms per step against 1.34 ms with everything built after the exchange)
            return ShardedStitchJob(frames_, cams, all_cams, rank, world, warper_type=wl["warper"], blender_type=wl["blender"],
                                    num_bands=nb, ctx=c, group=dist, split_boundary=True,
                                    transport=(jobs[0].transport if jobs else None))
        j = StitchJob(frames_, cams, warper_type=wl["warper"], blender_type=wl["blender"], num_bands=nb, ctx=c)
        j.warper.set_scale(all_cams)
        return j

    # --streams S: S contexts = S HIP streams; consecutive panoramas (independent steps) alternate between them, so the
    # small coarse-level kernels of one panorama overlap with the large kernels of the next.  At N > 1 the panoramas in
    # flight of a rank share ONE transport (one communicator, exchanges in issue order)
    jobs, ctxs = [], []
    for s_i in range(max(1, args.streams)):
        c = ctx if s_i == 0 else S.Context(ctx.device)
        j = make_job(c, frames if s_i == 0 else jobs[0].frames)
        j.plan()
        jobs.append(j)
        ctxs.append(c)
    job = jobs[0]

    def barrier():
        for c in ctxs:
            c.sync()
        if dist is not None:
            dist.barrier()

    def reduce_max(dt):
        return dt if dist is None else dist.all_reduce_max(dt)

    def run_step(i):
        return jobs[i % len(jobs)].run()

    dt_total, last = timed_steps(run_step, barrier, args.steps, args.warmup, len(jobs), reduce_max)
    ms_per_step = dt_total / args.steps * 1e3
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, last, rank, world)
    del last

    share = parity_n = None
    if args.full:
        # the spread of the headline: more rounds of exactly --steps steps (the headline's round first) until >= --min-seconds are timed
        rounds = [dt_total]
        if dt_total < args.min_seconds:
            rounds += timed_rounds(run_step, barrier, args.steps, 0, len(jobs), args.min_seconds - dt_total, reduce_max)

        # per-kernel durations: HIP events on the ctx stream, separate pass over the same steps
        ctx.prof_reset()
        ctx.prof_enable(True)
        for _ in range(max(1, args.profile_steps)):
            out = job.run()
            del out
        ctx.prof_enable(False)
        kernels = ctx.prof_results()
        ctx.prof_reset()

        # the same-family single-GPU rate (N > 1): this rank's share as an unsharded panorama of its own — no strips, no
        # exchange, the whole band; what `value / n_gpus` is to be compared with, since the N = 1 line is another geometry
        if world > 1:
            sj = [StitchJob(jobs[0].frames, cams, warper_type=wl["warper"], blender_type=wl["blender"], num_bands=nb, ctx=c) for c in ctxs]
            for j in sj:
                j.warper.set_scale(all_cams)
            sr = timed_rounds(lambda i: sj[i % len(sj)].run(), barrier, max(4, args.steps // 2), 1, len(sj), args.min_seconds / 2, reduce_max)
            share = fpg * W * H / 1e6 / (sum(sr) / (max(4, args.steps // 2) * len(sr)))
            del sj

        if world > 1 and not args.no_parity:  # every blender type shards (feather and "no": distributed.py, round 3)
            parity_n = sharded_parity(jobs[0], dist, rank, world, wl, all_cams)

    if rank != 0:
        if dist is not None:
            dist.barrier()
            dist.close()
        return

    src_mpix = n_total * W * H / 1e6
    wsz = job.plan_.sizes if world > 1 else job.warped_sizes
    warped_mpix = sum(w * h for w, h in wsz) / 1e6
    value = src_mpix / (ms_per_step / 1e3)
    bands_txt = f"{getattr(job, 'last_num_bands', wl['bands'])}-band " if wl["blender"] == "multiband" else ""
    result = {
        "metric": "warped+blended Mpix/s", "value": round(value, 1), "unit": "Mpix/s", "n_gpus": world,
        "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_per_step, 4), "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": "u8/int16 (fixed-point remap, int32 pyramid sums, fp32 weights)",
        "data": "synthetic",
        "steps_executed": args.steps,
        "config": {"workload": f"{wl['name']}; {wl['warper']} warp + {bands_txt}{wl['blender']} blend, inputs resident in HBM",
                   "baseline_config": wl["cfg"], "frames_per_gpu": fpg,
                   "sharding": ("contiguous yaw columns -> panorama column bands, "
                                + ("warped-image strips" if getattr(jobs[0], "exchange", "strips") == "strips" else "per-level contribution strips")
                                + f" over {jobs[0].transport.name} send/recv") if world > 1 else "single GPU",
                   "ranks_share_a_gpu": bool(shared and world > 1),
                   "panoramas_in_flight": len(jobs),
                   "warped_mpix_per_step": round(warped_mpix, 2),
                   "source_mpix_per_step": round(src_mpix, 2)},
    }
    if world > 1:
        p = job.plan_
        tr = jobs[0].transport
        result["config"]["transport"] = dict(name=tr.name, **(tr.info() if hasattr(tr, "info") else {}))  # rccl: ncclCommCount, ncclGetVersion
        result["config"]["exchange"] = {"messages": len(p.messages), "bytes_per_step": p.exchanged_bytes(),
                                        "rank0_sends_MB": round(sum(m[4] for m in p.sends(0)) / 1e6, 1),
                                        "busiest_link_MB": round(p.busiest_link_bytes() / 1e6, 1),  # xGMI is point to point
                                        "band_balance": p.balance, "band_edges": p.edges}
    if not args.full:
        print(json.dumps(result), flush=True)
        if dist is not None:
            dist.barrier()
            dist.close()
        return

    per_round = sorted(src_mpix * args.steps / r for r in rounds)
    kernels.sort(key=lambda k: -k["total_ms"])
    dom = kernels[0]
    avg_ms = dom["total_ms"] / dom["calls"]
    bytes_per_launch = dom["algo_bytes"] / dom["calls"]
    achieved = bytes_per_launch / (avg_ms / 1e3) / 1e9
    traffic, traffic_of, rocprof_us = None, {}, {}
    khash = kernel_source_hash()
    if args.traffic_json and os.path.exists(args.traffic_json):
        tj = json.load(open(args.traffic_json))
        # per-launch PMC bytes of the same kernels on the same workload AND the same kernel sources; anything else: null
        if tj.get("kernel_source_hash") == khash and tj.get("workload_cfg", 2) == wl["cfg"] and world == 1:
            traffic_of = {k: round(v["traffic_bytes"]) for k, v in tj.items() if isinstance(v, dict) and "traffic_bytes" in v}
            traffic = traffic_of.get(dom["kernel"])
            rocprof_us = tj.get("rocprofv3_avg_us", {})  # rocprofv3 --kernel-trace --stats of the same command on the same sources
    roofline = {"bound": "hbm", "kernel": dom["kernel"], "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS,
                "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": traffic,
                "avg_launch_us": round(avg_ms * 1e3, 2), "algo_bytes_per_launch": round(bytes_per_launch),
                "launches_per_step": dom["calls"] / max(1, args.profile_steps), "kernel_source_hash": khash}
    if dom["kernel"] in rocprof_us:
        # the same fraction from rocprofv3's average duration of this kernel (profiles/, another run on another box of the pool: the two
        # clocks agree within a few per cent)
        roofline["avg_launch_us_rocprofv3"] = rocprof_us[dom["kernel"]]
        roofline["frac_rocprofv3"] = round(bytes_per_launch / (rocprof_us[dom["kernel"]] * 1e-6) / 1e9 / HBM_PEAK_GBS, 4)
    ksum = sum(k["total_ms"] for k in kernels)
    kbytes = sum(k["algo_bytes"] for k in kernels)
    # the whole path against the same roofline: the algorithmic bytes of ALL kernels of a step over the step's wall time (with
    # --streams panoramas in flight) and over the summed kernel time of one panorama alone
    psteps = max(1, args.profile_steps)
    roofline["path_frac"] = {"algo_bytes_per_step": round(kbytes / psteps),
                             "over_wall": round(kbytes / psteps / (ms_per_step / 1e3) / 1e9 / HBM_PEAK_GBS, 4),
                             "over_kernel_sum": round(kbytes / max(ksum, 1e-9) / 1e6 / HBM_PEAK_GBS, 4)}
    rounds_s = sum(rounds)
    result.update({
        "timed_rounds": {"rounds": len(rounds), "steps_per_round": args.steps, "seconds": round(rounds_s, 4),
                         "value": round(src_mpix * args.steps * len(rounds) / rounds_s, 1),
                         "value_min": round(per_round[0], 1), "value_median": round(per_round[len(per_round) // 2], 1),
                         "value_max": round(per_round[-1], 1),
                         "note": "the headline's round of exactly --steps steps and more such rounds until >= %.2g s are timed; "
                                 "value = all steps / all time" % args.min_seconds},
        "roofline": roofline,
        "kernels": [{"kernel": k["kernel"], "calls_per_step": k["calls"] / max(1, args.profile_steps),
                     "avg_us": round(k["total_ms"] / k["calls"] * 1e3, 2),
                     "algo_GBps": round(k["algo_bytes"] / max(k["total_ms"], 1e-9) / 1e6, 1),
                     "frac_of_hbm_peak": round(k["algo_bytes"] / max(k["total_ms"], 1e-9) / 1e6 / HBM_PEAK_GBS, 4),
                     "algo_bytes_per_launch": round(k["algo_bytes"] / k["calls"]),
                     "traffic": traffic_of.get(k["kernel"])} for k in kernels],
        "all_kernels": {"sum_ms_per_step": round(ksum / max(1, args.profile_steps), 4),
                        "algo_GBps": round(kbytes / max(ksum, 1e-9) / 1e6, 1),
                        "frac_of_hbm_peak": round(kbytes / max(ksum, 1e-9) / 1e6 / HBM_PEAK_GBS, 4),
                        "note": "bytes the fused kernels move (algorithmic, per kernel) / summed kernel time: the bandwidth fraction of the path; "
                                "kernels[].traffic = HBM bytes per launch from the PMC passes (2 x FETCH_SIZE + WRITE_SIZE, mean over the launches "
                                "of that name), null unless the profile was taken on these very kernel sources"},
    })
    if parity_n is not None:
        result["parity"] = parity_n
    if world > 1:
        result["same_family_single_gpu"] = {
            "value_per_gpu": round(share, 1), "unit": "Mpix/s",
            "efficiency_vs_it": round(value / world / share, 4),
            "note": "slowest rank's rate on its own 4-frame (8-frame) share as an unsharded panorama, measured in this run: the "
                    "single-GPU rate of THIS geometry (the N = 1 line runs config 2, whose frames warp to 0.82 of their "
                    "source size; config 3's +-56 degree rows warp to 2.0 x)"}
    if world == 1 and hasattr(job, "corners") and wl["blender"] == "multiband":
        m = survey_8d_bytes(job.sizes, job.corners, job.warped_sizes, job.last_num_bands)
        gbps = m["total"] / (ms_per_step / 1e3) / 1e9
        result["model_speed_index"] = {
            "model": "SURVEY.md 8(d): bytes OpenCV's UNFUSED dataflow would move for this pass (maps not stored) / step time. "
                     "Not a bandwidth fraction of this implementation (the fused path moves about 2.3x fewer bytes): see "
                     "all_kernels.frac_of_hbm_peak and kernels[].frac_of_hbm_peak for that",
            "bytes_per_source_px": round(m["total"] / m["P_s"], 2), "bytes_per_step": round(m["total"]),
            "model_GBps": round(gbps, 1), "index_vs_8TBps": round(gbps / HBM_PEAK_GBS, 4),
            "P_s": m["P_s"], "P_w": m["P_w"], "P_f": m["P_f"], "P_d": m["P_d"]}
    if world == 1:
        # latency of ONE panorama: one stream, a device sync after every step
        lat_job = jobs[0]
        for _ in range(2):
            lat_job.run()
        ctx.sync()
        lats = []
        for _ in range(max(5, args.steps // 2)):
            t1 = time.perf_counter()
            out = lat_job.run()
            ctx.sync()
            lats.append(time.perf_counter() - t1)
            del out
        lats.sort()
        result["latency_ms_single_stream"] = {"median": round(lats[len(lats) // 2] * 1e3, 4), "min": round(lats[0] * 1e3, 4),
                                              "max": round(lats[-1] * 1e3, 4), "panoramas": len(lats)}
        # SURVEY 8(d) words the metric as "first warp launch -> panorama resident": that is this number; `value` is the throughput of
        # a stream of panoramas (--streams in flight)
        result["value_single_stream"] = round(src_mpix / lats[len(lats) // 2], 1)
        # the same number under the name VERDICT r5 asked for, next to `value` at the top level, and what each of the two is
        result["value_latency"] = result["value_single_stream"]
        result["value_definition"] = {"value": f"throughput of a stream of panoramas, {len(jobs)} in flight on {len(jobs)} HIP streams",
                                      "value_latency": "SURVEY 8(d)'s wording: source Mpix / (first warp launch -> panorama resident), one panorama alone"}
    if world == 1 and not args.no_extra:
        result["extra"] = extra_legs(args, S, synthetic, StitchJob, ctxs, wl, jobs[0], all_cams, frames)
    if world == 1 and args.e2e_steps > 0:
        result["pcie_inclusive"] = pcie_legs(args, S, StitchJob, ctxs, wl, frames, cams, src_mpix, nb)
    if world == 1 and not args.no_cpu_baseline:
        n_cpu = args.cpu_frames or len(frames)
        cb, o_pano, o_mask = cpu_baseline(wl, frames, cams, all_cams, n_cpu)
        result["cpu_baseline"] = cb
        if n_cpu >= len(frames):
            # the panorama of the timed path (same job object, same kernels) against the oracle's, byte for byte
            g_pano, g_mask = (np.asarray(a) for a in jobs[0].run())
            if g_pano.shape == o_pano.shape:
                d = np.abs(g_pano.astype(np.int16) - o_pano.astype(np.int16))
                result["parity"] = {"vs": "oracle (oracle/stx_oracle.cpp, default model: exact trig, scalar pyrDown order, Q15 remap)",
                                    "max_abs_diff": int(d.max()), "differing_bytes": int(np.count_nonzero(d)),
                                    "mask_equal": bool(np.array_equal(g_mask, o_mask)), "panorama_shape": list(g_pano.shape)}
            else:
                result["parity"] = {"vs": "oracle", "shape_mismatch": [list(g_pano.shape), list(o_pano.shape)]}
    print(json.dumps(result), flush=True)
    if dist is not None:
        dist.barrier()
        dist.close()


def quick_rate(jobs, ctxs, mpix, steps=6, warmup=2, min_seconds=0.25):
    def barrier():
        for c in ctxs:
            c.sync()

    r = timed_rounds(lambda i: jobs[i % len(jobs)].run(), barrier, steps, warmup, len(jobs), min_seconds, lambda x: x)
    ms = sum(r) / (steps * len(r)) * 1e3
    return {"value": round(mpix / (ms / 1e3), 1), "unit": "Mpix/s", "ms_per_step": round(ms, 4), "steps_executed": steps * len(r)}


def extra_legs(args, S, synthetic, StitchJob, ctxs, wl, job, all_cams, host_frames):
    """Other operating points on the same GPU, same timing method (two panoramas in flight), fewer steps.  Not `value`."""
    import numpy as np

    out = {}
    if wl["cfg"] == 2 and wl["blender"] == "multiband":
        src_mpix = sum(w * h for w, h in job.sizes) / 1e6
        # (ii) of SURVEY 8(d): Voronoi seam masks ANDed with the warped masks (binary, full resolution)
        S.set_device_resident(True)
        try:
            _, masks, _ = job.warper.warp_images_and_masks(job.frames, job.cameras)
            h_masks = [np.asarray(m) for m in masks]
        finally:
            S.set_device_resident(False)
        seams = synthetic.voronoi_seam_masks(h_masks, job.corners, job.warped_sizes)
        js = []
        for c in ctxs:
            j = StitchJob(job.frames, job.cameras, num_bands=wl["bands"], ctx=c, feed_masks=seams)  # host arrays: the job sees the cells
            j.warper.set_scale(all_cams)
            js.append(j)
        out["voronoi_seam_masks"] = dict(quick_rate(js, ctxs, src_mpix), note="full-resolution 0/255 seam masks fed instead of the warped masks; "
                                         "every image warped and fed only over the columns its seam cell can reach (StitchJob crop_to_masks)")
        # the reference's default pipeline: low-resolution seam masks resized per panorama (SeamFinder.resize) -> grey edges,
        # non-binary masks -> the fp32-weight level-0 kernel
        low = [np.ascontiguousarray(m[::11, ::11]) for m in seams]
        js = []
        for c in ctxs:
            j = StitchJob(job.frames, job.cameras, num_bands=wl["bands"], ctx=c, seam_masks=low)
            j.warper.set_scale(all_cams)
            js.append(j)
        out["resized_seam_masks"] = dict(quick_rate(js, ctxs, src_mpix),
                                         note="0.09-scale seam masks -> SeamFinder.resize on the device every step (dilate, "
                                              "INTER_LINEAR_EXACT, AND): non-binary masks, fp32-weight level-0 gather; cropped to the seam cells' reach")
        del js
        # The reference's DEFAULT composition (stitching/stitcher.py:22-48, run as :117-128): gain_blocks compensator (block gain maps
        # from the low-resolution pass: here smooth synthetic ones of the size BlocksCompensator makes for 0.1-Mpx images, 32-px blocks),
        # dp_color seam masks resized per panorama (here the Voronoi cells at 0.09 scale) and multiband at blend_strength 5 — the band
        # count comes out of the panorama size (stitching/blender.py:25-32), 7 for this one
        rng = np.random.default_rng(4242)
        lscale = (0.1e6 / (wl["width"] * wl["height"])) ** 0.5
        gmaps = []
        for k, (w_, h_) in enumerate(job.warped_sizes):
            gh, gw = (int(h_ * lscale) + 31) // 32 + 1, (int(w_ * lscale) + 31) // 32 + 1
            yy, xx = np.mgrid[0:gh, 0:gw]
            gmaps.append((1.0 + 0.12 * np.sin(0.7 * xx + k) * np.cos(0.5 * yy - k) + 0.02 * rng.standard_normal((gh, gw))).astype(np.float32))
        comp = S.ExposureErrorCompensator("gain_blocks")
        comp.set_gains(gmaps)
        js = []
        for c in ctxs:
            j = StitchJob(job.frames, job.cameras, blend_strength=5, ctx=c, seam_masks=low, compensator=comp)
            j.warper.set_scale(all_cams)
            js.append(j)
        leg = dict(quick_rate(js, ctxs, src_mpix), compensator="gain_blocks (batched, gain maps resident)", seam_masks="0.09 scale, resized on the device",
                   blend_strength=5, note="the reference's DEFAULT_SETTINGS composition on config 2's frames: warp -> gain_blocks apply -> "
                                          "SeamFinder.resize -> multiband; cropped to the seam cells' reach")
        leg["bands"] = js[0].last_num_bands
        if not args.no_cpu_baseline:
            o_pano, o_mask, o_bands = oracle_chain(wl, host_frames, job.cameras, all_cams, gain_maps=gmaps, low_seams=low, blend_strength=5)
            leg["parity"] = parity_record(js[0], o_pano, o_mask, "oracle chain: warp -> block_gain_apply -> seam_resize -> %d-band blend" % o_bands)
        out["reference_defaults"] = leg
        del js
        # The other arithmetic models the library offers (include/stitching_amd.h: STX_REMAP_*, STX_PYRDOWN_*, STX_TRIG_*), priced on the
        # same frames, each checked against the oracle under the same model
        modes = {}
        for name, setup, teardown, okw in (
            ("remap_float", lambda: S.set_remap_mode("float"), S.set_remap_mode, dict(model=dict(remap="float"))),
            ("pyrdown_simd_hv8", lambda: S.set_pyrdown_mode("simd-hv", 8), lambda p: S.set_pyrdown_mode(*p), dict(model=dict(pyrdown32f="simd_hv", lanes=8))),
            ("trig_glibc", lambda: S.set_trig_mode("glibc"), S.set_trig_mode, dict(trig=2)),  # oracle.TRIG_GLIBC,
        ):
            prev = setup()
            try:
                js = []
                for c in ctxs:
                    j = StitchJob(job.frames, job.cameras, num_bands=wl["bands"], ctx=c)
                    j.warper.set_scale(all_cams)
                    js.append(j)
                m = dict(quick_rate(js, ctxs, src_mpix))
                if not args.no_cpu_baseline:
                    o_pano, o_mask, _ = oracle_chain(wl, host_frames, job.cameras, all_cams, **okw)
                    m["parity"] = parity_record(js[0], o_pano, o_mask, "oracle under the same model")
                modes[name] = m
                del js
            finally:
                teardown(prev)
        out["modes"] = modes
    if wl["cfg"] == 2:
        # BASELINE configs[3] (config 4), one GPU's share: 8 x 8000x6000, cylindrical, 7 bands
        cams4 = synthetic.grid_cameras(2, 4, 8000, 6000, max_edge_lat_deg=50.0, layout_yaw=16)
        fr4 = [S.DeviceImage.from_numpy(synthetic.make_frame(100 + i, 8000, 6000), ctxs[0]) for i in range(8)]
        js = [StitchJob(fr4, cams4, warper_type="cylindrical", num_bands=7, ctx=c) for c in ctxs]
        out["config4_share"] = dict(quick_rate(js, ctxs, 8 * 48.0, steps=4), bands=7,
                                    note="8 x 8000x6000 (2 of 16 yaw columns x 4 pitch rows), cylindrical warp + 7-band blend")
        del js, fr4
        # BASELINE configs[4] (config 5): 16 affine scan tiles, feather / no
        cams5 = synthetic.affine_scan_cameras(16, 4000, 3000)
        fr5 = [S.DeviceImage.from_numpy(synthetic.make_frame(i, 4000, 3000), ctxs[0]) for i in range(16)]
        for bt in ("feather", "no"):
            js = [StitchJob(fr5, cams5, warper_type="affine", blender_type=bt, ctx=c) for c in ctxs]
            out[f"config5_{bt}"] = dict(quick_rate(js, ctxs, 16 * 12.0, steps=4), note=f"16 affine scan tiles 4000x3000, {bt} blender")
        del js, fr5
    return out


def pcie_legs(args, S, StitchJob, ctxs, wl, frames, cams, src_mpix, nb):
    """PCIe-inclusive rates (never `value`): host numpy frames in, host panorama out."""
    import numpy as np

    from stitching_amd import pinned_empty
    from stitching_amd.pipeline import stitch

    kw = dict(warper_type=wl["warper"], blender_type=wl["blender"], num_bands=nb)
    stitch(frames, cams, **kw)
    t1 = time.perf_counter()
    for _ in range(args.e2e_steps):
        stitch(frames, cams, **kw)
    e2e = (time.perf_counter() - t1) / args.e2e_steps
    res = {"value": round(src_mpix / e2e, 1), "unit": "Mpix/s", "ms_per_step": round(e2e * 1e3, 2),
           "note": "pageable numpy frames H2D + roi sync + panorama D2H every step; not `value`"}
    # the same with page-locked frames (a decoder writing into stitching_amd.pinned_empty arrays) and a page-locked panorama buffer
    pframes = []
    for f in frames:
        pf = pinned_empty(f.shape, f.dtype)
        np.copyto(pf, f)
        pframes.append(pf)
    pout = {}

    def pinned_step():
        pano, pmask = StitchJob(pframes, cams, **kw).run()
        for key, d in (("pano", pano), ("mask", pmask)):
            if key not in pout or pout[key].shape != d.shape:
                pout[key] = pinned_empty(d.shape, d.dtype)
            d.numpy(out=pout[key])

    pinned_step()
    t1 = time.perf_counter()
    for _ in range(args.e2e_steps):
        pinned_step()
    e2p = (time.perf_counter() - t1) / args.e2e_steps
    res["pinned"] = {"value": round(src_mpix / e2p, 1), "ms_per_step": round(e2p * 1e3, 2)}
    # ... and as a stream of panoramas alternating between two contexts with queued (asynchronous) uploads and
    # read-backs: the upload of one panorama overlaps the read-back of the previous one (both PCIe directions busy)
    if len(ctxs) >= 2:
        pouts = [dict(), dict()]

        def piped_step(i):
            c, po = ctxs[i % 2], pouts[i % 2]
            c.sync()  # this context's previous panorama has landed in its host buffers
            pano, pmask = StitchJob(pframes, cams, ctx=c, async_upload=True, **kw).run()
            for key, d in (("pano", pano), ("mask", pmask)):
                if key not in po or po[key].shape != d.shape:
                    po[key] = pinned_empty(d.shape, d.dtype)
                d.numpy(out=po[key], wait=False)

        for i in range(2):
            piped_step(i)
        for c in ctxs[:2]:
            c.sync()
        n_piped = 2 * max(2, args.e2e_steps)
        t1 = time.perf_counter()
        for i in range(n_piped):
            piped_step(i)
        for c in ctxs[:2]:
            c.sync()
        e2q = (time.perf_counter() - t1) / n_piped
        same = all(np.array_equal(pouts[k]["pano"], pout["pano"]) for k in range(2))
        res["pinned_pipelined"] = {"value": round(src_mpix / e2q, 1), "ms_per_step": round(e2q * 1e3, 2),
                                   "equals_synchronous_result": bool(same)}
    return res


if __name__ == "__main__":
    main()
