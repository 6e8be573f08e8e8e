"""A step of a known rig launches pixel work only (StitchJob with reuse_geometry, pipeline.py): the warp's column / row tables are kept in
the job's geometry (stx_warp_tables), the blender's descriptor table is resident in the weights handle, and the panorama mask is the
one the first run made.  Four runs of a job on four 320 x 240 frames (spherical, 4 bands) with new frames each, against a job that keeps
nothing: every panorama and mask byte for byte, and the counters of include/stitching_amd_debug.h."""
import ctypes as C

import numpy as np
import pytest

import stitching_amd as S
from stitching_amd import synthetic
from stitching_amd.pipeline import StitchJob

pytestmark = pytest.mark.gpu

N, W, H, BANDS = 4, 320, 240, 4


def frames(run):
    return [synthetic.make_frame(10 * run + i, W, H) for i in range(N)]


def hooks(ctx):
    out = []
    for name in ("stx_debug_warp_table_launches", "stx_debug_blend_uploads", "stx_debug_blend_mask_stored", "stx_debug_blend_replayed"):
        n = C.c_int(-1)
        assert getattr(ctx._lib, name)(ctx.handle, C.byref(n)) == 0
        out.append(n.value)
    return tuple(out)


def run(job, sets, k):
    pano, mask = job.run(sets[k])
    return np.asarray(pano), np.asarray(mask), hooks(job.ctx)


def test_a_known_rig_repeats_nothing_that_the_pixels_do_not_change(gpu_ctx):
    cams = synthetic.ring_cameras(N, W, H, span_deg=120.0)
    # every run's frames on the device beforehand: a run then allocates what a step of a rig allocates and nothing else, so the blocks it is
    # handed — the addresses in the blender's descriptor table — are the previous run's
    sets = [[S.DeviceImage.from_numpy(f, gpu_ctx) for f in frames(k)] for k in range(6)]
    job = StitchJob(sets[0], cams, warper_type="spherical", num_bands=BANDS, ctx=gpu_ctx)
    control = StitchJob(sets[0], cams, warper_type="spherical", num_bands=BANDS, ctx=gpu_ctx, reuse_geometry=False)
    want = [run(control, sets, k) for k in range(6)]
    assert all(w[2] == (1, 1, 1, 0) for w in want), "the control makes tables, uploads and stores the mask every run"
    assert not np.array_equal(want[0][0], want[1][0])

    got = [run(job, sets, k) for k in range(4)]
    assert job.last_reused and job.last_weights_adopted and job.last_num_bands == BANDS
    for k in range(4):
        assert np.array_equal(got[k][1], want[k][1]) and np.array_equal(got[k][0], want[k][0]), f"run {k}"
    assert got[0][2] == (1, 1, 1, 0), "a first run"
    for k in (1, 2, 3):
        tables, _, mask_stored, replayed = got[k][2]
        assert (tables, mask_stored, replayed) == (0, 0, BANDS - 2), f"run {k}"
    assert sum(g[2][1] for g in got) <= 2, "the keeper's table and one resident copy"

    job.release_geometry()
    again = [run(job, sets, k) for k in (4, 5)]
    assert again[0][2] == (1, 1, 1, 0), "after release_geometry() a first run again"
    assert again[1][2][0] == 0 and again[1][2][2] == 0
    for r, k in zip(again, (4, 5)):
        assert np.array_equal(r[1], want[k][1]) and np.array_equal(r[0], want[k][0]), f"run {k}"
