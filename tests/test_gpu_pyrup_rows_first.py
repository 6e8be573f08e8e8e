"""pyrUp rows-first in the packed gathers and the level-0 gather's direct store of uncovered tiles, on the MI355X: the scenes of
tests/pyrup_rows_first_scenes.py through the multi-band blender of the C ABI, each once as a first run (the searching kernels) and as the
panoramas of a known rig — a keeper, then adopters that replay (the calls StitchJob.run makes on its blender: keep_weights / use_weights) —
with 0 differing bytes against the oracle in the u8 panorama, the mask and the int16 panorama; the adopters with and without the int16
panorama.  One StitchJob on a ring of two cameras with 1.9 k uncovered columns between them against a job that keeps nothing.
What the scenes reach, and why coarse heights 1, 2 and odd ones are the CPU test's, is in the scenes' module."""
import ctypes as C
import functools

import numpy as np
import pytest

import stitching_amd as S
from oracle import oracle as O
from stitching_amd import _lib, synthetic
from stitching_amd.blender import _BlenderHandle
from stitching_amd.pipeline import StitchJob
from tests import constructed_multiband as CM
from tests import pyrup_rows_first_scenes as PS

pytestmark = pytest.mark.gpu

CASES = [("edges", 3), ("edges", 4), ("holes", 3), ("holes", 4), ("holes", 3, True), ("holes", 4, True)]


@functools.lru_cache(maxsize=None)
def _case(builder, *args):
    """(scene, the oracle's int16 panorama, u8 panorama, mask): made once per case, read-only"""
    scene = getattr(PS, builder)(*args)
    b = O._OracleBlenderHandle(CM.MULTIBAND, scene.bands, 0.0)
    b.prepare(scene.roi)
    assert b.num_bands() == scene.B
    for img, mask, corner in scene.feeds:
        b.feed(np.asarray(img).astype(np.int16), mask, corner)
    out16, mask = b.blend()
    out8 = O.convert_scale_abs(out16)
    for a in (out16, out8, mask):
        a.setflags(write=False)
    return scene, out16, out8, mask


def _replayed(ctx):
    n = C.c_int(-1)
    assert ctx._lib.stx_debug_blend_replayed(ctx.handle, C.byref(n)) == 0
    return n.value


def _blend(ctx, scene, feeds, keep=False, use=None, want_s16=True):
    b = _BlenderHandle(ctx, _lib.BLEND_MULTIBAND, scene.bands, 0.0, scene.roi)
    assert b.num_bands() == scene.B
    for img, mask, corner in feeds:
        b.feed(img, mask, corner)
    kept = b.keep_weights() if keep else None
    if use is not None:
        assert b.use_weights(use) is True
    got = [d.numpy() for d in b.blend(want_s16=want_s16)]
    return got, kept, _replayed(ctx)


def _assert_bytes(got, case, what):
    _, want16, want8, wantm = case
    for name, g, w in (("u8 panorama", got[0], want8), ("mask", got[1], wantm)) + ((("int16 panorama", got[2], want16),) if len(got) > 2 else ()):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        diff = np.argwhere(g != w)
        assert len(diff) == 0, "%s, %s: %d differing values, the first at %s: %s against the oracle's %s" % (
            what, name, len(diff), tuple(int(v) for v in diff[0]), g[tuple(diff[0])], w[tuple(diff[0])])


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_first_run_and_known_rig_against_the_oracle(gpu_ctx, case):
    case = _case(*case)
    scene = case[0]
    feeds = [(S.DeviceImage.from_numpy(i, gpu_ctx), S.DeviceImage.from_numpy(m, gpu_ctx), c) for i, m, c in scene.feeds]
    got, _, replayed = _blend(gpu_ctx, scene, feeds)
    assert replayed == 0
    _assert_bytes(got, case, "first run")
    got, kept, replayed = _blend(gpu_ctx, scene, feeds, keep=True)
    assert kept is not None and replayed == 0
    _assert_bytes(got, case, "keeper")
    for want_s16 in (True, False, True):
        got, _, replayed = _blend(gpu_ctx, scene, feeds, use=kept, want_s16=want_s16)
        assert replayed == scene.B - 2, "every packed gather of an adopter replays"
        _assert_bytes(got, case, "adopter%s" % ("" if want_s16 else " without the int16 panorama"))
    kept.free()


def test_a_job_with_uncovered_tile_columns_between_two_cameras(gpu_ctx):
    """two frames 340 degrees apart: whole 512-column tiles of the panorama between them lie under no image; the known-rig runs (replay,
    no mask store) equal the runs of a job that keeps nothing"""
    n, w, h, bands = 2, 320, 240, 3
    cams = synthetic.ring_cameras(n, w, h, focal_factor=1.5, span_deg=340.0)
    sets = [[S.DeviceImage.from_numpy(synthetic.make_frame(10 * k + i, w, h), gpu_ctx) for i in range(n)] for k in range(3)]
    job = StitchJob(sets[0], cams, warper_type="spherical", num_bands=bands, ctx=gpu_ctx)
    control = StitchJob(sets[0], cams, warper_type="spherical", num_bands=bands, ctx=gpu_ctx, reuse_geometry=False)
    for k in range(3):
        want = [np.asarray(a) for a in control.run(sets[k])]
        got = [np.asarray(a) for a in job.run(sets[k])]
        assert job.last_reused == (k > 0) and job.last_weights_adopted == (k > 0) and job.last_num_bands == bands
        assert _replayed(gpu_ctx) == (bands - 2 if k > 0 else 0)
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0]), f"run {k}"
    x0 = min(c[0] for c in job.corners)
    spans = sorted((c[0] - x0, c[0] - x0 + s[0]) for c, s in zip(job.corners, job.warped_sizes))
    free = [t for t in range(0, spans[-1][1], 512) if not any(a < t + 512 and b > t for a, b in spans)]
    assert len(free) >= 2, (spans, "no tile column without an image")
    assert not want[1][:, free[0]:free[0] + 512].any() and not want[0][:, free[0]:free[0] + 512].any()
