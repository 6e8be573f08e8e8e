"""The warp through the lens without a GPU: what Python refuses before any context exists — lens_mode strings, "fused" without lenses or
with a final_megapix that resizes the frames, counts of frames, lenses and cameras — and that lens_mode="rectify" and lenses=None call
nothing new: with the library handle replaced by a recorder, neither ever reaches stx_warp_lens_batch."""
import numpy as np
import pytest

import stitching_amd as S
from stitching_amd import _lib, pipeline
from stitching_amd.camera import CameraParams
from stitching_amd.pipeline import Composer, check_final_size, check_lens_mode

SIZE = (96, 72)
K = np.array([[70.0, 0.0, 48.0], [0.0, 70.0, 36.0], [0.0, 0.0, 1.0]])


def lens(dst_size=None):
    return S.LensMap.brown(K, (-0.25, 0.06, 0.001, -0.0008, -0.01), SIZE, dst_size=dst_size)


def frames(n=2):
    return [np.zeros((SIZE[1], SIZE[0], 3), np.uint8) for _ in range(n)]


def cams(n=2):
    return [CameraParams(focal=70.0, aspect=1.0, ppx=48.0, ppy=36.0, R=np.eye(3, dtype=np.float32)) for _ in range(n)]


def test_lens_mode_strings():
    assert pipeline.LENS_MODES == ("rectify", "fused")
    assert check_lens_mode("rectify", None) is False and check_lens_mode("rectify", [lens()]) is False
    assert check_lens_mode("fused", [lens()]) is True
    for bad in ("Fused", "fuse", "", "lens", None, 1):
        with pytest.raises(S.StitchingError, match="lens_mode"):
            check_lens_mode(bad, [lens()])
    with pytest.raises(S.StitchingError, match="needs lenses"):
        check_lens_mode("fused", None)


@pytest.mark.parametrize("call", ["prepare", "compose", "stitch", "module"])
def test_every_entry_refuses_a_wrong_mode_before_it_needs_a_device(call, monkeypatch):
    monkeypatch.setattr(pipeline, "get_context", lambda *a, **k: pytest.fail("a context was asked for"))
    c = Composer(finder="voronoi")
    fn = {"prepare": lambda **kw: c.prepare(frames(), cams(), **kw), "compose": lambda **kw: c.compose(frames(), cams(), **kw),
          "stitch": lambda **kw: c.stitch(frames(), **kw), "module": lambda **kw: pipeline.compose(frames(), cams(), **kw)}[call]
    with pytest.raises(S.StitchingError, match="one of"):
        fn(lenses=lens(), lens_mode="both")
    with pytest.raises(S.StitchingError, match="needs lenses"):
        fn(lens_mode="fused")


def test_fused_with_a_final_megapix_that_resizes_is_refused(monkeypatch):
    monkeypatch.setattr(pipeline, "get_context", lambda *a, **k: pytest.fail("a context was asked for"))
    check_final_size(-1, [SIZE, SIZE])
    check_final_size(1.0, [SIZE, SIZE])  # 1 megapixel is more than 96 x 72: never enlarged, nothing resized
    with pytest.raises(S.StitchingError, match="final_megapix=0.003"):
        check_final_size(0.003, [SIZE, SIZE])
    with pytest.raises(S.StitchingError, match="lens belongs to the frame's own size"):
        Composer(finder="voronoi", final_megapix=0.003, medium_megapix=0.002, low_megapix=0.001).prepare(frames(), cams(), lenses=lens(),
                                                                                                        lens_mode="fused")
    # the rectified size decides, not the source's: 0.005 megapixels hold 80 x 60, not 96 x 72
    check_final_size(0.005, [(80, 60), (80, 60)])
    with pytest.raises(S.StitchingError, match="final_megapix"):
        check_final_size(0.005, [SIZE, SIZE])


def test_counts_of_frames_lenses_and_cameras(monkeypatch):
    monkeypatch.setattr(pipeline, "get_context", lambda *a, **k: pytest.fail("a context was asked for"))
    monkeypatch.setattr(S.warper, "get_context", lambda *a, **k: pytest.fail("a context was asked for"))
    c = Composer(finder="voronoi")
    with pytest.raises(S.StitchingError, match="3 lenses for 2 frames"):
        c.prepare(frames(), cams(), lenses=[lens()] * 3, lens_mode="fused")
    with pytest.raises(S.StitchingError, match="not a LensMap"):
        c.prepare(frames(), cams(), lenses=[lens(), "brown"], lens_mode="fused")
    with pytest.raises(S.StitchingError, match="1 lenses for 2 frames"):
        pipeline.StitchJob(frames(), cams(), lenses=[lens()])
    w = S.Warper("spherical")
    w.set_scale(cams())
    with pytest.raises(S.StitchingError, match="1 lenses for 2 frames"):
        w.warp_images_through_lenses(frames(), [lens()], cams())
    with pytest.raises(S.StitchingError, match="3 cameras for 2 frames"):
        w.warp_images_through_lenses(frames(), lens(), cams(3))


class Recorder:
    """stands where the library handle does: every entry point called through it is noted and fails (there is no device)"""

    def __init__(self):
        self.called = []

    def __getattr__(self, name):
        def fn(*args):
            self.called.append(name)
            return -1
        return fn


class FakeContext:
    def __init__(self):
        self._lib, self.handle = Recorder(), 1


@pytest.mark.parametrize("lenses", [None, "one"])
def test_rectify_mode_and_no_lenses_never_reach_the_new_entry(lenses, monkeypatch):
    assert "stx_warp_lens_batch" in _lib.PROTOTYPES
    ctx = FakeContext()
    monkeypatch.setattr(_lib, "lib", lambda: ctx._lib)
    for mod in (pipeline, S.warper, S.device, S.rectify):
        if hasattr(mod, "get_context"):
            monkeypatch.setattr(mod, "get_context", lambda *a, **k: ctx)
    c = Composer(finder="voronoi", ctx=ctx)
    kw = {} if lenses is None else {"lenses": lens()}
    for fn in (lambda: c.prepare(frames(), cams(), lens_mode="rectify", **kw), lambda: c.compose(frames(), cams(), **kw),
               lambda: pipeline.compose(frames(), cams(), ctx=ctx, **kw), lambda: pipeline.StitchJob(frames(), cams(), ctx=ctx).run()):
        with pytest.raises(Exception):
            fn()  # the recorder's entry points all fail: the first device call ends the attempt
    assert ctx._lib.called and "stx_warp_lens_batch" not in ctx._lib.called
    # (an attempt ends at its first device call here; tests/test_gpu_lens_warp.py runs both modes to the end with the new code paths
    # booby-trapped)
