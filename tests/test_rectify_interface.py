"""The host side of lens rectification that needs no device: every refusal is raised before anything is uploaded or launched, one
LensMap is broadcast over a list, and the `lenses=` keyword of Composer's four methods."""
import ctypes as C
import inspect

import numpy as np
import pytest

import stitching_amd as S
from stitching_amd import _lib
from stitching_amd.rectify import lens_list, node_counts

K = np.array([[70.0, 0.0, 47.3], [0.0, 70.0, 35.6], [0.0, 0.0, 1.0]])
DIST = (-0.25, 0.06, 0.001, -0.0008, -0.01)
SRC = (96, 72)


class NoDevice:
    """a context that fails the test when anything reaches for the device"""

    def __getattr__(self, name):
        raise AssertionError(f"the refusal came too late: the context was asked for {name}")


def lens(**kw):
    return S.LensMap.brown(K, DIST, SRC, **kw)


def frame(size=SRC, c=3, dtype=np.uint8):
    w, h = size
    return np.zeros((h, w) if c == 1 else (h, w, c), dtype)


class Foreign:
    def __init__(self, shape, typestr="|u1"):
        self.__cuda_array_interface__ = {"version": 3, "shape": shape, "typestr": typestr, "data": (0x7F0000001000, False), "strides": None}


# ---- LensMap ----------------------------------------------------------------------------------------------------------------------
def test_lens_map_surface():
    m = lens(dst_size=(70, 37))
    assert m.src_size == SRC and m.dst_size == (70, 37) and m.new_K.shape == (3, 3)
    assert m.nodes.dtype == np.int32 and m.nodes.shape == (4, 6, 2) and node_counts((70, 37)) == (6, 4)
    assert not m.nodes.flags.writeable and isinstance(m.error(), float)
    plain = S.LensMap(m.nodes, SRC, (70, 37))
    assert np.array_equal(plain.nodes, m.nodes) and plain.new_K is None
    with pytest.raises(S.StitchingError, match="no exact model"):
        plain.error()


@pytest.mark.parametrize("make,match", [
    (lambda: S.LensMap(np.zeros((4, 5, 2), np.int32), SRC, (70, 37)), "nodes of shape"),          # the node count does not match (W, H)
    (lambda: S.LensMap(np.zeros((4, 6, 2), np.float32), SRC, (70, 37)), "integer nodes"),
    (lambda: S.LensMap(np.full((4, 6, 2), 1 << 22, np.int64), SRC, (70, 37)), "Q6"),
    (lambda: S.LensMap(np.zeros((2, 1026, 2), np.int32), SRC, (16385, 1)), "1 .. 16384"),          # a side above 16 384
    (lambda: lens(dst_size=(16, 16385)), "1 .. 16384"),
    (lambda: S.LensMap.brown(K, DIST, (16385, 72)), "1 .. 16384"),
    (lambda: S.LensMap.from_maps(np.zeros((1, 16385)), np.zeros((1, 16385)), SRC), "1 .. 16384"),
    (lambda: lens(dst_size=(0, 5)), "1 .. 16384"),
    (lambda: S.LensMap.brown(K, DIST[:3], SRC), "4, 5 or 8"),
    (lambda: S.LensMap.brown(K[:2], DIST, SRC), "3 x 3"),
    (lambda: S.LensMap.fisheye(K, DIST, SRC), "four"),
    (lambda: lens(fit="outside"), "fit"),
    (lambda: S.LensMap.brown(K, (np.nan, 0, 0, 0), SRC), "finite"),
    (lambda: S.LensMap.from_maps(np.full((5, 5), np.inf), np.zeros((5, 5)), SRC), "not finite"),  # a refusal, not a clip
    (lambda: S.LensMap.from_maps(np.zeros((5, 5)), np.zeros((5, 6)), SRC), "one shape"),
])
def test_lens_map_refusals(make, match):
    with pytest.raises(S.StitchingError, match=match):
        make()


# ---- rectify_all: refused on the host, before the context is touched ------------------------------------------------------------------
@pytest.mark.parametrize("frames,lenses,kw,match", [
    ([frame(), frame()], [lens()], {}, "1 lenses for 2 frames"),                    # the counts differ
    ([frame()], [lens(), lens()], {}, "2 lenses for 1 frames"),
    ([frame()], [K], {}, "not a LensMap"),
    ([frame()], 5, {}, "LensMap or a sequence"),
    ([frame()], lens(), {"border": "reflect"}, "border"),
    ([frame(dtype=np.int16)], lens(), {}, "u8 with 1 or 3 channels"),               # not u8
    ([frame(dtype=np.float32, c=1)], lens(), {}, "u8 with 1 or 3 channels"),
    ([frame(c=4)], lens(), {}, "4 channel"),                                       # not 1 or 3 channels
    ([frame(c=2)], lens(), {}, "2 channel"),
    ([frame((95, 72))], lens(), {}, "95x72, its lens was made for 96x72"),          # not the map's source size
    ([frame(), frame((96, 71), c=1)], lens(), {}, "frame 1 is 96x71"),
    ([Foreign((72, 96, 4))], lens(), {}, "4 channel"),                              # a foreign array is judged by its interface
    ([Foreign((72, 96, 3), "<f4")], lens(), {}, "u8 with 1 or 3 channels"),
    ([Foreign((72, 95, 3))], lens(), {}, "95x72"),
])
def test_rectify_refuses_before_the_device(frames, lenses, kw, match):
    with pytest.raises(S.StitchingError, match=match):
        S.rectify_all(frames, lenses, ctx=NoDevice(), **kw)


def test_rectify_of_one_frame_refuses_alike():
    with pytest.raises(S.StitchingError, match="its lens was made for"):
        S.rectify(frame((10, 10)), lens(), ctx=NoDevice())
    with pytest.raises(S.StitchingError, match="not a LensMap"):
        S.rectify(frame(), None, ctx=NoDevice())


def test_nothing_to_do_needs_no_device():
    assert S.rectify_all([], [], ctx=NoDevice()) == []
    assert S.rectify_all([], lens(), masks=True, ctx=NoDevice()) == ([], [])


def test_one_lens_is_broadcast():
    m = lens()
    got = lens_list(m, 3)
    assert len(got) == 3 and all(g is m for g in got)
    assert lens_list([m, m], 2) == [m, m] and lens_list(m, 0) == []
    # ... and rectify_all takes it that way: the second frame, not the count, is what is refused
    with pytest.raises(S.StitchingError, match="frame 1 is 10x10"):
        S.rectify_all([frame(), frame((10, 10))], m, ctx=NoDevice())


# ---- the C entry points: null handles are refused with a message, before any HIP call -----------------------------------------------
def test_c_entry_points_refuse_null_handles():
    L = _lib.lib()
    out = C.c_void_p()
    nodes = np.zeros((2, 2, 2), np.int32)
    ptr = nodes.ctypes.data_as(C.POINTER(C.c_int))
    assert L.stx_lens_map_create(None, 16, 16, 16, 16, 2, 2, ptr, C.byref(out)) != 0 and b"null" in L.stx_last_error()
    assert out.value is None
    one = (C.c_void_p * 1)()
    assert L.stx_rectify(None, 1, one, one, 0, 0, one, None) != 0 and b"null" in L.stx_last_error()
    assert L.stx_lens_map_free(None) == 0
    assert {"stx_lens_map_create", "stx_lens_map_free", "stx_rectify"} <= set(_lib.EXPORTS)


# ---- Composer ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", [S.Composer, S.AffineComposer])
@pytest.mark.parametrize("method", ["prepare", "run", "compose", "stitch"])
def test_lenses_keyword_defaults_to_none(cls, method):
    p = inspect.signature(getattr(cls, method)).parameters
    assert "lenses" in p and p["lenses"].default is None


@pytest.mark.parametrize("cls", [S.Composer, S.AffineComposer])
def test_composer_refuses_a_wrong_count_of_lenses(cls):
    composer = cls(ctx=NoDevice())
    frames = [frame(), frame(), frame()]
    cameras = [object()] * 3
    with pytest.raises(S.StitchingError, match="2 lenses for 3 frames"):
        composer.prepare(frames, cameras, lenses=[lens(), lens()])
    with pytest.raises(S.StitchingError, match="2 lenses for 3 frames"):
        composer.compose(frames, cameras, lenses=[lens(), lens()])
    with pytest.raises(S.StitchingError, match="2 lenses for 3 frames"):
        composer.stitch(frames, lenses=[lens(), lens()])
    with pytest.raises(S.StitchingError, match="2 lenses for 3 frames"):
        composer.run(None, images=frames, lenses=[lens(), lens()])
    with pytest.raises(S.StitchingError, match="lenses go with new images"):
        composer.run(None, lenses=[lens()])


def test_plan_checks_distorted_sizes_against_the_lenses():
    plan = S.ComposePlan.__new__(S.ComposePlan)
    plan.frame_sizes = [(70, 37), (70, 37)]
    good = lens(dst_size=(70, 37))
    plan.check_frames([frame(), frame()], [good, good])
    with pytest.raises(S.StitchingError, match="the lenses were made for"):
        plan.check_frames([frame(), frame((70, 37))], [good, good])
    with pytest.raises(S.StitchingError, match="the lenses rectify to"):
        plan.check_frames([frame(), frame()], [good, lens()])
    plan.check_frames([frame((70, 37)), frame((70, 37))])  # without lenses: the rule as it was
    with pytest.raises(S.StitchingError, match="same rig, same sizes"):
        plan.check_frames([frame(), frame()])
