"""The host side of device frame emit that needs no device: what each format makes of an image, and every refusal of the Python layer
— read-only targets, shapes and dtypes that do not fit, plane counts, alpha, streams — against constructed objects."""
import ctypes as C
import types

import pytest

import stitching_amd as S
from stitching_amd import _lib
from stitching_amd.emit import plane_shapes, target_planes

PTR = 0x7F0000001000
U8 = _lib.U8


class Obj:
    """the least a foreign device array is: an object with the dict"""

    def __init__(self, shape, typestr="|u1", strides=None, ptr=PTR, read_only=False, **more):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (ptr, read_only), "version": 3, "strides": strides}
        self.__cuda_array_interface__.update(more)


def image(h, w, c=3, elem=U8):
    """what emit_all sees of a DeviceImage before the C call: its geometry and its handle — no device behind it"""
    im = object.__new__(S.DeviceImage)
    im.ctx, im._h = types.SimpleNamespace(handle=None), C.c_void_p(0)  # a closed context: nothing to free
    im.height, im.width, im.channels, im._elem, im.stride_bytes = h, w, c, elem, (w * c + 63) // 64 * 64
    return im


# ---- what a format makes of an image ------------------------------------------------------------------------------------------------
def test_plane_shapes_of_every_format():
    assert plane_shapes("bgr", 5, 7) == [(5, 7, 3, U8)] and plane_shapes("rgb", 5, 7) == [(5, 7, 3, U8)]
    assert plane_shapes("bgra", 5, 7) == [(5, 7, 4, U8)] and plane_shapes("rgba", 5, 7) == [(5, 7, 4, U8)]
    assert plane_shapes("gray", 5, 7, 1) == [(5, 7, 1, U8)]
    assert plane_shapes("nv12", 5, 7) == [(5, 7, 1, U8), (3, 4, 2, U8)]
    assert plane_shapes("i420", 6, 8) == [(6, 8, 1, U8), (3, 4, 1, U8), (3, 4, 1, U8)]
    assert plane_shapes("nv12", 1, 1) == [(1, 1, 1, U8), (1, 1, 2, U8)]
    for c, elem in ((1, U8), (2, U8), (3, _lib.S16), (4, _lib.F32)):
        assert plane_shapes(None, 5, 7, c, elem) == [(5, 7, c, elem)]


@pytest.mark.parametrize("fmt,c,elem,match", [
    ("bgr", 1, U8, "3 channel"), ("rgb", 4, U8, "3 channel"), ("bgra", 4, U8, "3 channel"), ("nv12", 1, U8, "3 channel"),
    ("i420", 3, _lib.S16, "u8"), ("gray", 3, U8, "1 channel"), ("gray", 1, _lib.F32, "u8"), ("yuyv", 3, U8, "unknown pixel format"),
])
def test_source_layouts_that_do_not_fit_the_format(fmt, c, elem, match):
    with pytest.raises(S.StitchingError, match=match):
        plane_shapes(fmt, 4, 6, c, elem)
    with pytest.raises(S.StitchingError, match=match):
        S.emit(image(4, 6, c, elem), fmt, ctx=object())


# ---- targets --------------------------------------------------------------------------------------------------------------------------
def test_accepted_targets():
    assert target_planes(Obj((4, 6, 3), strides=(31, 3, 1)), "bgr", 4, 6) == [(PTR, 4, 6, 3, U8, 31, None)]
    assert target_planes(Obj((4, 6, 4)), "rgba", 4, 6)[0][3:6] == (4, U8, 24)
    assert target_planes(Obj((4, 6)), "gray", 4, 6, 1)[0][1:4] == (4, 6, 1)
    assert target_planes(Obj((4, 6, 1)), "gray", 4, 6, 1)[0][1:4] == (4, 6, 1)
    assert target_planes(Obj((4, 6, 2), "<f4"), None, 4, 6, 2, _lib.F32)[0][3:5] == (2, _lib.F32)
    y, uv = target_planes((Obj((5, 7), strides=(11, 1)), Obj((3, 4, 2), ptr=PTR + 4096)), "nv12", 5, 7)
    assert y[:6] == (PTR, 5, 7, 1, U8, 11) and uv[:6] == (PTR + 4096, 3, 4, 2, U8, 8)
    planes = target_planes([Obj((5, 7)), Obj((3, 4), ptr=PTR + 4096), Obj((3, 4), ptr=PTR + 8192)], "i420", 5, 7)
    assert [p[1:4] for p in planes] == [(5, 7, 1), (3, 4, 1), (3, 4, 1)]
    y, uv = target_planes(Obj((6, 8), stream=7), "nv12", 4, 8)  # the single contiguous array
    assert y == (PTR, 4, 8, 1, U8, 8, 7) and uv == (PTR + 32, 2, 4, 2, U8, 8, 7)


@pytest.mark.parametrize("target,fmt,hw,match", [
    (Obj((4, 6, 3), read_only=True), "bgr", (4, 6), "read-only"),
    ((Obj((4, 6)), Obj((2, 3, 2), read_only=True)), "nv12", (4, 6), "read-only"),
    (Obj((6, 8), read_only=True), "nv12", (4, 8), "read-only"),
    (Obj((4, 6, 4)), "bgr", (4, 6), "image plane"),           # the channels of another format
    (Obj((4, 6, 3)), "bgra", (4, 6), "image plane"),
    (Obj((4, 7, 3)), "bgr", (4, 6), "image plane"),           # another size
    (Obj((5, 6, 3)), "rgb", (4, 6), "image plane"),
    (Obj((4, 6, 3), "<i2"), "bgr", (4, 6), "image plane"),    # another dtype
    ((Obj((4, 6, 3)),), "bgr", (4, 6), "one array"),
    ((Obj((4, 6)),), "nv12", (4, 6), "2 planes"),
    ((Obj((4, 6)), Obj((2, 3, 2)), Obj((2, 3))), "nv12", (4, 6), "2 planes"),
    ((Obj((4, 6)), Obj((2, 3, 2))), "i420", (4, 6), "3 planes"),
    (Obj((6, 8)), "i420", (4, 8), "tuple of planes"),
    ((Obj((4, 6)), Obj((2, 3))), "nv12", (4, 6), "UV plane"),
    ((Obj((5, 7)), Obj((2, 3, 2))), "nv12", (5, 7), "UV plane"),        # the floor sizes of an odd image
    ((Obj((4, 7)), Obj((2, 3, 2))), "nv12", (4, 6), "Y plane"),
    ((Obj((4, 6)), Obj((2, 3)), Obj((2, 4))), "i420", (4, 6), "V plane"),
    ((Obj((4, 6)), Obj((3, 3)), Obj((2, 3))), "i420", (4, 6), "U plane"),
    (Obj((9, 8)), "nv12", (4, 8), "Y plane"),                 # a single array of another height
    (Obj((6, 8), strides=(16, 1)), "nv12", (4, 8), "contiguous"),
    (Obj((7, 8)), "nv12", (4, 8), "H and W even"),
    (Obj((4, 6, 3), strides=(17, 3, 1)), "bgr", (4, 6), "row stride"),
    (Obj((4, 6, 3), stream=0), "bgr", (4, 6), "stream"),
    (object(), "bgr", (4, 6), "__cuda_array_interface__"),
])
def test_target_refusals(target, fmt, hw, match):
    with pytest.raises(S.StitchingError, match=match):
        target_planes(target, fmt, *hw)
    with pytest.raises(S.StitchingError, match=match):
        S.emit(image(*hw), fmt, out=target, ctx=object())


def test_arguments_are_checked_before_the_device_is_touched():
    """no images: nothing to do; every other call here would reach the C library (and fail on `object()` as a context) if the Python
    layer let it through"""
    assert S.emit_all([], ctx=object()) == []
    im = image(4, 6)
    with pytest.raises(S.StitchingError, match="formats for"):
        S.emit_all([im], format=["bgr", "bgr"], ctx=object())
    with pytest.raises(S.StitchingError, match="targets for"):
        S.emit_all([im], "bgr", out=[Obj((4, 6, 3)), Obj((4, 6, 3))], ctx=object())
    with pytest.raises(S.StitchingError, match="alpha images for"):
        S.emit_all([im], "bgra", alpha=[image(4, 6, 1), image(4, 6, 1)], ctx=object())
    with pytest.raises(S.StitchingError, match="matrix"):
        S.emit_all([im], "nv12", matrix="bt2020", ctx=object())
    with pytest.raises(S.StitchingError, match="matrix"):
        S.emit_all([im], "nv12", range="studio", ctx=object())
    with pytest.raises(S.StitchingError, match="stream"):
        S.emit_all([im], "bgr", stream=0, ctx=object())
    with pytest.raises(S.StitchingError, match="different streams"):
        S.emit_all([im, im], "bgr", out=[Obj((4, 6, 3), stream=5), Obj((4, 6, 3), ptr=PTR + 4096, stream=6)], ctx=object())
    with pytest.raises(S.StitchingError, match="different streams"):
        S.emit(im, "nv12", out=(Obj((4, 6), stream=5), Obj((2, 3, 2), ptr=PTR + 4096, stream=6)), ctx=object())
    # alpha: only with bgra / rgba, u8 x 1 of the source's size
    with pytest.raises(S.StitchingError, match="has no alpha"):
        S.emit(im, "bgr", alpha=image(4, 6, 1), ctx=object())
    with pytest.raises(S.StitchingError, match="has no alpha"):
        S.emit(im, "nv12", alpha=image(4, 6, 1), ctx=object())
    for bad in (image(4, 7, 1), image(5, 6, 1), image(4, 6, 3), image(4, 6, 1, _lib.F32)):
        with pytest.raises(S.StitchingError, match="alpha image is u8"):
            S.emit(im, "rgba", alpha=bad, ctx=object())


def test_the_binding_declares_the_item_structure():
    E = _lib.EmitItem
    assert [n for n, _ in E._fields_] == ["src", "alpha", "format", "has_target", "plane", "pitch"]
    assert C.sizeof(E) == 2 * 8 + 2 * 4 + 3 * 8 + 3 * 8  # two pointers, two ints, three pointers, three long longs
    assert "stx_emit" in _lib.EXPORTS
    assert S.emit is not None and S.emit_all is not None and "emit" in S.__all__ and "emit_all" in S.__all__
