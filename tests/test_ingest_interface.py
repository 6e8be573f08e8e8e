"""The host side of device frame ingest that needs no device: `parse_cuda_array_interface` on constructed dicts, the split of a single
nv12 array, plane counts and plane shapes of every format."""
import pytest

import stitching_amd as S
from stitching_amd import _lib
from stitching_amd.ingest import frame_planes, parse_cuda_array_interface, split_nv12

PTR = 0x7F0000001000


class Obj:
    """the least a foreign device array is: an object with the dict"""

    def __init__(self, shape, typestr="|u1", strides=None, ptr=PTR, **more):
        self.__cuda_array_interface__ = iface(shape, typestr, strides, ptr, **more)


def iface(shape, typestr="|u1", strides=None, ptr=PTR, version=3, **more):
    d = {"shape": tuple(shape), "typestr": typestr, "data": (ptr, False), "version": version, "strides": strides}
    d.update(more)
    return d


# ---- accepted ---------------------------------------------------------------------------------------------------------------------
def test_packed_shapes_and_dtypes():
    assert parse_cuda_array_interface(iface((4, 6))) == (PTR, 4, 6, 1, _lib.U8, 6, None)
    assert parse_cuda_array_interface(iface((4, 6, 3))) == (PTR, 4, 6, 3, _lib.U8, 18, None)
    assert parse_cuda_array_interface(iface((4, 6, 4), "<i2")) == (PTR, 4, 6, 4, _lib.S16, 48, None)
    assert parse_cuda_array_interface(iface((4, 6, 2), "<f4")) == (PTR, 4, 6, 2, _lib.F32, 48, None)
    assert parse_cuda_array_interface(iface((1, 1, 1))) == (PTR, 1, 1, 1, _lib.U8, 1, None)


def test_object_or_dict_and_versions():
    assert parse_cuda_array_interface(Obj((4, 6, 3))) == parse_cuda_array_interface(iface((4, 6, 3)))
    assert parse_cuda_array_interface(iface((4, 6), version=2))[1:3] == (4, 6)
    d = iface((4, 6))
    del d["strides"]  # absent is None
    assert parse_cuda_array_interface(d)[5] == 6
    assert parse_cuda_array_interface(iface((4, 6), data=(PTR, True)))[0] == PTR  # a read-only source is a source


def test_row_stride_may_be_padded():
    assert parse_cuda_array_interface(iface((4, 6, 3), strides=(18, 3, 1)))[5] == 18
    assert parse_cuda_array_interface(iface((4, 6, 3), strides=(256, 3, 1)))[5] == 256
    assert parse_cuda_array_interface(iface((4, 6), strides=(11, 1)))[5] == 11
    assert parse_cuda_array_interface(iface((4, 6, 2), "<f4", strides=(52, 8, 4)))[5] == 52


def test_stream_entry_as_the_protocol_defines_it():
    assert parse_cuda_array_interface(iface((4, 6)))[6] is None
    assert parse_cuda_array_interface(iface((4, 6), stream=None))[6] is None
    assert parse_cuda_array_interface(iface((4, 6), stream=1))[6] == 1  # the legacy default stream
    assert parse_cuda_array_interface(iface((4, 6), stream=2))[6] == 2  # the per-thread default stream
    assert parse_cuda_array_interface(iface((4, 6), stream=0x55AA00))[6] == 0x55AA00
    with pytest.raises(S.StitchingError, match="stream"):
        parse_cuda_array_interface(iface((4, 6), stream=0))


# ---- refused, each with a message that says which ------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,match", [
    (iface((4, 6), mask=Obj((4, 6))), "mask"),
    (iface((0, 6)), "zero-sized"),
    (iface((4, 0, 3)), "zero-sized"),
    (iface((4, 6, 3), strides=(0, 3, 1)), "zero or negative"),
    (iface((4, 6, 3), strides=(-18, 3, 1)), "zero or negative"),
    (iface((4, 6), strides=(6, -1)), "zero or negative"),
    (iface((4, 6, 3), strides=(17, 3, 1)), "row stride"),
    (iface((4, 6, 3), strides=(36, 6, 1)), "packed"),      # every second pixel
    (iface((4, 6, 3), strides=(72, 12, 4)), "packed"),     # a channel slice of something wider
    (iface((6, 4), strides=(1, 6)), "packed"),             # a transposed view
    (iface((4, 6, 3), strides=(18, 3)), "strides"),
    (iface((4, 6), "<f8"), "unsupported dtype"),
    (iface((4, 6), "<u2"), "unsupported dtype"),
    (iface((4, 6), "|i1"), "unsupported dtype"),
    (iface((4, 6), "<c8"), "unsupported dtype"),
    (iface((4, 6), ">i2"), "big-endian"),
    (iface((4, 6), ">f4"), "big-endian"),
    (iface((4, 6, 5)), "at most 4"),
    (iface((6,)), "HxW"),
    (iface((2, 4, 6, 3)), "HxW"),
    (iface((4, 6), version=1), "version"),
    (iface((4, 6), version=None), "version"),
    (iface((4, 6), data=(0, False)), "data"),
    (iface((4, 6), data=None), "data"),
    (iface((4, 6), typestr=None), "typestr"),
])
def test_refusals(d, match):
    with pytest.raises(S.StitchingError, match=match):
        parse_cuda_array_interface(d)


def test_not_an_interface_at_all():
    with pytest.raises(S.StitchingError, match="__cuda_array_interface__"):
        parse_cuda_array_interface(object())
    with pytest.raises(S.StitchingError, match="__cuda_array_interface__"):
        parse_cuda_array_interface([[1, 2], [3, 4]])


# ---- the single nv12 array ----------------------------------------------------------------------------------------------------------
def test_split_of_a_single_nv12_array():
    y, uv = split_nv12(parse_cuda_array_interface(iface((6, 8), stream=7)))
    assert y == (PTR, 4, 8, 1, _lib.U8, 8, 7)
    assert uv == (PTR + 4 * 8, 2, 4, 2, _lib.U8, 8, 7)
    assert frame_planes(Obj((6, 8)), "nv12") == [y[:6] + (None,), uv[:6] + (None,)]
    y, uv = frame_planes(Obj((3, 2)), "nv12")  # the smallest: 2 x 2
    assert (y[1:4], uv[0] - y[0], uv[1:4]) == ((2, 2, 1), 4, (1, 1, 2))


@pytest.mark.parametrize("obj,match", [
    (Obj((7, 8)), "H and W even"),                    # rows no multiple of 3
    (Obj((6, 7)), "H and W even"),                    # odd width
    (Obj((6, 8), strides=(16, 1)), "contiguous"),     # a padded surface has two planes
    (Obj((6, 8, 1), "<i2"), "u8"),
    (Obj((6, 8, 3)), "u8"),
])
def test_single_nv12_array_refusals(obj, match):
    with pytest.raises(S.StitchingError, match=match):
        frame_planes(obj, "nv12")


def test_rows_of_an_odd_height_cannot_come_as_one_array():
    """H = 2 only: 9 rows are 6 + 3, never an odd H (the UV plane of an odd height has ceil(H / 2) rows: pass (Y, UV))"""
    y, uv = frame_planes(Obj((9, 8)), "nv12")
    assert y[1] == 6 and uv[1] == 3


# ---- plane counts and plane shapes --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(1, 1), (2, 2), (3, 5), (6, 8), (7, 259)])
def test_planar_frames_take_the_ceiling_sizes(h, w):
    ch, cw = (h + 1) // 2, (w + 1) // 2
    planes = frame_planes((Obj((h, w), strides=(w + 3, 1)), Obj((ch, cw, 2), strides=(2 * cw + 2, 2, 1), ptr=PTR + 4096)), "nv12")
    assert [p[1:6] for p in planes] == [(h, w, 1, _lib.U8, w + 3), (ch, cw, 2, _lib.U8, 2 * cw + 2)]
    planes = frame_planes((Obj((h, w)), Obj((ch, cw), ptr=PTR + 4096), Obj((ch, cw), ptr=PTR + 8192)), "i420")
    assert [p[:4] for p in planes] == [(PTR, h, w, 1), (PTR + 4096, ch, cw, 1), (PTR + 8192, ch, cw, 1)]


@pytest.mark.parametrize("frame,fmt,match", [
    ((Obj((4, 6)),), "nv12", "2 planes"),
    ((Obj((4, 6)), Obj((2, 3, 2)), Obj((2, 3))), "nv12", "2 planes"),
    ((Obj((4, 6)), Obj((2, 3, 2))), "i420", "3 planes"),
    (Obj((6, 8)), "i420", "tuple of planes"),
    ((Obj((4, 6)), Obj((2, 3))), "nv12", "UV plane"),          # interleaved pairs are H/2 x W/2 x 2
    ((Obj((4, 6)), Obj((2, 6))), "nv12", "UV plane"),
    ((Obj((5, 7)), Obj((2, 3, 2))), "nv12", "UV plane"),        # the floor sizes of an odd frame
    ((Obj((5, 7)), Obj((3, 4, 2), "<i2")), "nv12", "UV plane"),
    ((Obj((4, 6)), Obj((2, 3)), Obj((2, 4))), "i420", "V plane"),
    ((Obj((4, 6)), Obj((3, 3)), Obj((2, 3))), "i420", "U plane"),
    ((Obj((4, 6)), Obj((2, 3, 2)), Obj((2, 3))), "i420", "U plane"),
    ((Obj((4, 6, 3)), Obj((2, 3, 2))), "nv12", "Y plane"),
    ((Obj((4, 6), "<f4"), Obj((2, 3)), Obj((2, 3))), "i420", "Y plane"),
    ((Obj((4, 6, 3)), Obj((4, 6, 3))), "bgr", "one array"),
    ((Obj((4, 6, 3)),), None, "one array"),
    (Obj((4, 6, 4)), "bgr", "3 channel"),
    (Obj((4, 6)), "rgb", "3 channel"),
    (Obj((4, 6, 3)), "bgra", "4 channel"),
    (Obj((4, 6, 3)), "rgba", "4 channel"),
    (Obj((4, 6, 3)), "gray", "1 channel"),
    (Obj((4, 6, 3), "<i2"), "bgr", "u8"),
    (Obj((4, 6), "<f4"), "gray", "u8"),
    (Obj((4, 6, 3)), "yuyv", "unknown pixel format"),
])
def test_plane_count_and_shape_errors(frame, fmt, match):
    with pytest.raises(S.StitchingError, match=match):
        frame_planes(frame, fmt)


def test_format_none_takes_every_image_layout():
    for shape, typestr in (((4, 6), "|u1"), ((4, 6, 2), "|u1"), ((4, 6, 3), "<i2"), ((4, 6, 4), "<f4"), ((4, 6, 1), "<f4")):
        (p,) = frame_planes(Obj(shape, typestr), None)
        assert p[1:3] == (4, 6) and p[3] == (shape[2] if len(shape) == 3 else 1)
    for fmt, c in (("bgr", 3), ("rgb", 3), ("bgra", 4), ("rgba", 4)):
        assert frame_planes(Obj((4, 6, c)), fmt)[0][3] == c
    assert frame_planes(Obj((4, 6)), "gray")[0][3] == 1


def test_arguments_are_checked_before_the_device_is_touched():
    """no frames: nothing to do; bad formats / matrices fail in Python (no context is made on a machine without a GPU: the first
    two calls would raise there)"""
    assert S.ingest_all([], ctx=object()) == []
    with pytest.raises(S.StitchingError, match="formats for"):
        S.ingest_all([Obj((4, 6, 3))], format=["bgr", "bgr"], ctx=object())
    with pytest.raises(S.StitchingError, match="matrix"):
        S.ingest_all([Obj((4, 6, 3))], matrix="bt2020", ctx=object())
    with pytest.raises(S.StitchingError, match="stream"):
        S.ingest_all([Obj((4, 6, 3))], stream=0, ctx=object())
    with pytest.raises(S.StitchingError, match="different streams"):
        S.ingest_all([Obj((4, 6, 3), stream=5), Obj((4, 6, 3), stream=6)], ctx=object())


def test_the_binding_declares_the_frame_structure():
    import ctypes as C

    F = _lib.ForeignFrame
    assert [n for n, _ in F._fields_] == ["plane", "pitch", "w", "h", "channels", "elem", "format"]
    assert C.sizeof(F) == 3 * 8 + 3 * 8 + 5 * 4 + 4  # three pointers, three long longs, five ints, padded to 8
    assert _lib.INGEST_FORMATS == {None: 0, "bgr": 1, "rgb": 2, "bgra": 3, "rgba": 4, "gray": 5, "nv12": 6, "i420": 7}
    assert "stx_ingest" in _lib.EXPORTS
