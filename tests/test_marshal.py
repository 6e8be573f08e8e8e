"""stitching_amd._marshal: what the estimators' Python fronts share.  No GPU, and but for one_context's default no library."""
import ctypes as C

import numpy as np
import pytest

from stitching_amd import _marshal as M
from stitching_amd.stitching_error import StitchingError


class _Handle:
    def __init__(self, h):
        self._h = h


class _UMat:
    def __init__(self, a):
        self.a = a

    def get(self):
        return self.a


@pytest.mark.parametrize("dtype, ctype", [(np.int32, C.c_int), (np.int64, C.c_longlong), (np.uint8, C.c_ubyte), (np.int8, C.c_byte),
                                          (np.float32, C.c_float), (np.float64, C.c_double)])
def test_ptr_is_typed_by_the_dtype_and_points_at_the_array(dtype, ctype):
    a = np.arange(6, dtype=dtype).reshape(2, 3)
    p = M.ptr(a)
    assert isinstance(p, C.POINTER(ctype))
    assert C.cast(p, C.c_void_p).value == a.ctypes.data
    assert [p[k] for k in range(6)] == a.reshape(-1).tolist()
    p[4] = 9  # no copy was made
    assert a[1, 1] == 9


@pytest.mark.parametrize("a", [np.zeros((4, 4), np.int32)[:, ::2], np.zeros((4, 4), np.float64).T, np.zeros(3, np.uint16),
                               np.zeros(3, np.float16), np.zeros(3, bool), [1, 2, 3], None])
def test_ptr_refuses_what_it_would_have_to_copy_or_cast(a):
    with pytest.raises(StitchingError, match="C-contiguous numpy array"):
        M.ptr(a)


def test_handles_keeps_none_and_addresses():
    h = M.handles([_Handle(C.c_void_p(0x1000)), None, _Handle(0x2000), 0x3000])
    assert isinstance(h, C.c_void_p * 4)
    assert list(h) == [0x1000, None, 0x2000, 0x3000]
    assert len(M.handles([])) == 0
    assert list(M.handles([None] * 3)) == [None, None, None]


def test_int_pairs_shapes():
    t = M.int_pairs([(1, 2), (3, 4), (-5, 6)], 3)
    assert t.shape == (3, 2) and t.dtype == np.int32 and t.flags.c_contiguous
    assert t.tolist() == [[1, 2], [3, 4], [-5, 6]]
    assert M.int_pairs(np.arange(8, dtype=np.int64)[::2].reshape(2, 2), 2).tolist() == [[0, 2], [4, 6]]
    assert M.int_pairs([], 0).shape == (0, 2)
    with pytest.raises(ValueError):
        M.int_pairs([(1, 2), (3, 4)], 3)


def test_one_context(monkeypatch):
    class FakeImage:
        def __init__(self, ctx):
            self.ctx = ctx

    default, a, b = object(), object(), object()
    monkeypatch.setattr(M, "DeviceImage", FakeImage)
    monkeypatch.setattr(M, "get_context", lambda: default)
    assert M.one_context([]) is default
    assert M.one_context([np.zeros((2, 2)), None]) is default
    assert M.one_context([np.zeros((2, 2)), FakeImage(a), None, FakeImage(a)]) is a
    with pytest.raises(StitchingError, match="^device images of more than one context$"):
        M.one_context([FakeImage(a), FakeImage(b)])


def test_image_spec_and_host_array():
    g = np.zeros((3, 5), np.uint8)
    a, wh, ch, dt = M.image_spec(g, "mask", 0)
    assert a is g and wh == (5, 3) and ch == 1 and dt == np.uint8
    c = np.zeros((3, 5, 4), np.float32)
    a, wh, ch, dt = M.image_spec(c, "image", 1)
    assert a is c and wh == (5, 3) and ch == 4 and dt == np.float32
    a, wh, ch, dt = M.image_spec(_UMat(g), "mask", 2)
    assert a is g and wh == (5, 3) and ch == 1
    assert M.host_array(_UMat(g)) is g and M.host_array(g) is g
    assert M.host_array([[1, 2]]).shape == (1, 2)
    with pytest.raises(StitchingError, match=r"^image 7: expected an HxW or HxWxC array, got shape \(4,\)$"):
        M.image_spec(np.zeros(4, np.uint8), "image", 7)
    with pytest.raises(StitchingError, match=r"^mask 0: expected an HxW or HxWxC array, got shape \(0,\)$"):
        M.image_spec([], "mask", 0)


def test_info_dict_casts():
    info = np.array([3.0, 2.0, 0.25, 1.0])
    d = M.info_dict(info, [("pairs", int), ("levels", int), ("device_ms", float), ("solver", lambda v: {1: "device"}[int(v)])])
    assert d == {"pairs": 3, "levels": 2, "device_ms": 0.25, "solver": "device"}
    assert list(d) == ["pairs", "levels", "device_ms", "solver"]
    assert type(d["pairs"]) is int and type(d["device_ms"]) is float
    assert M.info_dict(info, [("a", int)]) == {"a": 3}  # the names decide how much is read


def test_count_then_fill():
    calls = []

    def call(count, out):
        calls.append(out)
        C.cast(count, C.POINTER(C.c_longlong))[0] = 3
        if out is not None:
            out[:3] = [7, 8, 9]

    out, k = M.count_then_fill(call, C.c_longlong, lambda n: np.zeros(n, np.int64))
    assert k == 3 and out.tolist() == [7, 8, 9] and calls[0] is None and calls[1] is out
    # nothing to report: the outputs still hold one element, so that their pointers are valid
    out, k = M.count_then_fill(lambda count, out: None, C.c_int, lambda n: np.zeros(n, np.int32))
    assert k == 0 and out.shape == (1,)
