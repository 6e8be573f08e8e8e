"""What the device estimators' Python fronts share: reading what a caller hands in (numpy arrays, cv.UMat-likes, DeviceImages, device
arrays of other frameworks), choosing the context, and the ctypes spelling of arrays, handle lists, results and info.  Private."""
import ctypes as C

import numpy as np

from .device import DeviceImage, as_device, get_context, is_foreign_device_array
from .stitching_error import StitchingError

# keyed by the dtype itself: looking up `dtype.name` costs more than the rest of ptr() together
_POINTERS = {np.dtype(name): C.POINTER(ctype) for name, ctype in (("int32", C.c_int), ("int64", C.c_longlong), ("uint8", C.c_ubyte),
                                                                 ("int8", C.c_byte), ("float32", C.c_float), ("float64", C.c_double))}


def host_array(a):
    """numpy array of a numpy array, a cv.UMat-like (`.get()`) or anything np.asarray takes"""
    if not isinstance(a, np.ndarray) and hasattr(a, "get"):
        a = a.get()
    return np.asarray(a)


def image_spec(a, what, i):
    """-> (numpy array or DeviceImage, (w, h), channels, dtype) without a host copy of a device image; a foreign device array becomes a
    DeviceImage on the device."""
    if is_foreign_device_array(a):
        a = as_device(a)
    if isinstance(a, DeviceImage):
        return a, (a.width, a.height), a.channels, a.dtype
    a = host_array(a)
    if a.ndim not in (2, 3):
        raise StitchingError(f"{what} {i}: expected an HxW or HxWxC array, got shape {a.shape}")
    return a, (a.shape[1], a.shape[0]), (1 if a.ndim == 2 else a.shape[2]), a.dtype


def one_context(arrays):
    """The context of the DeviceImages among `arrays` (the default context without any); more than one is refused."""
    ctxs = {id(a.ctx): a.ctx for a in arrays if isinstance(a, DeviceImage)}
    if len(ctxs) > 1:
        raise StitchingError("device images of more than one context")
    return next(iter(ctxs.values())) if ctxs else get_context()


def handles(bufs):
    """void*[n] of the images' handles; an entry that has none (None: a null pointer; the address of a host array) goes in as it is"""
    return (C.c_void_p * len(bufs))(*[getattr(b, "_h", b) for b in bufs])


def ptr(a):
    """The typed ctypes pointer of a C-contiguous numpy array; nothing is copied or cast, so anything else is refused."""
    pointer = _POINTERS.get(a.dtype) if isinstance(a, np.ndarray) and a.flags.c_contiguous else None
    if pointer is None:
        raise StitchingError(f"internal: ptr() takes a C-contiguous numpy array of {', '.join(map(str, _POINTERS))}")
    return a.ctypes.data_as(pointer)


def int_pairs(values, n):
    """(n, 2) C-contiguous int32 table of corners or sizes"""
    return np.ascontiguousarray(np.asarray(values, np.int32).reshape(n, 2))


def adopt(ctx, outs, resident):
    """Output handles -> DeviceImages, or their host copies when the caller's data is not resident"""
    res = [DeviceImage(ctx, C.c_void_p(h)) for h in outs]
    return res if resident else [r.numpy() for r in res]


def info_dict(values, names_and_casts):
    """{name: cast(values[k])} for the k-th (name, cast)"""
    return {name: cast(v) for (name, cast), v in zip(names_and_casts, values)}


def count_then_fill(call, ctype, make):
    """The C ABI's two-call protocol: call(count, None) leaves the number of results in `count` (a `ctype` by reference), make(k)
    allocates the outputs for max(1, count) of them and call(count, outputs) fills them.  -> (outputs, count)"""
    count = ctype(0)
    call(C.byref(count), None)
    out = make(max(1, count.value))
    call(C.byref(count), out)
    return out, count.value
