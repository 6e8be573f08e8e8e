"""Device frame ingest: frames that were born on the device become `DeviceImage`s without a trip through the host.

A frame is any object that speaks `__cuda_array_interface__` (another framework's device array, a wrapper round a decoder's
surface) in the pixel formats video arrives in; `ingest_all` converts a whole list with ONE launch (`stx_ingest`).  Ingest always
copies or converts into a buffer of the library's own and never adopts the foreign pointer: the kernels rely on readable bytes in
front of every image the library allocates, which foreign memory does not promise.  tests/numpy_ingest.py is
the contract, byte for byte.

No framework is imported here or anywhere in the package: this is duck typing and ctypes.
"""
import ctypes as C

from . import _lib
from .stitching_error import StitchingError

_TYPESTR = {"|u1": (_lib.U8, 1), "<i2": (_lib.S16, 2), "<f4": (_lib.F32, 4)}
_PLANES = {"nv12": ("Y", "UV"), "i420": ("Y", "U", "V")}
_PACKED_CHANNELS = {"bgr": 3, "rgb": 3, "bgra": 4, "rgba": 4, "gray": 1}


def parse_cuda_array_interface(obj_or_dict):
    """`__cuda_array_interface__` (the object or its dict) -> (ptr, h, w, c, elem, pitch_bytes, stream).

    Accepted: version >= 2; typestr |u1, <i2, <f4; a 2-D (H, W) or 3-D (H, W, C <= 4) shape; strides None (packed) or a tuple whose
    element and channel strides are the packed ones, with any row stride >= the row bytes.  `stream` comes back as the protocol
    defines it: None (absent or None: no ordering needed), 1 (the legacy default stream), 2 (the per-thread default stream) or a
    stream handle; 0 is invalid.  Everything else is refused with a StitchingError that says what."""
    d = obj_or_dict if isinstance(obj_or_dict, dict) else getattr(obj_or_dict, "__cuda_array_interface__", None)
    if not isinstance(d, dict):
        raise StitchingError(f"{type(obj_or_dict).__name__} has no __cuda_array_interface__")
    version = d.get("version")
    if not isinstance(version, int) or version < 2:
        raise StitchingError(f"__cuda_array_interface__ version {version!r}: version 2 or later is needed")
    if d.get("mask") is not None:
        raise StitchingError("__cuda_array_interface__ with a mask entry is not taken")
    typestr = d.get("typestr")
    if not isinstance(typestr, str) or len(typestr) < 3:
        raise StitchingError(f"__cuda_array_interface__ typestr {typestr!r}")
    if typestr[0] == ">":
        raise StitchingError(f"big-endian data ({typestr}) is not taken")
    if typestr not in _TYPESTR:
        raise StitchingError(f"unsupported dtype {typestr}: images are |u1, <i2 or <f4")
    elem, size = _TYPESTR[typestr]
    shape = d.get("shape")
    if not isinstance(shape, (tuple, list)) or len(shape) not in (2, 3) or not all(isinstance(s, int) for s in shape):
        raise StitchingError(f"expected an HxW or HxWxC device array, got shape {shape!r}")
    h, w = int(shape[0]), int(shape[1])
    c = int(shape[2]) if len(shape) == 3 else 1
    if h <= 0 or w <= 0 or c <= 0:
        raise StitchingError(f"zero-sized device array of shape {tuple(shape)}")
    if c > 4:
        raise StitchingError(f"{c} channels: images have at most 4")
    row = w * c * size
    strides = d.get("strides")
    if strides is None:
        pitch = row
    else:
        if not isinstance(strides, (tuple, list)) or len(strides) != len(shape) or not all(isinstance(s, int) for s in strides):
            raise StitchingError(f"strides {strides!r} do not fit shape {tuple(shape)}")
        if any(s <= 0 for s in strides):
            raise StitchingError(f"zero or negative strides {tuple(strides)} are not taken")
        packed = (c * size, size) if len(shape) == 3 else (size,)
        if tuple(strides[1:]) != packed:
            raise StitchingError(f"strides {tuple(strides)}: pixels and channels must be packed ({packed}), only rows may be padded")
        pitch = int(strides[0])
        if pitch < row:
            raise StitchingError(f"row stride {pitch} is below the {row} bytes of a row")
    data = d.get("data")
    if not isinstance(data, (tuple, list)) or len(data) != 2 or not isinstance(data[0], int) or data[0] == 0:
        raise StitchingError(f"__cuda_array_interface__ data {data!r}: (device pointer, read_only) is needed")
    stream = d.get("stream")
    if stream is not None:
        if not isinstance(stream, int) or isinstance(stream, bool) or stream == 0:
            raise StitchingError(f"__cuda_array_interface__ stream {stream!r} is invalid (0 is disallowed by the protocol)")
    return int(data[0]), h, w, c, elem, pitch, stream


def split_nv12(parsed):
    """One contiguous (H * 3 / 2) x W u8 array (H, W even) -> its parsed planes [Y: H x W, UV: H/2 x W/2 x 2]."""
    ptr, rows, w, c, elem, pitch, stream = parsed
    if c != 1 or elem != _lib.U8:
        raise StitchingError("a single nv12 array is (H * 3 / 2) x W of u8")
    if pitch != w:
        raise StitchingError("a single nv12 array must be contiguous: pass (Y, UV) for padded surfaces")
    if rows % 3 or w % 2:
        raise StitchingError(f"a single nv12 array of {rows} x {w} is no (H * 3 / 2) x W with H and W even: pass (Y, UV)")
    h = rows // 3 * 2
    return [(ptr, h, w, 1, elem, pitch, stream), (ptr + h * pitch, h // 2, w // 2, 2, elem, pitch, stream)]


def frame_planes(frame, format=None):
    """A frame of `format` -> the list of its parsed planes, shapes checked (pure Python: no device is touched)."""
    if format not in _lib.INGEST_FORMATS:
        raise StitchingError(f"unknown pixel format {format!r}: one of {[f for f in _lib.INGEST_FORMATS]}")
    if format in _PLANES:
        names = _PLANES[format]
        if isinstance(frame, (tuple, list)):
            if len(frame) != len(names):
                raise StitchingError(f"{format} takes {len(names)} planes {names}, got {len(frame)}")
            planes = [parse_cuda_array_interface(p) for p in frame]
        elif format == "nv12":
            planes = split_nv12(parse_cuda_array_interface(frame))
        else:
            raise StitchingError("i420 takes the tuple of planes (Y, U, V)")
        _, h, w, c, elem, _, _ = planes[0]
        if c != 1 or elem != _lib.U8:
            raise StitchingError(f"{format}: the Y plane is H x W of u8")
        ch, cw = (h + 1) // 2, (w + 1) // 2
        for name, p in zip(names[1:], planes[1:]):
            want = (ch, cw, 2) if name == "UV" else (ch, cw, 1)
            if p[4] != _lib.U8 or (p[1], p[2], p[3]) != want:
                shape = want[:2] + ((2,) if name == "UV" else ())
                raise StitchingError(f"{format}: the {name} plane of a {h} x {w} frame is u8 of shape {shape}, got {p[1:4]}")
        return planes
    if isinstance(frame, (tuple, list)):
        raise StitchingError(f"format {format!r} takes one array, not a tuple of planes")
    p = parse_cuda_array_interface(frame)
    if format is not None and (p[4] != _lib.U8 or p[3] != _PACKED_CHANNELS[format]):
        raise StitchingError(f"format {format!r} takes u8 with {_PACKED_CHANNELS[format]} channel(s), got {p[3]} channel(s) of element type {p[4]}")
    return [p]


def _stream_of(planes, stream):
    """The stream to order after: `stream=` overrides the objects' own entries; None: no ordering."""
    if stream is not None:
        if not isinstance(stream, int) or isinstance(stream, bool) or stream == 0:
            raise StitchingError(f"stream {stream!r} is invalid: 1 (legacy default), 2 (per-thread default) or a stream handle")
        return {stream}
    return {p[6] for p in planes if p[6] is not None}


def ingest_all(frames, format=None, matrix="bt709", range="limited", stream=None, wait=True, ctx=None):
    """A list of foreign device frames -> a list of DeviceImages, by one launch.

    frames: objects with `__cuda_array_interface__`; for the planar formats tuples of plane objects — (Y, UV) for "nv12", (Y, U, V)
        for "i420" — or, for nv12 with even H and W, one contiguous (H * 3 / 2) x W u8 array.  Sizes may differ.
    format: None (any image layout of the library, copied as it is), "bgr", "rgb", "bgra", "rgba", "gray", "nv12", "i420" — one for the
        list, or a list with one per frame.  Everything but None and "gray" becomes u8 BGR.
    matrix / range: "bt601" | "bt709", "limited" | "full" for the YUV formats.
    stream: the producer's stream (1: legacy default, 2: per-thread default, else a handle); overrides the objects' own `stream` entry.
        The conversion is ordered after it on the device, without a host wait.  With neither, the caller vouches that the frames are
        complete.
    wait=True syncs the context before returning: the sources may be recycled at once (a decoder's surface pool).  wait=False only
        queues the work, as from_numpy(wait=False) does: the sources stay untouched until ctx.sync()."""
    from .device import DeviceImage, get_context  # (device imports this module for as_device)

    ctx = ctx or get_context()
    frames = list(frames)
    if not frames:
        return []
    formats = list(format) if isinstance(format, (list, tuple)) else [format] * len(frames)
    if len(formats) != len(frames):
        raise StitchingError(f"{len(formats)} formats for {len(frames)} frames")
    if matrix not in _lib.INGEST_MATRICES or range not in _lib.INGEST_RANGES:
        raise StitchingError(f"matrix {matrix!r} / range {range!r}: bt601 | bt709, limited | full")
    table = (_lib.ForeignFrame * len(frames))()
    streams = set()
    for F, frame, fmt in zip(table, frames, formats):
        planes = frame_planes(frame, fmt)
        for k, p in enumerate(planes):
            F.plane[k], F.pitch[k] = p[0], p[5]
        _, F.h, F.w, F.channels, F.elem, _, _ = planes[0]
        F.format = _lib.INGEST_FORMATS[fmt]
        streams |= _stream_of(planes, stream)
    outs = (C.c_void_p * len(frames))()
    streams = sorted(streams)
    if len(streams) > 1:  # one launch is ordered after one stream
        raise StitchingError(f"the frames name {len(streams)} different streams: pass stream= or ingest them per producer")
    _lib.check(ctx._lib.stx_ingest(ctx.handle, len(frames), table, _lib.INGEST_MATRICES[matrix], _lib.INGEST_RANGES[range],
                            C.c_void_p(streams[0]) if streams else None, 1 if streams else 0, outs))
    imgs = [DeviceImage(ctx, C.c_void_p(h)) for h in outs]
    if wait:
        ctx.sync()
    return imgs


def ingest(frame, format=None, matrix="bt709", range="limited", stream=None, wait=True, ctx=None):
    """One foreign device frame -> DeviceImage (see ingest_all)."""
    return ingest_all([frame], format=format, matrix=matrix, range=range, stream=stream, wait=wait, ctx=ctx)[0]
