"""Device frame emit: panoramas (any `DeviceImage`) leave for an encoder or a compositor without a trip through the host.

The mirror of `stitching_amd.ingest`: `emit_all` converts a list of images into the pixel formats video leaves in — NV12 / I420 for a
hardware encoder, BGRA / RGBA with the panorama mask as alpha for a compositor, RGB, or plain copies — with ONE launch (`stx_emit`),
either into planes of the library's own or in place into the caller's surfaces: any object that speaks `__cuda_array_interface__`,
with its own base and pitch.  Emit writes only the rows of the target planes, never their padding.
tests/numpy_emit.py is the contract, byte for byte.

No framework is imported here or anywhere in the package: this is duck typing and ctypes.
"""
import ctypes as C

from . import _lib
from .ingest import _PACKED_CHANNELS, _PLANES, _stream_of, parse_cuda_array_interface, split_nv12
from .stitching_error import StitchingError


def plane_shapes(format, h, w, c=3, elem=_lib.U8):
    """What `format` makes of an h x w image of c channels of `elem` -> the list of its planes' (h, w, c, elem).  The source's layout
    is checked against the format here (pure Python: no device is touched)."""
    if format not in _lib.INGEST_FORMATS:
        raise StitchingError(f"unknown pixel format {format!r}: one of {[f for f in _lib.INGEST_FORMATS]}")
    if format is None:
        return [(h, w, c, elem)]
    want = 1 if format == "gray" else 3
    if c != want or elem != _lib.U8:
        raise StitchingError(f"format {format!r} is made from u8 with {want} channel(s), the image has {c} channel(s) of element type {elem}")
    if format in _PLANES:
        ch, cw = (h + 1) // 2, (w + 1) // 2
        chroma = [(ch, cw, 2, _lib.U8)] if format == "nv12" else [(ch, cw, 1, _lib.U8)] * 2
        return [(h, w, 1, _lib.U8)] + chroma
    return [(h, w, _PACKED_CHANNELS[format], _lib.U8)]


def _writable(obj):
    """A target plane -> its parsed interface; read-only memory is refused."""
    p = parse_cuda_array_interface(obj)
    d = obj if isinstance(obj, dict) else obj.__cuda_array_interface__
    if d["data"][1]:
        raise StitchingError("the target is read-only (__cuda_array_interface__ data[1] is true): emit writes in place")
    return p


def target_planes(target, format, h, w, c=3, elem=_lib.U8):
    """The caller's target for an h x w image emitted as `format` -> the list of its parsed planes, count, shapes and dtypes checked
    against what the format makes of the image (pure Python: no device is touched).  target: one object with
    `__cuda_array_interface__`; for nv12 / i420 the tuple of plane objects, or, for nv12 with even sizes, one contiguous
    (H * 3 / 2) x W u8 array."""
    shapes = plane_shapes(format, h, w, c, elem)
    if format in _PLANES:
        names = _PLANES[format]
        if isinstance(target, (tuple, list)):
            if len(target) != len(names):
                raise StitchingError(f"{format} is written to {len(names)} planes {names}, got {len(target)}")
            planes = [_writable(p) for p in target]
        elif format == "nv12":
            planes = split_nv12(_writable(target))
        else:
            raise StitchingError("i420 is written to the tuple of planes (Y, U, V)")
    else:
        if isinstance(target, (tuple, list)):
            raise StitchingError(f"format {format!r} is written to one array, not a tuple of planes")
        names, planes = ("image",), [_writable(target)]
    for name, p, want in zip(names, planes, shapes):
        if (p[1], p[2], p[3], p[4]) != want:
            raise StitchingError(f"{format}: the {name} plane of a {h} x {w} image is {want[0]} x {want[1]} with {want[2]} channel(s) of element "
                                 f"type {want[3]}, the target has {p[1]} x {p[2]} with {p[3]} channel(s) of element type {p[4]}")
    return planes


def _per_item(value, n, what):
    """one value for the list, or a list with one per image"""
    values = list(value) if isinstance(value, list) else [value] * n
    if len(values) != n:
        raise StitchingError(f"{len(values)} {what} for {n} images")
    return values


def emit_all(images, format=None, out=None, alpha=None, matrix="bt709", range="limited", stream=None, wait=True, ctx=None):
    """A list of images -> their pixels in `format`, by one launch.

    images: DeviceImages, crop views included (anything else goes through as_device).  Sizes may differ.
    format: None (any image layout of the library, copied as it is), "bgr", "rgb", "bgra", "rgba", "gray", "nv12", "i420" — one for the
        list, or a list with one per image.  Everything but None and "gray" is made from u8 BGR.
    out: None — the planes are allocated and returned as DeviceImages: one image for the packed formats, (Y, UV) for "nv12", (Y, U, V)
        for "i420".  Or a list with one target per image (None entries are allocated): an object with `__cuda_array_interface__`, the
        tuple of plane objects of nv12 / i420, or, for nv12 with even sizes, one contiguous (H * 3 / 2) x W u8 array.  Targets are
        written in place — only the rows of their planes, whatever their base and pitch — and the same objects are returned.
    alpha: for "bgra" / "rgba" a u8 image of the source's size whose bytes become the alpha channel (the panorama mask); None: 255.
        One for the list (a list of one image), or a list with one (or None) per image.
    matrix / range: "bt601" | "bt709", "limited" | "full" for the YUV formats.
    stream: the consumer's stream (1: legacy default, 2: per-thread default, else a handle); overrides the targets' own `stream`
        entry.  The launch is ordered after what is queued there (the encoder may still be reading the surface) and the stream after
        the launch, on the device, without a host wait.  With neither, the caller vouches that the targets are free.
    wait=True syncs the context before returning: the targets are complete.  wait=False only queues the work."""
    from .device import DeviceImage, as_device, get_context

    ctx = ctx or get_context()
    images = list(images)
    n = len(images)
    if not n:
        return []
    formats = list(format) if isinstance(format, (list, tuple)) else [format] * n
    if len(formats) != n:
        raise StitchingError(f"{len(formats)} formats for {n} images")
    if matrix not in _lib.INGEST_MATRICES or range not in _lib.INGEST_RANGES:
        raise StitchingError(f"matrix {matrix!r} / range {range!r}: bt601 | bt709, limited | full")
    outs, alphas = _per_item(out, n, "targets"), _per_item(alpha, n, "alpha images")
    images = [im if isinstance(im, DeviceImage) else as_device(im, ctx) for im in images]
    alphas = [a if a is None or isinstance(a, DeviceImage) else as_device(a, ctx) for a in alphas]
    table = (_lib.EmitItem * n)()
    streams = set(_stream_of([], stream))
    for i, (E, im, fmt, target, a) in enumerate(zip(table, images, formats, outs, alphas)):
        h, w = im.height, im.width
        if target is None:
            plane_shapes(fmt, h, w, im.channels, im._elem)
        else:
            planes = target_planes(target, fmt, h, w, im.channels, im._elem)
            for k, p in enumerate(planes):
                E.plane[k], E.pitch[k] = p[0], p[5]
            E.has_target = 1
            streams |= _stream_of(planes, stream)
        if a is not None:
            if fmt not in ("bgra", "rgba"):
                raise StitchingError(f"image {i}: format {fmt!r} has no alpha")
            if (a.height, a.width, a.channels, a._elem) != (h, w, 1, _lib.U8):
                raise StitchingError(f"image {i}: the alpha image is u8 of {h} x {w}, got {a.dtype} of shape {a.shape}")
            E.alpha = a._h.value
        E.src, E.format = im._h.value, _lib.INGEST_FORMATS[fmt]
    streams = sorted(streams)
    if len(streams) > 1:  # one launch is ordered against one stream
        raise StitchingError(f"the targets name {len(streams)} different streams: pass stream= or emit them per consumer")
    made = (C.c_void_p * (3 * n))()
    _lib.check(ctx._lib.stx_emit(ctx.handle, n, table, _lib.INGEST_MATRICES[matrix], _lib.INGEST_RANGES[range],
                                 C.c_void_p(streams[0]) if streams else None, 1 if streams else 0, made))
    results = []
    for i, target in enumerate(outs):
        if target is None:
            planes = tuple(DeviceImage(ctx, C.c_void_p(h)) for h in made[3 * i:3 * i + 3] if h)
            results.append(planes if formats[i] in _PLANES else planes[0])
        else:
            results.append(target)
    if wait:
        ctx.sync()
    return results


def emit(image, format=None, out=None, alpha=None, matrix="bt709", range="limited", stream=None, wait=True, ctx=None):
    """One image -> its pixels in `format`, in planes of the library's own or in place in `out` (see emit_all)."""
    return emit_all([image], format=format, out=None if out is None else [out], alpha=None if alpha is None else [alpha], matrix=matrix,
                    range=range, stream=stream, wait=wait, ctx=ctx)[0]
