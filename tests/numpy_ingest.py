"""The contract of device frame ingest (stx_ingest, stitching_amd.ingest): plain numpy, integer only.  The device equals `to_bgr`
byte for byte (tests/test_gpu_ingest.py).

Packed formats copy, reverse or drop channels.  The 4:2:0 formats (nv12, i420) become BGR with replicated chroma — pixel (x, y) takes
the chroma sample (x >> 1, y >> 1), odd sizes have chroma planes of the ceiling sizes — by the usual 8-bit-fraction roundings of the
BT.601 / BT.709 matrices, all in int32 with an arithmetic shift:

    C = Y - 16 (range "limited") or Y ("full"),  D = U - 128,  E = V - 128
    R = clip8((yk*C          + rv*E + 128) >> 8)
    G = clip8((yk*C - gu*D   - gv*E + 128) >> 8)
    B = clip8((yk*C + bu*D          + 128) >> 8)

How far this is from the matrices themselves (`exact_bgr`: float64, no rounding, clipped to [0, 255]) follows from the constants:
with k_i the integer coefficients, m_i the real ones and x_i the terms they multiply, the sum before the shift is S = sum k_i x_i, so
|S / 256 - sum m_i x_i| <= sum |k_i / 256 - m_i| max|x_i| =: delta (max|C| = 239 limited / 255 full, max|D| = max|E| = 128);
(S + 128) >> 8 is floor(S / 256 + 1/2), within 1/2 of S / 256; and clipping both sides to [0, 255] brings them no further apart.  So

    |to_bgr - exact_bgr| <= 1/2 + delta          (`bound_exact`, real valued)
    |to_bgr - round(exact_bgr)| <= floor(1 + delta)   (`bound_levels`: both sides are integers, rounding adds at most another 1/2)

`coefficient_error` computes delta per channel from the float64 matrices; tests/test_ingest_contract.py checks both bounds over all
2^24 (Y, U, V) triples of each variant.  Derived values (delta of the worst channel; bound_exact; bound_levels):

    bt601 limited   0.2853 (R)   0.7853   1
    bt709 limited   0.4933 (G)   0.9933   1
    bt601 full      0.1840 (B)   0.6840   1
    bt709 full      0.1026 (G)   0.6026   1

so the integer formula is within ONE 8-bit level of the rounded float64 conversion, for every triple of every variant.
"""
import numpy as np

# (yk, rv, gu, gv, bu) by (matrix, range)
COEFFICIENTS = {
    ("bt601", "limited"): (298, 409, 100, 208, 516),
    ("bt709", "limited"): (298, 459, 55, 136, 541),
    ("bt601", "full"): (256, 359, 88, 183, 454),
    ("bt709", "full"): (256, 403, 48, 120, 475),
}
VARIANTS = tuple(COEFFICIENTS)
# luma weights (Kr, Kb) of the two standards
LUMA = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
FORMATS = (None, "bgr", "rgb", "bgra", "rgba", "gray", "nv12", "i420")


def coefficients(matrix="bt709", range_="limited"):
    """(yoff, yk, rv, gu, gv, bu): the integer constants of one variant."""
    if (matrix, range_) not in COEFFICIENTS:
        raise ValueError(f"unknown matrix / range {matrix!r} / {range_!r}")
    return ((16 if range_ == "limited" else 0),) + COEFFICIENTS[(matrix, range_)]


def real_coefficients(matrix="bt709", range_="limited"):
    """The same five constants as real numbers (not multiplied by 256), from the standard's luma weights in float64."""
    kr, kb = LUMA[matrix]
    kg = 1.0 - kr - kb
    ys, cs = (255.0 / 219.0, 255.0 / 224.0) if range_ == "limited" else (1.0, 1.0)
    return (ys, 2.0 * (1.0 - kr) * cs, 2.0 * kb * (1.0 - kb) / kg * cs, 2.0 * kr * (1.0 - kr) / kg * cs, 2.0 * (1.0 - kb) * cs)


def coefficient_error(matrix="bt709", range_="limited"):
    """delta of the docstring for (R, G, B): how far the integer coefficients can carry the sum from the real matrix, in levels."""
    yoff, yk, rv, gu, gv, bu = coefficients(matrix, range_)
    ys, mrv, mgu, mgv, mbu = real_coefficients(matrix, range_)
    cmax = float(max(255 - yoff, yoff))
    ey = abs(yk / 256.0 - ys) * cmax
    return (ey + abs(rv / 256.0 - mrv) * 128.0,
            ey + abs(gu / 256.0 - mgu) * 128.0 + abs(gv / 256.0 - mgv) * 128.0,
            ey + abs(bu / 256.0 - mbu) * 128.0)


def bound_exact(matrix="bt709", range_="limited"):
    """Largest |to_bgr - exact_bgr| the derivation allows, in 8-bit levels (real valued)."""
    return 0.5 + max(coefficient_error(matrix, range_))


def bound_levels(matrix="bt709", range_="limited"):
    """Largest |to_bgr - round(exact_bgr)| the derivation allows, in whole 8-bit levels."""
    return int(np.floor(1.0 + max(coefficient_error(matrix, range_))))


def yuv_to_bgr(y, u, v, matrix="bt709", range_="limited"):
    """Integer conversion of broadcastable Y, U, V arrays (any integer dtype holding 0 .. 255) -> uint8 array [..., 3] in B, G, R order."""
    yoff, yk, rv, gu, gv, bu = coefficients(matrix, range_)
    c = yk * (np.asarray(y).astype(np.int32) - yoff)
    d = np.asarray(u).astype(np.int32) - 128
    e = np.asarray(v).astype(np.int32) - 128
    r = (c + rv * e + 128) >> 8
    g = (c - gu * d - gv * e + 128) >> 8
    b = (c + bu * d + 128) >> 8
    return np.clip(np.stack(np.broadcast_arrays(b, g, r), axis=-1), 0, 255).astype(np.uint8)


def exact_bgr(y, u, v, matrix="bt709", range_="limited"):
    """The real matrices in float64, clipped to [0, 255] and not rounded: what `yuv_to_bgr` approximates."""
    yoff = 16 if range_ == "limited" else 0
    ys, mrv, mgu, mgv, mbu = real_coefficients(matrix, range_)
    c = ys * (np.asarray(y).astype(np.float64) - yoff)
    d = np.asarray(u).astype(np.float64) - 128.0
    e = np.asarray(v).astype(np.float64) - 128.0
    return np.clip(np.stack(np.broadcast_arrays(c + mbu * d, c - mgu * d - mgv * e, c + mrv * e), axis=-1), 0.0, 255.0)


def chroma_shape(h, w):
    return ((h + 1) // 2, (w + 1) // 2)


def _plane(a, shape, what):
    a = np.asarray(a)
    if a.dtype != np.uint8 or a.shape != shape:
        raise ValueError(f"{what}: expected uint8 of shape {shape}, got {a.dtype} of shape {a.shape}")
    return a


def to_bgr(planes, fmt=None, matrix="bt709", range_="limited"):
    """What ingest makes of a frame.  `planes`: one array, or the tuple of plane arrays of nv12 (Y, UV) / i420 (Y, U, V)."""
    if fmt not in FORMATS:
        raise ValueError(f"unknown format {fmt!r}")
    if fmt in ("nv12", "i420"):
        y = np.asarray(planes[0])
        if y.ndim != 2:
            raise ValueError("the Y plane is H x W")
        h, w = y.shape
        ch, cw = chroma_shape(h, w)
        y = _plane(y, (h, w), "Y")
        if fmt == "nv12":
            if len(planes) != 2:
                raise ValueError("nv12 takes (Y, UV)")
            uv = _plane(planes[1], (ch, cw, 2), "UV")
            u, v = uv[..., 0], uv[..., 1]
        else:
            if len(planes) != 3:
                raise ValueError("i420 takes (Y, U, V)")
            u, v = _plane(planes[1], (ch, cw), "U"), _plane(planes[2], (ch, cw), "V")
        yy, xx = np.arange(h)[:, None] >> 1, np.arange(w)[None, :] >> 1
        return yuv_to_bgr(y, u[yy, xx], v[yy, xx], matrix, range_)
    a = np.asarray(planes)
    if fmt is None:
        if a.dtype not in (np.uint8, np.int16, np.float32) or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] > 4):
            raise ValueError(f"no image layout: {a.dtype} of shape {a.shape}")
        return a.copy()
    if fmt == "gray":
        return _plane(a, a.shape[:2], "gray").copy()
    c = 3 if fmt in ("bgr", "rgb") else 4
    a = _plane(a, a.shape[:2] + (c,), fmt)
    return np.ascontiguousarray(a[..., 2::-1] if fmt in ("rgb", "rgba") else a[..., :3])
