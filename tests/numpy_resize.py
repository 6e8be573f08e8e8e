"""cv::resize(INTER_LINEAR_EXACT) for 8-bit images and SeamFinder.resize, restated in plain Python / numpy: the contract the device
kernels (stitching_amd/csrc/stx_resize.hip, stx_resize_host.cpp) are compared with byte for byte, next to the CPU oracle.

Written apart from oracle/oracle.py on purpose: the coefficients are made one destination index at a time with Python floats (IEEE
double, one rounding per operation, never fused) and Python's round() (half to even), the pixels with integer numpy arrays.
tests/test_constructed_resizes.py shows that both agree on every constructed family (0 differing bytes).

  coeffs(src_n, dst_n)          interpolationLinear<ufixedpoint16>::getCoeffs: per destination index (offset, coeff1, interior)
  resize_with(src, cx, cy)      the 8.8 horizontal sums and the vertical blend for given coefficient rows
  resize_linear_exact(src, wh)  cv.resize(src, wh, interpolation=cv.INTER_LINEAR_EXACT)
  dilate3x3(mask)               cv.dilate(mask, None): pixels outside the image take no part
  seam_resize(low, final, sub)  SeamFinder.resize: dilate, enlarge, AND; sub = (full_w, full_h, x0, y0): `final` is that rectangle of a
                                final mask of full_w x full_h, and the result is that rectangle of the whole result
"""
import math

import numpy as np


def coeff(v, src_n, dst_n):
    """-> (offset, coeff1, interior) of destination index v.  scale = 1.0 / (dst / src); fval = scale * (v + 0.5) - 0.5 (two roundings);
    offset = floor(fval); coeff1 = the fraction * 256 rounded half to even.  Left of the first source sample: (0, 0, not interior);
    at or beyond the last, or with a one-sample source: (src_n - 1, 0, not interior)."""
    scale = 1.0 / (float(dst_n) / float(src_n))
    prod = scale * (float(v) + 0.5)
    fval = prod - 0.5
    ival = math.floor(fval)
    if ival >= 0 and src_n > 1:
        if ival < src_n - 1:
            return ival, int(round((fval - float(ival)) * 256.0)), True
        return src_n - 1, 0, False
    return 0, 0, False


def coeffs(src_n, dst_n, first=0, count=None, one=coeff):
    """-> ofs, c1, interior (arrays) for the destination indices first .. first + count - 1 of an axis enlarged from src_n to dst_n"""
    count = dst_n - first if count is None else count
    t = [one(v, src_n, dst_n) for v in range(first, first + count)]
    return (np.array([a[0] for a in t], np.int64), np.array([a[1] for a in t], np.int64), np.array([a[2] for a in t], bool))


def resize_with(src, cx, cy, clamp=True):
    """src (h, w) or (h, w, c) u8; cx / cy = (ofs, c1, interior) of the destination columns / rows.
    Horizontal: h = p[o] * (256 - c1) + p[min(o + 1, w - 1)] * c1 (8.8); vertical: interior rows (h0 * (256 - d1) + h1 * d1 + 2^15) >> 16,
    the others (h0 + 128) >> 8."""
    src = np.asarray(src, np.uint8)
    sh, sw = src.shape[:2]
    s = src.reshape(sh, sw, -1).astype(np.int64)
    (ox, c1, _), (oy, d1, iy) = cx, cy
    ox1 = np.minimum(ox + 1, sw - 1) if clamp else ox + 1
    oy1 = np.minimum(oy + 1, sh - 1) if clamp else oy + 1
    hs = s[:, ox, :] * (256 - c1)[None, :, None] + s[:, ox1, :] * c1[None, :, None]
    inner = (hs[oy] * (256 - d1)[:, None, None] + hs[oy1] * d1[:, None, None] + (1 << 15)) >> 16
    edge = (hs[oy] + 128) >> 8
    out = np.where(iy[:, None, None], inner, edge)
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8).reshape((len(oy), len(ox)) + src.shape[2:])


def resize_linear_exact(src, size):
    src = np.asarray(src, np.uint8)
    return resize_with(src, coeffs(src.shape[1], int(size[0])), coeffs(src.shape[0], int(size[1])))


def dilate3x3(mask):
    m = np.asarray(mask, np.uint8)
    h, w = m.shape
    out = np.zeros_like(m)
    for y in range(h):
        for x in range(w):
            out[y, x] = m[max(y - 1, 0):min(y + 2, h), max(x - 1, 0):min(x + 2, w)].max()
    return out


def seam_resize(low, final, sub=None):
    final = np.asarray(final, np.uint8)
    low = np.asarray(low, np.uint8)
    h, w = final.shape
    fw, fh, x0, y0 = (w, h, 0, 0) if sub is None else (int(v) for v in sub)
    assert 0 <= x0 and 0 <= y0 and x0 + w <= fw and y0 + h <= fh
    r = resize_with(dilate3x3(low), coeffs(low.shape[1], fw, x0, w), coeffs(low.shape[0], fh, y0, h))
    return r & final
