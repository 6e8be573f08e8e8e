"""Constructed validity masks and cameras for the source-mask path of the warp (csrc/stx_warp.hip: the VALID instantiations of
warp_fast_kernel, and warp_kernel / warp_general_kernel with a mask beside the source).  Pure numpy, no GPU and no product code.

Two patterns per source size:
  hash    1 + (7 x + 13 y) % 251: grey, never 0 and never 255 inside, different in every neighbour and not symmetric in x and y — a sample
          taken one pixel off, with x and y swapped, through a wrong pitch, or replaced by 255 shows;
  binary  a 0 / 255 checkerboard of period 1 with a few zeroed blocks in the middle: the masks a rig really has are binary, and a
          nearest sample one pixel off flips every byte.

The rounding family (tests/constructed_warps.py: plane_case / Axis, one pixel per column and per row, everything inside the source):
  31/64, 33/64  v = k + 31/64 and k + 33/64: 32 v is a tie, s = cvRound(32 v) = 32 k + 16 in both, so (s + 16) >> 5 = k + 1 in both —
                but cvRound(v) is k for the first and k + 1 for the second.  The index is the coordinate's, not the pattern's.
  1/2           v = k + 1/2: the tie of the coordinate itself goes to the even pixel, k of both parities along the columns and rows.
"""
import numpy as np

from tests import constructed_warps as CW

_masks = {}


def hash_mask(sw, sh, x0=0):
    """the hash pattern of a sw x sh mask whose first column has position x0 (slices of a wider mask keep the wider one's positions)"""
    y, x = np.mgrid[0:sh, x0:x0 + sw]
    return (1 + (7 * x + 13 * y) % 251).astype(np.uint8)


def binary_mask(sw, sh):
    y, x = np.mgrid[0:sh, 0:sw]
    # pixel (0, 0) is 255: the ties k + 1/2 of both axes go to even pixels, whose sum is even — the other polarity would sample 0 in
    # every tie case and tell nothing apart there
    m = ((1 - ((x + y) & 1)) * 255).astype(np.uint8)
    # zeroed blocks in the middle: a third of the width from a quarter on, and a short one further right
    m[sh // 4:sh // 4 + max(sh // 3, 1), sw // 4:sw // 4 + max(sw // 3, 1)] = 0
    m[sh // 2:sh // 2 + max(sh // 5, 1), (2 * sw) // 3:(2 * sw) // 3 + max(sw // 7, 1)] = 0
    return m


PATTERNS = {"hash": hash_mask, "binary": binary_mask}


def mask(pattern, size):
    """the pattern's mask of a source size, made once (read only)"""
    key = (pattern, tuple(size))
    if key not in _masks:
        a = np.ascontiguousarray(PATTERNS[pattern](*size))
        a.setflags(write=False)
        _masks[key] = a
    return _masks[key]


WIDE_OFF = 3   # a mask that is a column-offset slice of a wider one: odd base address, pitch != width


def wide_mask(size):
    """(the wider mask, the offset): columns [WIDE_OFF, WIDE_OFF + sw) are the frame's mask; hash pattern over the wide positions"""
    sw, sh = size
    return hash_mask(sw + 2 * WIDE_OFF + 2, sh), WIDE_OFF


def family_rounding(family="mask_rounding"):
    out = []
    for axis in "xy":
        n, sz = CW._major((CW.SW, CW.SH), axis)
        for name, frac in (("31_64", 31 / 64), ("33_64", 33 / 64), ("tie_1_2", 1 / 2)):
            # along the lanes one pixel a column and one a row: k of both parities in every row; the other axis rests in pixel 1
            major = CW.Axis(1, 1, 3 + frac)
            ax, ay = CW._axes(axis, major, sz[1] if axis == "x" else sz[0])
            out.append(CW.plane_case(f"{family}-{axis}-{name}", family, sz, ax, ay, axis=axis, frac=frac))
    return out


ROUNDING = {c.name: c for c in family_rounding()}
ALL_CASES = {**CW.CASES, **ROUNDING}
