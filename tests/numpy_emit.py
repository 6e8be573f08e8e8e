"""The contract of device frame emit (stx_emit, stitching_amd.emit): plain numpy, integer only.  The device equals `from_bgr` byte
for byte (tests/test_gpu_emit.py).  It is the mirror of tests/numpy_ingest.py: the shapes `from_bgr` returns are the shapes `to_bgr`
takes.

Packed formats copy, reverse channels or add an alpha byte.  The 4:2:0 formats (nv12, i420) are made from u8 BGR in int32 with
16-bit fractions and an arithmetic shift:

    Y = clip8(((kyb*B + kyg*G + kyr*R + 32768) >> 16) + yoff)            per pixel; yoff = 16 (range "limited") or 0 ("full")
    U = clip8(((kub*SB + kug*SG + kur*SR + 131072) >> 18) + 128)         per 2 x 2 block, from the block's channel SUMS (0 .. 1020)
    V likewise

A block's coordinates are clamped to the image, so an odd last column or row is replicated (a 1 x 1 image's only block is four times
its pixel).  The chroma rounds once — there is no rounded average first — and is box-centred: the sample belongs to the middle of its
block, which is the siting ingest's chroma replication assumes.

The constants (`COEFFICIENTS`, in B, G, R order) follow one rule (`derive_coefficients`): with m the float64 forward matrix that
numpy_ingest.LUMA's luma weights give — Y = Kb B + Kg G + Kr R, U = (B - Y) / (2 (1 - Kb)), V = (R - Y) / (2 (1 - Kr)), scaled by
219/255 (Y) and 224/255 (U, V) for limited range — the B and R constants are rint(m * 65536), and G takes the remainder, so that a luma
row sums to 65536 (full) or 56284 = rint(65536 * 219 / 255) (limited) and a chroma row to 0: white stays white, grey has no colour.

How far this is from the matrix itself (`exact_yuv`: float64, no rounding, clipped to [0, 255]): the sum before the shift is
S = sum k_i x_i with 0 <= x_i <= 255 (a block's sums divided by 4 are averages in the same range), so
|S / 65536 - sum m_i x_i| <= sum |k_i / 65536 - m_i| * 255 =: delta (`coefficient_error`); (S + 32768) >> 16 is floor(S / 65536 + 1/2),
within 1/2 of S / 65536; adding the integer offset and clipping both sides to [0, 255] brings them no further apart.  So

    |from_bgr - exact_yuv| <= 1/2 + delta,       delta <= 0.0051 for every row of every variant   (`bound_exact`)

Every sum stays below 2^31: the largest constant is below 2^16 and a block sum is at most 1020.  Only full-range chroma ever clips:
B = 255, G = R = 0 gives U = 256 before the clip.
"""
import numpy as np

from tests import numpy_ingest

# ((kyb, kyg, kyr), (kub, kug, kur), (kvb, kvg, kvr)) by (matrix, range)
COEFFICIENTS = {
    ("bt601", "limited"): ((6416, 33039, 16829), (28784, -19070, -9714), (-4681, -24103, 28784)),
    ("bt601", "full"): ((7471, 38470, 19595), (32768, -21710, -11058), (-5329, -27439, 32768)),
    ("bt709", "limited"): ((4064, 40254, 11966), (28784, -22188, -6596), (-2639, -26145, 28784)),
    ("bt709", "full"): ((4732, 46871, 13933), (32768, -25259, -7509), (-3005, -29763, 32768)),
}
VARIANTS = tuple(COEFFICIENTS)
FORMATS = numpy_ingest.FORMATS
LUMA_ROW_SUM = {"limited": 56284, "full": 65536}


def real_matrix(matrix="bt709", range_="limited"):
    """The 3 x 3 forward matrix in float64, rows Y, U, V, columns B, G, R (not multiplied by 65536)."""
    kr, kb = numpy_ingest.LUMA[matrix]
    kg = 1.0 - kr - kb
    ys, cs = (219.0 / 255.0, 224.0 / 255.0) if range_ == "limited" else (1.0, 1.0)
    y = np.array([kb, kg, kr])
    u = (np.array([1.0, 0.0, 0.0]) - y) / (2.0 * (1.0 - kb))
    v = (np.array([0.0, 0.0, 1.0]) - y) / (2.0 * (1.0 - kr))
    return np.stack([y * ys, u * cs, v * cs])


def derive_coefficients(matrix="bt709", range_="limited"):
    """The rule of the docstring: rint(m * 65536) for B and R, the remainder of the row's sum on G."""
    m = real_matrix(matrix, range_)
    rows = []
    for row, total in zip(m, (LUMA_ROW_SUM[range_], 0, 0)):
        b, r = int(np.rint(row[0] * 65536.0)), int(np.rint(row[2] * 65536.0))
        rows.append((b, total - b - r, r))
    return tuple(rows)


def coefficients(matrix="bt709", range_="limited"):
    if (matrix, range_) not in COEFFICIENTS:
        raise ValueError(f"unknown matrix / range {matrix!r} / {range_!r}")
    return COEFFICIENTS[(matrix, range_)]


def coefficient_error(matrix="bt709", range_="limited"):
    """delta of the docstring for the rows (Y, U, V), in 8-bit levels."""
    k = np.array(coefficients(matrix, range_), np.float64)
    return tuple(float(v) for v in (np.abs(k / 65536.0 - real_matrix(matrix, range_)).sum(axis=1) * 255.0))


def bound_exact(matrix="bt709", range_="limited"):
    """Largest |from_bgr - exact_yuv| the derivation allows for (Y, U, V), in 8-bit levels (real valued)."""
    return tuple(0.5 + d for d in coefficient_error(matrix, range_))


def _i32(a):
    return np.asarray(a).astype(np.int32)


def luma(b, g, r, matrix="bt709", range_="limited"):
    """Y of broadcastable B, G, R arrays (any integer dtype holding 0 .. 255) -> uint8"""
    (kb, kg, kr), _, _ = coefficients(matrix, range_)
    yoff = 16 if range_ == "limited" else 0
    return np.clip(((kb * _i32(b) + kg * _i32(g) + kr * _i32(r) + 32768) >> 16) + yoff, 0, 255).astype(np.uint8)


def chroma(sb, sg, sr, matrix="bt709", range_="limited"):
    """(U, V) of broadcastable 2 x 2 block sums SB, SG, SR (0 .. 1020) -> two uint8 arrays"""
    _, ku, kv = coefficients(matrix, range_)
    sb, sg, sr = _i32(sb), _i32(sg), _i32(sr)
    return tuple(np.clip(((k[0] * sb + k[1] * sg + k[2] * sr + 131072) >> 18) + 128, 0, 255).astype(np.uint8) for k in (ku, kv))


def exact_yuv(b, g, r, matrix="bt709", range_="limited"):
    """The real matrix in float64 on real-valued B, G, R (a block's averages for the chroma), clipped to [0, 255] and not rounded:
    array [..., 3] of Y, U, V — what `luma` and `chroma` approximate."""
    m = real_matrix(matrix, range_)
    x = np.stack(np.broadcast_arrays(np.asarray(b, np.float64), np.asarray(g, np.float64), np.asarray(r, np.float64)), axis=-1)
    off = np.array([16.0 if range_ == "limited" else 0.0, 128.0, 128.0])
    return np.clip(x @ m.T + off, 0.0, 255.0)


def block_sums(img):
    """u8 H x W x 3 -> int32 ceil(H/2) x ceil(W/2) x 3: the channel sums of every 2 x 2 block, coordinates clamped to the image."""
    h, w = img.shape[:2]
    a = img.astype(np.int32)
    y0, x0 = np.arange(0, h, 2), np.arange(0, w, 2)
    y1, x1 = np.minimum(y0 + 1, h - 1), np.minimum(x0 + 1, w - 1)
    return a[y0][:, x0] + a[y0][:, x1] + a[y1][:, x0] + a[y1][:, x1]


def _image(a, c, what):
    a = np.asarray(a)
    if a.dtype != np.uint8 or a.ndim != (2 if c == 1 else 3) or (c > 1 and a.shape[2] != c):
        raise ValueError(f"{what}: expected uint8 with {c} channel(s), got {a.dtype} of shape {a.shape}")
    return a


def from_bgr(img, fmt=None, matrix="bt709", range_="limited", alpha=None):
    """What emit makes of an image: one array, or the tuple of plane arrays of nv12 (Y, UV) / i420 (Y, U, V)."""
    if fmt not in FORMATS:
        raise ValueError(f"unknown format {fmt!r}")
    a = np.asarray(img)
    if alpha is not None and fmt not in ("bgra", "rgba"):
        raise ValueError(f"format {fmt!r} has no alpha")
    if fmt is None:
        if a.dtype not in (np.uint8, np.int16, np.float32) or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] > 4):
            raise ValueError(f"no image layout: {a.dtype} of shape {a.shape}")
        return a.copy()
    if fmt == "gray":
        return _image(a, 1, "gray").copy()
    a = _image(a, 3, fmt)
    if fmt == "bgr":
        return a.copy()
    if fmt == "rgb":
        return np.ascontiguousarray(a[..., ::-1])
    if fmt in ("bgra", "rgba"):
        out = np.empty(a.shape[:2] + (4,), np.uint8)
        out[..., :3] = a if fmt == "bgra" else a[..., ::-1]
        if alpha is None:
            out[..., 3] = 255
        else:
            m = _image(alpha, 1, "alpha")
            if m.shape != a.shape[:2]:
                raise ValueError(f"alpha of shape {m.shape} for an image of {a.shape[:2]}")
            out[..., 3] = m
        return out
    y = luma(a[..., 0], a[..., 1], a[..., 2], matrix, range_)
    s = block_sums(a)
    u, v = chroma(s[..., 0], s[..., 1], s[..., 2], matrix, range_)
    y, u, v = (np.ascontiguousarray(p) for p in (y, u, v))
    return (y, np.ascontiguousarray(np.stack([u, v], axis=-1))) if fmt == "nv12" else (y, u, v)
