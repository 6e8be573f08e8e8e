"""Constructed rectangles, warped masks and images for exposure tracking (tests/numpy_exposure_track.py): the smallest inputs that reach
every path of csrc/stx_exposure_track.hip and its host side.  Shared by the contract's own test (CPU) and the kernel test (GPU)."""
import numpy as np

from tests import numpy_exposure_track as NT


def case(rects, stride, seed, masks=None, edit=None):
    """images: uniform in 1 .. 254 (nothing saturated) unless `edit` paints some; masks: all 255 unless given"""
    rng = np.random.default_rng(seed)
    imgs = [rng.integers(1, 255, (h, w, 3), dtype=np.uint8) for _, _, w, h in rects]
    mk = [np.full((h, w), 255, np.uint8) for _, _, w, h in rects]
    if masks is not None:
        masks(mk)
    if edit is not None:
        edit(imgs)
    return {"rects": [tuple(r) for r in rects], "stride": stride, "masks": mk, "imgs": imgs}


def expected(c, imgs=None):
    """-> (pairs (J, 2), self counts, stats (J, 8)) of the contract"""
    vs, origins, self_counts = NT.grids(c["rects"], c["masks"], c["stride"])
    stats = NT.pair_stats(c["rects"], vs, origins, c["imgs"] if imgs is None else imgs, c["stride"])
    return np.array(NT.pair_jobs(c["rects"]), np.int32).reshape(-1, 2), self_counts, stats


def _grey(mk):
    mk[0][4:12, 20:34] = 0      # inside the overlap with image 1
    mk[0][14:22, 24:40] = 128   # grey: does not count
    mk[1][0:6, 0:10] = 128
    mk[1][20:26, 8:20] = 0


def _saturate_first(imgs):
    imgs[0][6:14, 22:30] = 0
    imgs[0][16:20, 30:38, 1] = 255   # one channel alone


def _blank_third(mk):
    mk[2][:] = 0


CASES = {
    # name: (case, what it must reach)
    "single": lambda: case([(-3, 2, 20, 10)], 3, 1),
    "apart": lambda: case([(0, 0, 20, 10), (30, 0, 20, 10)], 2, 2),
    "thin_strip": lambda: case([(1, 1, 10, 20), (9, 1, 10, 20)], 8, 3),           # columns 9, 10: no multiple of 8
    "negative_s3": lambda: case([(-7, -5, 40, 30), (-4, -8, 35, 30)], 3, 4),
    "negative_s8": lambda: case([(-19, -13, 50, 40), (-9, -20, 45, 40)], 8, 5),
    "s1_tiles": lambda: case([(0, 0, 160, 40), (10, 0, 150, 40)], 1, 6),          # 150 x 40 lattice points: 5 x 2 tiles, ragged both ways
    "grey_mask": lambda: case([(0, 0, 48, 30), (16, 2, 48, 30)], 2, 7, masks=_grey),
    "saturated_first": lambda: case([(0, 0, 48, 30), (16, 2, 48, 30)], 2, 8, edit=_saturate_first),
    "three": lambda: case([(0, 0, 40, 30), (20, 5, 40, 30), (10, -10, 40, 30)], 2, 9),
    "empty_next_to_full": lambda: case([(0, 0, 40, 30), (20, 5, 40, 30), (10, -10, 40, 30)], 2, 10, masks=_blank_third),
}
