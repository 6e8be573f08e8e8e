"""Constructed inputs for the multi-band blender (csrc/stx_blend_fast.hip: the batched level-0 pyrDown, the packed gathers
mb_level0_pk_kernel / mb_level0_deferred_kernel / mb_level_pk_kernel and their epilogues; csrc/stx_blend.hip: the generic kernels): every
family is built to reach paths of those kernels that warped rings and seeded noise do not name, and returns the facts that make it
reach them.  Pure numpy, no GPU and no product code.  tests/test_constructed_multiband.py asserts the facts, shows that both CPU
references agree on every scene and that each family tells the contract from a one-mistake variant of it;
tests/test_gpu_constructed_multiband.py runs the same scenes on the device.

Every builder returns a Scene: the requested band count, the feeds (u8 or int16 image, mask, corner) in feed order, the roi and `facts`,
a dict of what the construction promises, stated from the construction alone (never from a reference's output).

classify(scene) restates the tests the kernels make on their data — on the geometry the host derives and on the intermediate values of the
independent numpy reference (tests/numpy_blenders.NumpyMultiBand: G and W pyramids, accumulated sums, finished levels) — and returns how
many lanes (8 x 2 patches), wavefronts (512 x 2 tiles) and pyrDown runs take each branch, and the launches the host will pick."""
import collections
import math

import numpy as np

from tests import numpy_blenders as NB

# Constants of the kernels and of the host code the families are shaped around.  tests/test_constructed_multiband.py reads each of them
# back from the sources: a moved constant fails that test instead of letting a family quietly miss its edge.
TILE_W, TILE_H = 512, 2   # a wavefront of the gathers: 64 lanes x STRIP_W columns, LV_TH rows
STRIP_W, STRIP_H = 8, 2   # a lane's patch
LANES = 64
DN_TOW, DN_TOH = 64, 14   # output tile of the batched pyrDown kernels
DN_ROWS = 2 * DN_TOH + 3  # bordered rows a tile reads
RUN = 11                  # level-0 pixels per pyrDown task (4 outputs)
RUN_GROUP = 16            # tasks per bordered row of a tile: a wavefront holds 4 rows of them
TAP_LIMIT = 500           # up_patch_pks_math: packed collapse while every tap is within +-500
COUNT_SIGN, COUNT_SHIFT, COUNT_RCP = 1, 2, 16  # level0_epilogue_pk: counts <= 1: a - sign(a); <= 2: shift; < 16: one reciprocal; else division
COVER_IMAGES = 64         # one cover word (replay) and one ballot of the image search
PACKED_IMAGES = 255       # fast_level_ok: more images take the generic kernels (byte counters)
DEFER_SEGS = 256          # STX_DEFER_SEGS: tile column tx queues into segment tx % DEFER_SEGS
OCC_CELL = 64             # columns of a level per occupancy entry (and 2 rows)
FAST_LEVELS_BELOW = 3     # fast_level_ok: num_bands - level >= 3; the three coarsest levels are one launch (mb_coarse_kernel)
MAX_BANDS = 16            # STX_MAX_BANDS
MULTIBAND = 2             # STX_BLEND_MULTIBAND (the oracle's handle uses the same number)
GREYS = (1, 127, 128, 254)


def border(bands):
    """MultiBandBlender::feed's gap (stx_blend_host.cpp: mb_feed_rect): 3 * 2^bands columns and rows around the image"""
    return 3 << bands


def effective_bands(req, w, h):
    """stx_blend_create / MultiBandBlender::prepare: bands cropped to ceil(log2(longer side))"""
    return min(int(req), int(math.ceil(math.log(max(w, h)) / math.log(2.0))), MAX_BANDS)


def padded_roi(roi, bands):
    x, y, w, h = roi
    al = 1 << bands
    return x, y, w + (al - w % al) % al, h + (al - h % al) % al


def feed_rect(bands, proi, iw, ih, tl):
    """mb_feed_rect restated -> (fx, fy, fw, fh) relative to the padded roi and (left, top) of the image inside it"""
    rx, ry, rw, rh = proi
    gap, al = border(bands), 1 << bands
    tlx, tly = max(rx, tl[0] - gap), max(ry, tl[1] - gap)
    brx, bry = min(rx + rw, tl[0] + iw + gap), min(ry + rh, tl[1] + ih + gap)
    tlx = rx + (((tlx - rx) >> bands) << bands)
    tly = ry + (((tly - ry) >> bands) << bands)
    w, h = brx - tlx, bry - tly
    w += (al - w % al) % al
    h += (al - h % al) % al
    tlx -= max(tlx + w - (rx + rw), 0)
    tly -= max(tly + h - (ry + rh), 0)
    return (tlx - rx, tly - ry, w, h), (tl[0] - tlx, tl[1] - tly)


def level_regions(bands, x0, x1, rw):
    """mb_level_regions: the columns of every level that the panorama columns [x0, x1) depend on"""
    xb, xe = [x0], [x1]
    for i in range(1, bands + 1):
        al = 7 if i <= bands - FAST_LEVELS_BELOW else 1
        xb.append(max(0, (xb[-1] >> 1) - 1) & ~al)
        xe.append(min(rw >> i, ((((xe[-1] - 1) >> 1) + 2) + al) & ~al))
    return xb, xe


class Scene:
    """pitched: {feed index: (image fill, mask fill, x offset)} — feeds the device test uploads as views into larger buffers ("random":
    seeded bytes).  A mask is declared binary to the kernels when its whole uploaded buffer holds only 0 and 255 (stx_buf_from_host scans
    it; a view inherits its buffer's verdict): `binary` says so per feed"""

    def __init__(self, bands, feeds, facts, pitched=None):
        self.bands, self.feeds, self.facts, self.pitched = int(bands), list(feeds), facts, dict(pitched or {})
        x0 = min(c[0] for _, _, c in self.feeds)
        y0 = min(c[1] for _, _, c in self.feeds)
        x1 = max(c[0] + m.shape[1] for _, m, c in self.feeds)
        y1 = max(c[1] + m.shape[0] for _, m, c in self.feeds)
        self.roi = (x0, y0, x1 - x0, y1 - y0)
        self.B = effective_bands(self.bands, self.roi[2], self.roi[3])
        self.proi = padded_roi(self.roi, self.B)

    @property
    def binary(self):
        out = []
        for k, (_, m, _) in enumerate(self.feeds):
            p = self.pitched.get(k)
            out.append(bool(np.isin(m, (0, 255)).all()) and (p is None or p[1] in (0, 255)))
        return out

    @property
    def s16(self):
        return [np.asarray(i).dtype == np.int16 for i, _, _ in self.feeds]


def _noise(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3)).astype(np.uint8)


def _full(h, w):
    return np.full((h, w), 255, np.uint8)


# ---------------------------------------------------------------------------------------------------------------------------------
# classify
# ---------------------------------------------------------------------------------------------------------------------------------
def numpy_reference(scene):
    """the scene through NumpyMultiBand with its intermediates kept -> (blender, int16 panorama, mask)"""
    b = NB.NumpyMultiBand(scene.bands, keep=True)
    b.prepare(scene.roi)
    for img, mask, corner in scene.feeds:
        b.feed(np.asarray(img).astype(np.int16), mask, corner)
    out, m = b.blend()
    return b, out, m


def host_flags(scene):
    """what mb_finish and stx_fast_mb_down_batch derive from the descriptors"""
    n = len(scene.feeds)
    all_u8 = not any(scene.s16)
    pk_ok = all_u8 and all(scene.binary)
    return {"n": n, "all_u8": all_u8, "pk_ok": pk_ok, "fuse": scene.B >= FAST_LEVELS_BELOW, "fast": n <= PACKED_IMAGES}


def expected_launches(scene, adopted=False):
    """-> (kernels, prof): the instantiation the host picks per pyramid pass and per level (stx_launch_mb_pyramids, mb_finish,
    stx_fast_mb_level), and the profiler's scope names with their call counts.  adopted: a blender that took a kept rig's weights"""
    f, B = host_flags(scene), scene.B
    replay = adopted and f["n"] <= COVER_IMAGES
    kernels, prof = [], collections.Counter()
    for lv in range(B):
        if lv == 0:
            kernels.append("mb_down0_lds_kernel<%s, %s>" % ("true" if f["pk_ok"] else "false", "false" if adopted else "true"))
            kernels += ["mb_down0_kernel<true>"] * sum(scene.s16)
        else:
            kernels.append("mb_down_lds_kernel<%s>" % ("false" if adopted else "true"))
        prof["mb_down0" if lv == 0 else "mb_down"] += 1
    top = B - 2 if f["fuse"] else B
    for lv in range(top, -1, -1):
        if f["fuse"] and lv == B - 2:
            kernels.append("mb_coarse_kernel")
            prof["mb_coarse"] += 1
            continue
        prof["mb_level0" if lv == 0 else "mb_level"] += 1
        fast = B - lv >= FAST_LEVELS_BELOW and f["fast"] and (lv > 0 or f["all_u8"])
        if not fast:
            kernels.append("mb_level_kernel<%s>" % ("true" if lv == 0 else "false"))
        elif lv == 0 and f["pk_ok"]:
            kernels.append("mb_level0_pk_kernel<false, false, %s>" % ("true" if replay else "false"))
        elif lv == 0:
            kernels += ["mb_level0_pk_kernel<false, true, %s>" % ("true" if replay else "false"), "mb_level0_deferred_kernel"]
            prof["mb_level0_deferred"] += 1
        elif f["all_u8"]:
            kernels.append("mb_level_pk_kernel<%s>" % ("true" if replay else "false"))
        else:
            kernels.append("mb_level_fast_kernel<false, false, false, false>")
    replayed = sum(1 for k in kernels if replay and k.endswith("true>") and ("pk_kernel" in k))
    return kernels, dict(prof), replayed


def expected_sharded(scene, owners, messages, exchange):
    """The launches of a sharded blend (stitching_amd.distributed: one blender per rank, ShardPlan's `messages` = (image, source rank,
    destination rank, rectangle, bytes)) -> (kernels per rank, {scope: calls} summed over the ranks' blenders).  A rank's image table
    holds its own images, and per message to it a received image strip (exchange "strips": an image like any other, u8) or a received
    contribution (kind 1: has_contrib); per message from it (exchange "contribs") one batched export, a launch per emit class
    (stx_fast_mb_emit_class: level 0 of a u8 image, levels 1 .. B - 3 of a u8 image, of an int16 image; everything else generic)"""
    B, world = scene.B, max(owners) + 1
    prof, per_rank = collections.Counter(), []
    for g in range(world):
        own = [k for k in range(len(scene.feeds)) if owners[k] == g]
        got = [m[0] for m in messages if m[2] == g]
        kind0 = own + (got if exchange == "strips" else [])
        contribs = got if exchange == "contribs" else []
        all_u8 = not any(scene.s16[k] for k in kind0)
        has_contrib = bool(contribs)
        pk_ok = all_u8 and all(scene.binary[k] for k in kind0) and all(scene.binary[k] and not scene.s16[k] for k in contribs)
        kernels = []
        if kind0:
            for lv in range(B):
                if lv == 0:
                    kernels.append("mb_down0_lds_kernel<%s, true>" % ("true" if all_u8 and all(scene.binary[k] for k in kind0) else "false"))
                    kernels += ["mb_down0_kernel<true>"] * sum(scene.s16[k] for k in kind0)
                else:
                    kernels.append("mb_down_lds_kernel<true>")
                prof["mb_down0" if lv == 0 else "mb_down"] += 1
        for m in messages:
            if exchange != "contribs" or m[1] != g:
                continue
            u8 = not scene.s16[m[0]]
            classes = ["mb_emit_multi_kernel<true, false>" if u8 else "mb_level_kernel<true> (emit)"]
            if B - FAST_LEVELS_BELOW >= 1:
                classes.append("mb_emit_multi_kernel<false, true>" if u8 else "mb_emit_multi_kernel<false, false>")
            if B >= 1:
                classes.append("mb_level_kernel<false> (emit)")
            kernels += classes
            prof["mb_contrib"] += 1
        fuse = B >= FAST_LEVELS_BELOW
        for lv in range(B - 2 if fuse else B, -1, -1):
            if fuse and lv == B - 2:
                kernels.append("mb_coarse_kernel")
                prof["mb_coarse"] += 1
                continue
            prof["mb_level0" if lv == 0 else "mb_level"] += 1
            fast = B - lv >= FAST_LEVELS_BELOW and len(kind0) + len(contribs) <= PACKED_IMAGES and (lv > 0 or all_u8)
            if not fast:
                kernels.append("mb_level_kernel<%s>" % ("true" if lv == 0 else "false"))
            elif lv == 0 and pk_ok:
                kernels.append("mb_level0_pk_kernel<%s>" % ("true" if has_contrib else "false, false, false"))
            elif lv == 0 and not has_contrib:
                kernels += ["mb_level0_pk_kernel<false, true, false>", "mb_level0_deferred_kernel"]
                prof["mb_level0_deferred"] += 1
            elif lv == 0:
                kernels.append("mb_level_fast_kernel<true, true, false, false>")
            elif has_contrib:
                kernels.append("mb_level_fast_kernel<false, true, false, %s>" % ("true" if all_u8 else "false"))
            elif all_u8:
                kernels.append("mb_level_pk_kernel<false>")
            else:
                kernels.append("mb_level_fast_kernel<false, false, false, false>")
        per_rank.append(kernels)
    return per_rank, dict(prof)


def _lanes(a, reduce):
    """(H, W[, C]) -> per 8 x 2 patch (H / 2, W / 8[, C])"""
    h, w = a.shape[:2]
    return reduce(reduce(a.reshape((h // 2, 2, w // 8, 8) + a.shape[2:]), axis=3), axis=1)


def _occ(w):
    """the occupancy map the pyrDown kernels write for a weight level: one entry per 64 columns and row pair"""
    h, ww = w.shape
    p = np.pad(w != 0, ((0, -h % 2), (0, -ww % OCC_CELL)))
    return p.reshape(p.shape[0] // 2, 2, p.shape[1] // OCC_CELL, OCC_CELL).any(axis=(1, 3))


def _search_hit(fd, lv, tile_x, Y0, has_occ):
    """mb_tile_hit: rectangle test, then occ_hit_f (level 0 reads the level-1 map)"""
    fx, fy, fw, fh = fd["rect"]
    if lv == 0:
        ix, iy, iw, ih = fd["image"]
        if not (ix < tile_x + 512 and ix + iw > tile_x and iy < Y0 + 2 and iy + ih > Y0):
            return False
        sl, fr, x0, x1 = 1, (Y0 - fy) >> 1, (tile_x - fx) >> 1, (tile_x + 511 - fx) >> 1
    else:
        rx, ry, rw, rh = fx >> lv, fy >> lv, fw >> lv, fh >> lv
        if not (rx < tile_x + 512 and rx + rw > tile_x and ry < Y0 + 2 and ry + rh > Y0):
            return False
        sl, fr, x0 = lv, Y0 - ry, tile_x - rx
        x1 = x0 + 511
    if not has_occ:
        return True
    lw, lh = fw >> sl, fh >> sl
    x0, x1 = max(x0, 0), min(x1, lw - 1)
    if fr < 0 or fr >= lh or x0 > x1:
        return True
    if "occ" not in fd:
        fd["occ"] = {}
    if sl not in fd["occ"]:
        fd["occ"][sl] = _occ(fd["w"][sl])
    return bool(fd["occ"][sl][fr >> 1, x0 >> 6:(x1 >> 6) + 1].any())


def _collapse(finer_shape, coarse, x1, y1):
    """up_patch_pks_math's test per lane and plane of a level whose finished coarser level is `coarse`: the 18 taps (three rows by the
    row rule, six columns with the two border substitutions) -> (packed lanes per plane, 32-bit lanes per plane, per-lane extreme tap
    (H/2, W/8, 3) of the active lanes as a masked array, smallest and largest tap)"""
    ph, pw = finer_shape
    ch, cw = ph >> 1, pw >> 1
    Y0, X0 = np.arange(0, ph, 2), np.arange(0, pw, 8)
    cy, cx = Y0 >> 1, X0 >> 1
    rows = np.stack([np.minimum(np.abs(cy - 1), ch - 1), cy, np.minimum(cy + 1, ch - 1)], 1)   # (ny, 3)
    cols = np.stack([cx + d for d in (-1, 0, 1, 2, 3, 4)], 1)                                  # (nx, 6)
    cols[:, 0] = np.where(X0 == 0, cx + 1, cols[:, 0])                                         # (c2, c1) at the left edge
    cols[:, 5] = np.where(cx + 4 >= cw, cx + 3, cols[:, 5])                                    # (c4, c4) at the right edge
    taps = coarse.astype(np.int64)[rows[:, None, :, None], cols[None, :, None, :]]            # (ny, nx, 3, 6, planes)
    lo, hi = taps.min(axis=(2, 3)), taps.max(axis=(2, 3))
    active = ((Y0 < y1)[:, None] & (X0 < x1)[None, :])[:, :, None] & np.ones(3, bool)
    packed = (lo >= -TAP_LIMIT) & (hi <= TAP_LIMIT)
    return packed & active, ~packed & active, np.where(active, lo, 0), np.where(active, hi, 0)


def classify(scene, adopted=False):
    """-> dict: "flags", "kernels", "prof", "replayed" (expected_launches); "down0": run classes of the level-0 pyrDown and packed /
    fp32 mask sums per wavefront step; per level of the packed gathers "tier" (normalisation), "collapse" (packed / 32-bit per plane,
    extreme taps), "wrap" (lanes whose true sums leave int16, per sign and number of turns), "weights" (ones / general image visits of
    mb_level_pk_kernel), "search" (images per tile: rectangle hits and hits after the occupancy map); "defer": deferred lanes, entries
    per segment, wavefronts by number of deferred lanes"""
    ref, out, mask = numpy_reference(scene)
    B, flags = scene.B, host_flags(scene)
    kernels, prof, replayed = expected_launches(scene, adopted)
    res = {"B": B, "flags": flags, "kernels": kernels, "prof": prof, "replayed": replayed, "levels": {}, "out": out, "mask": mask, "ref": ref}
    rx, ry, rw, rh = scene.proi
    fw_final, fh_final = scene.roi[2], scene.roi[3]
    res["down0"] = classify_down0(scene) if B >= 1 else {}
    if B < FAST_LEVELS_BELOW or not flags["fast"]:
        return res
    xb, xe = level_regions(B, 0, fw_final, rw)
    # true (unwrapped) sums of every level
    true = [np.zeros((rh >> i, rw >> i, 3), np.int64) for i in range(B + 1)]
    for fd in ref.fed:
        x0, y0, w, h = fd["rect"]
        for i in range(B + 1):
            prod = NB.trunc_short((fd["lap"][i].astype(np.float32) * fd["w"][i][:, :, None]).astype(np.float32))
            true[i][y0 >> i:(y0 + h) >> i, x0 >> i:(x0 + w) >> i] += prod
    for lv in range(0, B - FAST_LEVELS_BELOW + 1):
        if lv == 0 and not flags["all_u8"]:
            continue  # int16 sources: the generic level-0 kernel
        x1, y1 = xe[lv], (fh_final if lv == 0 else rh >> lv)
        ph, pw = rh >> lv, rw >> lv
        Y0, X0 = np.arange(0, ph, 2), np.arange(0, pw, 8)
        active = (Y0 < y1)[:, None] & (X0 < x1)[None, :]
        L = {"lanes": int(active.sum())}
        # accumulator wrap
        t = true[lv]
        turns = np.floor_divide(t + 32768, 65536)  # 0: inside int16; +-k: k times round
        tmax, tmin = _lanes(turns, np.max).max(axis=2), _lanes(turns, np.min).min(axis=2)
        L["wrap"] = {"+1": int((active & (tmax == 1)).sum()), "+2": int((active & (tmax >= 2)).sum()),
                     "-1": int((active & (tmin == -1)).sum()), "-2": int((active & (tmin <= -2)).sum())}
        # collapse
        pk, wide, lo, hi = _collapse((ph, pw), ref.finished[lv + 1], x1, y1)
        L["collapse"] = {"packed": [int(v) for v in pk.sum(axis=(0, 1))], "wide": [int(v) for v in wide.sum(axis=(0, 1))],
                         "tap_min": int(lo.min()), "tap_max": int(hi.max()),
                         "at_limit": {v: int(((hi == v) & (lo >= -abs(v))).sum() if v > 0 else ((lo == v) & (hi <= abs(v))).sum())
                                      for v in (-TAP_LIMIT - 1, -TAP_LIMIT, TAP_LIMIT, TAP_LIMIT + 1)},
                         "one_plane": int((wide.sum(axis=2) == 1).sum())}
        if lv == 0:
            cnt = np.zeros((rh, rw), np.int64)
            grey = np.zeros((rh, rw), bool)
            for fd, (_, m, _) in zip(ref.fed, scene.feeds):
                ix, iy, iw, ih = fd["image"]
                cnt[iy:iy + ih, ix:ix + iw] += m & 1
                grey[iy:iy + ih, ix:ix + iw] |= ~np.isin(m, (0, 255))
            cmax = _lanes(cnt, np.max)
            deferred = _lanes(grey, np.any) & active & (not flags["pk_ok"])
            tier = np.where(cmax <= COUNT_SIGN, 0, np.where(cmax <= COUNT_SHIFT, 1, np.where(cmax < COUNT_RCP, 2, 3)))
            names = ("sign", "shift", "rcp", "div")
            L["tier"] = {names[i]: int((active & ~deferred & (tier == i)).sum()) for i in range(4)}
            L["tier"]["deferred"] = int(deferred.sum())
            L["count_max"] = int(cnt.max())
            # limits inside a patch: lanes whose counts lie on both sides of a tier limit
            cmin = _lanes(np.where(cnt > 0, cnt, 1 << 30), np.min)
            L["straddle"] = {"%d|%d" % (a, a + 1): int((active & (cmin <= a) & (cmax > a)).sum()) for a in (1, 2, 15, 254)}
            # exact multiples: a = q n with a != 0 (the quotient a / (n + 1e-5) truncates to q -+ 1 ... q), per tier and sign
            acc = ref.lap[0].astype(np.int64)
            with np.errstate(divide="ignore", invalid="ignore"):
                exact = (cnt[:, :, None] > 1) & (acc != 0) & (acc % np.maximum(cnt, 1)[:, :, None] == 0)
            L["exact"] = {"+": int((exact & (acc > 0)).sum()), "-": int((exact & (acc < 0)).sum())}
            # one above and one below a multiple (counts >= 3: with 2 the two are the same sums)
            rem, c3 = acc % np.maximum(cnt, 1)[:, :, None], (cnt >= 3)[:, :, None]
            above, below = c3 & (rem == 1), c3 & (rem == (cnt - 1)[:, :, None])
            L["off_by_one"] = {"+above": int((above & (acc > 0)).sum()), "+below": int((below & (acc > 0)).sum()),
                               "-above": int((above & (acc < 0)).sum()), "-below": int((below & (acc < 0)).sum())}
            L["acc_extremes"] = {"max": int((acc == 32767).sum()), "min": int((acc == -32768).sum())}
            if not flags["pk_ok"]:
                segs, per_wave = collections.Counter(), collections.Counter()
                for yi, xi in np.argwhere(active.any(axis=1)[:, None] & (np.arange(0, pw, TILE_W) < x1)[None, :]):
                    d = int(deferred[yi, xi * LANES:(xi + 1) * LANES].sum())
                    per_wave[d] += 1
                    if d:
                        segs[int(xi) % DEFER_SEGS] += d
                    first = np.flatnonzero(deferred[yi, xi * LANES:(xi + 1) * LANES])
                    if len(first) == 1:
                        per_wave["only lane %d" % first[0]] += 1
                L["defer"] = {"segments": dict(segs), "per_wave": dict(per_wave), "tile_columns": int(-(-x1 // TILE_W))}
        # the image search, and (levels >= 1) the weights of every image visit
        has_occ = not any(scene.s16)
        rect_hits = occ_hits = 0
        weights, tier, per_ballot = collections.Counter(), collections.Counter(), collections.Counter()
        for y0 in range(0, y1, 2):
            for tile_x in range(0, x1, TILE_W):
                lanes_x = np.arange(tile_x, min(tile_x + TILE_W, x1), 8)
                ones, mixed = np.zeros(len(lanes_x), int), np.zeros(len(lanes_x), bool)
                for k, fd in enumerate(ref.fed):
                    rect_hits += _search_hit(fd, lv, tile_x, y0, False)
                    if not _search_hit(fd, lv, tile_x, y0, has_occ and not scene.s16[k]):
                        continue
                    occ_hits += 1
                    per_ballot[k // COVER_IMAGES] += 1
                    if lv == 0:
                        continue
                    fx, fy, fw, fh = (v >> lv for v in fd["rect"])
                    lx, ly = lanes_x - fx, y0 - fy
                    inside = (lx >= 0) & (lx < fw)
                    if not (0 <= ly < fh) or not inside.any():
                        continue
                    w = fd["w"][lv][ly:ly + 2]
                    all1 = np.array([bool((w[:, x:x + 8] == 1).all()) for x in lx[inside]])
                    hi = np.array([bool((w[:, x:x + 8] != 0).any()) for x in lx[inside]])
                    weights["ones" if all1.all() else "general"] += 1
                    ones[inside] += all1
                    mixed[inside] |= ~all1 & hi
                if lv > 0:
                    sign = ~mixed & (ones <= 1)
                    tier["sign"] += int(sign.sum())
                    tier["div"] += int((~sign).sum())
        # a wavefront asks 64 images per ballot: ceil(n / 64) ballots; hits by the ballot that returns them
        L["search"] = {"rect": rect_hits, "hit": occ_hits, "ballots": -(-flags["n"] // COVER_IMAGES),
                       "hits_in_ballot": [per_ballot[i] for i in range(-(-flags["n"] // COVER_IMAGES))]}
        if lv > 0:
            L["weights"], L["tier"] = dict(weights), dict(tier)
        res["levels"][lv] = L
    return res


def classify_down0(scene):
    """dn_task_level0 / mb_down0_lds_kernel restated on the geometry (and, for the ballot, on the mask bytes): per image the class of
    every 11-pixel run, the s_low values of the mirrored runs, NEAR, and per wavefront step (4 bordered rows x 16 runs) of the images of
    a launch that is not declared binary whether the mask sums are packed or fp32"""
    B = scene.B
    runs, s_lows, near_c, masks = collections.Counter(), collections.Counter(), collections.Counter(), collections.Counter()
    limits, wave = collections.Counter(), collections.Counter()
    declared = all(scene.binary) and not any(scene.s16)
    for k, (img, m, tl) in enumerate(scene.feeds):
        ih, iw = m.shape
        (fx, fy, fw, fh), (left, top) = feed_rect(B, scene.proi, iw, ih, tl)
        if scene.s16[k]:
            runs["generic (int16)"] += 1
            continue
        ow, oh = fw >> 1, fh >> 1
        near = left <= iw and fw - left - iw <= iw and top <= ih and fh - top - ih <= ih
        near_c["near" if near else "far"] += 1
        if near and (left == iw or fw - left - iw == iw or top == ih or fh - top - ih == ih):
            limits["near at its limit"] += 1
        cls = {}
        for xo in range(0, ow, 4):
            c0 = 2 * xo - 2
            a0 = c0 - left
            in_frame = c0 >= 0 and c0 + 10 < fw
            if in_frame and a0 >= 0 and a0 + 10 < iw:
                cls[xo] = "interior"
                limits["interior a0 = 0"] += a0 == 0
                limits["interior a0 + 10 = iw - 1"] += a0 + 10 == iw - 1
            elif in_frame and (a0 + 10 < 0 or a0 >= iw):
                s_low = -(a0 + 10) - 1 if a0 + 10 < 0 else 2 * iw - 1 - (a0 + 10)
                side = "left" if a0 + 10 < 0 else "right"
                if s_low >= 0 and s_low + 10 < iw:
                    cls[xo] = "mirrored " + side
                    limits["s_low = 0"] += s_low == 0
                    limits["s_low + 10 = iw - 1"] += s_low + 10 == iw - 1
                else:
                    cls[xo] = "border"
                    limits["mirror fails " + side] += 1
                    limits["mirror fails by one"] += s_low == -1 or s_low + 10 == iw
            else:
                cls[xo] = "border"
                limits["c0 < 0"] += c0 < 0
                limits["c0 + 10 >= fw"] += c0 + 10 >= fw
                limits["a0 = -1"] += a0 == -1
                limits["a0 + 10 = iw"] += a0 + 10 == iw
        for c in cls.values():
            runs[c] += 1
        # mb_down0_lds_kernel's choice per wavefront, ahead of dn_task_level0: where the image is NEAR and every run of the tile column is
        # interior or mirrored, a lane takes its two tasks in one batch of loads (its own copy of the mirrored byte picks and of the grey
        # ballot); otherwise the task loop calls dn_task_level0.  The four wavefronts of a workgroup hold the same 16 runs
        is_batched = {}
        for X0 in range(0, ow, DN_TOW):
            mine = [cls[xo] for xo in range(X0, min(X0 + DN_TOW, ow), 4)]
            is_batched[X0] = near and all(c == "interior" or c.startswith("mirrored") for c in mine)
            wave[("batched" if is_batched[X0] else "task loop")] += 1
            if is_batched[X0]:
                wave["batched: mirrored runs"] += sum(c.startswith("mirrored") for c in mine)
                wave["batched: interior runs"] += sum(c == "interior" for c in mine)
                wave["batched: mirrored and interior in one tile"] += len(set(mine)) > 1
        # rows: by on -1, 0, ih - 1, ih
        for row in range(-2, fh + 1):
            r = -row if row < 0 else (2 * fh - 2 - row if row >= fh else row)  # reflect101 one image away
            by = r - top
            for name, v in (("by = -1", -1), ("by = 0", 0), ("by = ih - 1", ih - 1), ("by = ih", ih)):
                limits[name] += by == v
        if declared:
            continue
        # the per-wavefront ballot: tiles of 64 x 14 outputs, steps of 4 bordered rows
        for Y0 in range(0, oh, DN_TOH):
            r_end = 2 * min(DN_TOH, oh - Y0) + 3
            for X0 in range(0, ow, DN_TOW):
                for g in range(0, DN_ROWS, 4):
                    odd = seen = False
                    for r in range(g, min(g + 4, r_end, DN_ROWS)):
                        row = 2 * Y0 - 2 + r
                        rr = -row if row < 0 else (2 * fh - 2 - row if row >= fh else row)
                        by = rr - top
                        for q in range(RUN_GROUP):
                            xo = X0 + 4 * q
                            if xo >= ow or cls[xo] != "interior":
                                continue
                            seen = True
                            if 0 <= by < ih:
                                a0 = 2 * xo - 2 - left
                                odd |= bool((~np.isin(m[by, a0:a0 + RUN], (0, 255))).any())
                                if a0 + RUN < iw and m[by, a0 + RUN] not in (0, 255) and np.isin(m[by, a0:a0 + RUN], (0, 255)).all():
                                    limits["grey in byte 11 only"] += 1
                                limits["grey in byte 0"] += m[by, a0] not in (0, 255)
                                limits["grey in byte 10"] += m[by, a0 + 10] not in (0, 255)
                    if seen:
                        masks["fp32" if odd else "packed"] += 1
                        if is_batched[X0]:
                            masks["batched fp32" if odd else "batched packed"] += 1
    return {"runs": dict(runs), "near": dict(near_c), "limits": {k: int(v) for k, v in limits.items() if v}, "mask_sums": dict(masks),
            "waves": {k: int(v) for k, v in wave.items()}}


# ---------------------------------------------------------------------------------------------------------------------------------
# Family 1.  Accumulator wrap: n copies of one image over the same pixels under full masks.  The image holds isolated 255 pixels, 2 x 2
# and 4 x 4 blocks of 255 on 0 in its left half and the inverse in its right half: the Laplacians are about +-220 at level 0 and
# +-130 at level 1, and n of them pass +32767 and -32768.  s16: "same": image 0 fed as int16 with the same values (the panorama must not
# change; levels 1 .. B - 3 then take mb_level_fast_kernel, level 0 the generic kernel) | "big": image 0 holds 127 times the values, so
# that its own Laplacians saturate and the sums go round more than once
# ---------------------------------------------------------------------------------------------------------------------------------
WRAP_W, WRAP_H, WRAP_BANDS = 96, 16, 4
WRAP_N = (128, 129, 150, 255)


def wrap_image():
    a = np.zeros((WRAP_H, WRAP_W // 2), np.uint8)
    a[1::4, 1:16:4] = 255                      # isolated pixels
    for y in (2, 10):
        for x in (18, 26):
            a[y:y + 2, x:x + 2] = 255          # 2 x 2 blocks: level 1
    a[4:8, 36:40] = 255                        # a 4 x 4 block
    a[10:14, 42:46] = 255
    img = np.concatenate([a, 255 - a], axis=1)
    return np.repeat(img[:, :, None], 3, axis=2)


def accumulator_wrap(n, s16=None):
    img = wrap_image()
    img[:, :, 1] = img[::-1, :, 1]             # three different planes
    img[:, :, 2] = img[:, ::-1, 2]
    feeds = [(img, _full(WRAP_H, WRAP_W), (0, 0))] * n
    if s16:  # "same": image 0 | "big": images 0 .. 2, each about 100 times a u8 image: the sums go round more than once
        first = img.astype(np.int16) * (127 if s16 == "big" else 1)
        k = 3 if s16 == "big" else 1
        feeds = [(first, feeds[0][1], (0, 0))] * k + feeds[k:]
    # |L| <= 255 per u8 image and level: n images stay inside int16 while n * 255 <= 32767
    return Scene(WRAP_BANDS, feeds, {"n": n, "cannot_wrap": n * 255 <= 32767, "cannot_wrap_twice": not s16 and n * 255 < 98304})


# ---------------------------------------------------------------------------------------------------------------------------------
# Family 1b.  Sums exactly on the ends of int16.  137 copies of image A and one image B over the same pixels, full masks.  The left half
# of both is 0, the right half 255; at the odd row 5 they hold single pixels whose level-0 Laplacians L(v) (239 for 255 on 0 at an odd
# row and column, found per value v by a search in numpy over image counts and pixel values) add up to the ends:
#   column  9: 137 L(254) + L(172) =  32767
#   column 21: 137 L(254) + L(173) =  32768, which wraps to -32768
#   column 41: 137 L(0)   + L(228) = -32768 on the bright half, no wrap
# (u8 feeds need 129 images at least for either end, so only the division tier sees them)
# ---------------------------------------------------------------------------------------------------------------------------------
EXTREME_N = 138
EXTREME_SPOTS = {(5, 9): (254, 172, 32767), (5, 21): (254, 173, -32768), (5, 41): (0, 228, -32768)}  # (row, column): (v in A, v in B, sum)


def acc_extremes():
    a = np.zeros((16, 64, 3), np.uint8)
    a[:, 32:] = 255
    b = a.copy()
    for (y, x), (va, vb, _) in EXTREME_SPOTS.items():
        a[y, x], b[y, x] = va, vb
    feeds = [(a, _full(16, 64), (0, 0))] * (EXTREME_N - 1) + [(b, _full(16, 64), (0, 0))]
    return Scene(3, feeds, {"sums": {k: v[2] for k, v in EXTREME_SPOTS.items()}})


# ---------------------------------------------------------------------------------------------------------------------------------
# Family 2.  Count edges: n images of the panorama's size over the same pixels; image k's mask is 255 where the constructed count map
# exceeds k, so the coverage count of every pixel is the map's value.  Per pair (lo, hi) of COUNT_PAIRS 18 strips of 8 columns: the
# limit between pixel j and j + 1 for j = 0 .. 7 (j = 7: between two lanes) with lo on the left, the same with hi on the left, and the
# limit between the two rows of a patch both ways.  Rows 2 .. 7 repeat rows 0, 1 rotated by 1, 2, 3 pair blocks.  n - 1 images are
# equal and the last differs by one grey level on a checkerboard: the sums are exact multiples of the count where the checkerboard is
# even, one off where it is odd
# ---------------------------------------------------------------------------------------------------------------------------------
COUNT_H, COUNT_BANDS = 8, 4
COUNT_N = (1, 2, 3, 15, 16, 17, 63, 64, 65, 128, 129, 255, 256)


def count_pairs(n):
    pairs = [(0, 1), (1, 2), (2, 3), (15, 16), (16, 17), (17, n)]
    return [(min(a, n), min(b, n)) for a, b in pairs]


def count_map(n):
    blocks = []
    for lo, hi in count_pairs(n):
        rows = np.zeros((2, 18, 8), np.int64)
        for j in range(8):
            rows[:, j, :j + 1], rows[:, j, j + 1:] = lo, hi
            rows[:, 8 + j, :j + 1], rows[:, 8 + j, j + 1:] = hi, lo
        rows[0, 16], rows[1, 16] = lo, hi
        rows[0, 17], rows[1, 17] = hi, lo
        blocks.append(rows.reshape(2, 18 * 8))
    band = np.concatenate(blocks, axis=1)
    return np.concatenate([np.roll(band, 144 * k, axis=1) for k in range(COUNT_H // 2)], axis=0)


def count_edges(n):
    cmap = count_map(n)
    h, w = cmap.shape
    base = _noise(20, h, w)
    base[:, :, 0] = np.where(np.add.outer(np.arange(h), np.arange(w)) % 3 == 0, 255, 0)  # plane 0: extremes
    last = base.copy()
    yy, xx = np.mgrid[0:h, 0:w]
    odd = ((yy + xx) & 1) == 1
    last[odd] = np.where(last[odd] == 255, 254, last[odd] + 1)
    feeds = [((last if k == n - 1 else base), np.where(cmap > k, 255, 0).astype(np.uint8), (0, 0)) for k in range(n)]
    cmax = _lanes(cmap, np.max)
    tiers = {"sign": int((cmax <= 1).sum()), "shift": int(((cmax > 1) & (cmax <= 2)).sum()),
             "rcp": int(((cmax > 2) & (cmax < 16)).sum()), "div": int((cmax >= 16).sum())}
    return Scene(COUNT_BANDS, feeds, {"n": n, "count_map": cmap, "tiers": tiers, "counts": sorted(set(cmap.ravel().tolist()))})


# ---------------------------------------------------------------------------------------------------------------------------------
# Family 3.  Grey bytes: two overlapping u8 images with binary masks, 520 columns (two tile columns) by 6 rows, and single grey bytes
# in the mask of image 0 at the places `which` names.  A grey byte makes its mask non-binary: the level-0 gather defers the lanes over
# it, the level-0 pyrDown takes fp32 mask sums in the wavefront steps that read it
# ---------------------------------------------------------------------------------------------------------------------------------
GREY_W, GREY_H, GREY_BANDS = 520, 6, 3
GREY_WHICH = ("lane0_px0", "lane0_px7", "lane63_px0", "lane63_px7", "all64", "n64", "n65", "run_bytes", "views")
# (which, value): every grey value at the single-byte places; "all64" holds all four values and "views" none
GREY_CASES = tuple((w, v) for w in GREY_WHICH[:4] + ("run_bytes",) for v in GREYS) + (("all64", 1), ("n64", 127), ("n65", 128), ("views", 254))


def grey_bytes(which, value=127):
    m0, m1, corner1 = _full(GREY_H, GREY_W), _full(GREY_H, 300), (133, 0)
    m0[:, 400:450] = 0
    spots, pitched = [], None
    if which.startswith("lane"):
        lane, px = int(which[4:which.index("_")]), int(which[-1])
        spots = [(0 if px == 0 else 1, 8 * lane + px)]
    elif which == "all64":
        spots = [(2, 8 * lane + (lane % 8)) for lane in range(LANES)]
    elif which in ("n64", "n65"):  # 64 / 65 patches of tile column 0: lanes 0 .. 31 of the row pairs 0 and 1, and lane 40 of row pair 2
        spots = [(2 * rp + (lane & 1), 8 * lane + 3) for rp in (0, 1) for lane in range(32)] + ([(4, 8 * 40)] if which == "n65" else [])
    elif which == "run_bytes":
        # image 0 lies at column 0 of its feed rectangle: run q reads the mask columns 8 q - 2 .. 8 q + 8.  Bytes 0 and 10 of run 1
        # (columns 6, 16), and column 513: byte 11 of the last interior run (from 502 to 512; the run from 510 would end at 520 = iw and
        # meets the border), read by no interior run
        spots = [(0, 6), (3, 16), (5, 8 * 63 - 2 + RUN)]
    elif which == "views":
        # no grey byte anywhere, but the masks are views amid seeded bytes 1 .. 254: not declared binary, nothing deferred.  Image 1 is
        # two rows high at row 1 and ends at column 433: the lanes over it read a clamped row above and below it (cleared by the row
        # mask) and, in the strip from 432, seven bytes of the surroundings (cleared by lane_valid_bytes)
        pitched = {0: ("random", "random", 7), 1: ("random", "random", 5)}
        m1, corner1 = _full(2, 300), (133, 1)
    for i, (y, x) in enumerate(spots):
        m0[y, x] = value if which != "all64" else GREYS[i % 4]
    feeds = [(_noise(30, GREY_H, GREY_W), m0, (0, 0)), (_noise(31, m1.shape[0], 300), m1, corner1)]
    patches = sorted({(y // 2, x // 8) for y, x in spots})
    return Scene(GREY_BANDS, feeds, {"spots": spots, "deferred": patches, "declared_binary": False,
                                     "segments": dict(collections.Counter(x // LANES % DEFER_SEGS for _, x in patches))}, pitched)


# one grey byte in tile column 0 and one in tile column 256: both queue into segment 0
WIDE_W = DEFER_SEGS * TILE_W + 16


def grey_wide():
    feeds = []
    for k, x in enumerate((0, DEFER_SEGS * TILE_W)):
        m = _full(4, 16)
        m[1, 3 + k] = GREYS[k]
        feeds.append((_noise(40 + k, 4, 16), m, (x, 0)))
    return Scene(3, feeds, {"deferred": [(0, 0), (0, DEFER_SEGS * LANES)], "segments": {0: 2}, "tile_columns": DEFER_SEGS + 1})


# ---------------------------------------------------------------------------------------------------------------------------------
# Family 4.  Level-0 pyrDown runs: a backdrop and small images whose widths, heights and corners put 11-pixel runs on each side of
# every limit of dn_task_level0.  (iw, ih, x, y): with 3 bands the border is 24 columns; an image at x < 24 has left = x
# ---------------------------------------------------------------------------------------------------------------------------------
DOWN0_BANDS = 3
DOWN0_BACKDROP = (200, 72)
DOWN0_SMALL = ((1, 1, 40, 2), (2, 2, 60, 3), (3, 3, 80, 1), (10, 10, 100, 5), (11, 11, 17, 20), (12, 12, 19, 40), (13, 12, 19, 56),
               (25, 25, 120, 30), (24, 24, 150, 4), (11, 3, 189, 60), (12, 1, 170, 44), (23, 30, 17, 36), (12, 5, 15, 64))


def down0_runs(grey=False):
    w, h = DOWN0_BACKDROP
    feeds = [(_noise(50, h, w), _full(h, w), (0, 0))]
    for k, (iw, ih, x, y) in enumerate(DOWN0_SMALL):
        m = _full(ih, iw)
        if grey and iw >= 11:
            m[ih // 2, 0] = GREYS[k % 4]
        feeds.append((_noise(51 + k, ih, iw), m, (x, y)))
    return Scene(DOWN0_BANDS, feeds, {"widths": sorted({s[0] for s in DOWN0_SMALL}), "heights": sorted({s[1] for s in DOWN0_SMALL})})


# ---------------------------------------------------------------------------------------------------------------------------------
# Family 4b.  Batched pyrDown wavefronts.  With 7 bands the border is 384 columns: an image 400 x 64 at column 384 of a panorama of
# 1152 x 64 (128 padded: NEAR, at its limit below) has tile columns of 64 outputs (128 inputs) that lie wholly in its left or right border one mirror image away, tile columns wholly
# inside it, and tile columns that hold the image's edge (not batched).  grey: one grey byte in an interior batched tile column (the
# batched branch's own ballot) and one in the image's first column
# ---------------------------------------------------------------------------------------------------------------------------------
BATCHED_BANDS, BATCHED_W = 7, 1152


def down0_batched(grey=False):
    m = _full(64, 400)
    if grey:
        m[3, 150], m[40, 0] = GREYS[1], GREYS[3]
    feeds = [(_noise(55, 64, 400), m, (384, 0)), (_noise(56, 64, 64), _full(64, 64), (0, 0)), (_noise(57, 64, 64), _full(64, 64), (BATCHED_W - 64, 0))]
    return Scene(BATCHED_BANDS, feeds, {"border": border(BATCHED_BANDS)})


# ---------------------------------------------------------------------------------------------------------------------------------
# Family 5.  pyrUp borders: panoramas 8, 16 and 40 columns wide (coarse widths 4, 8, 20 under level 0) and 40 rows high with 3 bands:
# every strip of the narrowest is at once the first (X0 == fx) and the last of its row.  The device test feeds the images as views amid
# seeded bytes.  (A feed rectangle is a multiple of 2^B >= 8 wide and high and the packed gathers run on the levels <= B - 3 only: coarse
# sizes 1, 2 and 5 are the coarse kernel's and the generic kernels', see profiles/constructed_multiband.md)
# ---------------------------------------------------------------------------------------------------------------------------------
UP_W = (8, 16, 40)
UP_H = 40
UP_CASES = ((8, 3), (16, 3), (40, 3), (16, 4))  # (width, bands): 16 columns with 4 bands make level 1 one strip wide for mb_level_pk_kernel


def up_borders(w, bands=3):
    rng = np.random.default_rng(60 + w)
    m0 = np.where(rng.random((UP_H, w)) < 0.8, 255, 0).astype(np.uint8)
    m1 = np.where(rng.random((UP_H - 7, max(w - 3, 1))) < 0.8, 255, 0).astype(np.uint8)
    feeds = [(_noise(61, UP_H, w), m0, (0, 0)), (_noise(62, m1.shape[0], m1.shape[1]), m1, (min(3, w - m1.shape[1]), 7))]
    return Scene(bands, feeds, {"coarse_w": w // 2}, {0: ("random", 255, 6), 1: ("random", 0, 9)})


# ---------------------------------------------------------------------------------------------------------------------------------
# Family 6.  Occupancy edges: a backdrop, and an image of the panorama's size whose mask is 0 but for single pixels.  A pixel at column
# x gives W_1 its weight at the columns x' with 2 x' - 2 <= x <= 2 x' + 2.  Column 125: x' = 62, 63 — the last column of occupancy
# cell 0 of level 1; column 130: x' = 64 .. 66 — the first of cell 1; column 127: both; column 511 (with 1040 columns): the last column of
# tile column 0 at level 0, whose weight at level 1 reaches x' = 256 under tile column 1.  An image whose mask is all 0 is fed first,
# in the middle or last
# ---------------------------------------------------------------------------------------------------------------------------------
OCC_W = (512, 520, 1024, 1040)
OCC_H, OCC_BANDS = 8, 4
OCC_ZERO_AT = ("first", "middle", "last")


def occupancy_edges(w, zero_at="middle"):
    dots = [(0, 125), (2, 130), (5, 127), (7, 63), (6, 64)] + ([(3, 511), (4, 512)] if w > 512 else [(3, 511)]) + [(1, w - 1)]
    m = np.zeros((OCC_H, w), np.uint8)
    for y, x in dots:
        m[y, x] = 255
    back, sparse, zero = (_noise(70, OCC_H, w), _full(OCC_H, w), (0, 0)), (_noise(71, OCC_H, w), m, (0, 0)), (_noise(72, OCC_H, w), np.zeros((OCC_H, w), np.uint8), (0, 0))
    feeds = {"first": [zero, back, sparse], "middle": [back, zero, sparse], "last": [back, sparse, zero]}[zero_at]
    return Scene(OCC_BANDS, feeds, {"dots": dots, "zero_index": OCC_ZERO_AT.index(zero_at), "level_widths": [w >> i for i in range(OCC_BANDS + 1)]})


# ---------------------------------------------------------------------------------------------------------------------------------
# Family 7.  Collapse overshoot.  A backdrop of 255 whose mask has a square hole, and nested in the hole three images that are 0 but for
# a bright square blob at the hole's centre, each owning a square ring of the hole (mask sizes OVERSHOOT_RINGS, blob sizes
# OVERSHOOT_BLOBS).  At each level the image whose ring matches the level's scale dominates the weights, and its Laplacian there is
# positive: the normalised levels add up above 255.  The placement was found by a search in numpy (exhaustive over nested squares of
# 2 .. 48 pixels, then 8700 random draws of ring sizes, blob sizes and centres; profiles/constructed_multiband.md): the largest tap of
# the finished level 1 is 575 with 5 bands (584 in the random draws), and the value of the innermost blob tunes it down to exactly 500
# and 501.  The same scene twice as large with 6 bands puts the largest tap of the finished level 2 (mb_level_pk_kernel's collapse at
# level 1) on 500 and 501.  No u8 placement found reaches -500: the inverse scene ("neg") stops at -333.
# which: (level of the finished taps, largest tap) | "one_plane": planes 1 and 2 of every image hold 128 (taps of 128) | "neg"
# ---------------------------------------------------------------------------------------------------------------------------------
OVERSHOOT_RINGS, OVERSHOOT_BLOBS, OVERSHOOT_CENTRE = (5, 14, 20), (5, 14, 25), (66, 32)
OVERSHOOT_VALUE = {("l1", 500): 158, ("l1", 501): 159, ("l1", 575): 255, ("l2", 500): 172, ("l2", 501): 175}
OVERSHOOT_CASES = ("l1_500", "l1_501", "l1_575", "l1_501_one_plane", "l2_500", "l2_501", "neg")


def collapse_overshoot(which):
    parts = which.split("_")
    scale = 2 if parts[0] == "l2" else 1
    neg = which == "neg"
    value = 255 if neg else OVERSHOOT_VALUE[(parts[0], int(parts[1]))]
    w, h = 160 * scale, 64 * scale
    cx, cy = (v * scale for v in OVERSHOOT_CENTRE)
    bright, dark = (0, 255) if neg else (255, 0)
    feeds = [[np.full((h, w, 3), bright, np.uint8), _full(h, w), (0, 0)]]
    squares = []
    for i, (s, bl) in enumerate(zip(OVERSHOOT_RINGS, OVERSHOOT_BLOBS)):
        s, bl = s * scale, bl * scale
        img = np.full((h, w, 3), dark, np.uint8)
        img[cy - bl // 2:cy - bl // 2 + bl, cx - bl // 2:cx - bl // 2 + bl] = (255 - value if neg else value) if i == 0 else bright
        m = np.zeros((h, w), np.uint8)
        m[cy - s // 2:cy - s // 2 + s, cx - s // 2:cx - s // 2 + s] = 255
        feeds.append([img, m, (0, 0)])
        squares.append((cx - s // 2, cy - s // 2, s))
    for i in range(len(squares) - 1, -1, -1):  # every mask without the smaller squares, the backdrop without the largest
        x0, y0, s = squares[i]
        for f in [feeds[0]] + feeds[i + 2:]:
            f[1][y0:y0 + s, x0:x0 + s] = 0
    if "plane" in which:
        for f in feeds:
            f[0][:, :, 1:] = 128
    facts = {"level": scale, "tap": None if neg else int(parts[1]), "packed": neg or int(parts[1]) <= TAP_LIMIT, "one_plane": "plane" in which}
    return Scene(4 + scale, [tuple(f) for f in feeds], facts)


# ---------------------------------------------------------------------------------------------------------------------------------
# Family 8.  The launch matrix: the smallest scenes that make the host pick each launch reachable through the public entry points
# ---------------------------------------------------------------------------------------------------------------------------------
LAUNCH_CASES = ("bands0", "bands1", "bands2", "bands3", "bands5", "mixed_s16", "all_s16", "s16_overshoot", "grey", "n256")


def launch_matrix(case):
    w, h = 72, 40
    a, b = (_noise(80, h, w), _full(h, w), (0, 0)), (_noise(81, h - 8, w - 16), _full(h - 8, w - 16), (11, 5))
    b[1][:3, :5] = 0
    if case.startswith("bands"):
        return Scene(int(case[5:]), [a, b], {"case": case})
    if case == "mixed_s16":
        return Scene(5, [a, (b[0].astype(np.int16) * 64 - 8000, b[1], b[2])], {"case": case})
    if case == "all_s16":
        return Scene(5, [(a[0].astype(np.int16) * 128, a[1], a[2]), (b[0].astype(np.int16) * -128, b[1], b[2])], {"case": case})
    if case == "s16_overshoot":  # the overshoot scene 128 times as bright: the collapse's saturating add clips at 32767
        o = collapse_overshoot("l1_575")
        return Scene(o.bands, [(i.astype(np.int16) * 128, m, c) for i, m, c in o.feeds], {"case": case, "saturates": True})
    if case == "grey":
        g = b[1].copy()
        g[:, -4:] = np.array([200, 150, 100, 50], np.uint8)
        return Scene(5, [a, (b[0], g, b[2])], {"case": case})
    if case == "n256":
        return Scene(4, [a] + [(b[0][:8, :8], _full(8, 8), (k % 64, k // 64 * 8)) for k in range(255)], {"case": case})
    raise ValueError(case)


# strips, contributions and emit: three images over 1100 x 40 that two ranks share (stitching_amd.distributed, one process acting for
# both).  binary: every launch stays packed; grey: a received contribution next to a mask that is not binary (level 0 through
# mb_level_fast_kernel<true, true, false, false>); s16: an int16 image (the general emit class, the generic level-0 emit)
SHARDED_CASES = ("binary", "grey", "s16")
SHARDED_BANDS = 4


def sharded(case):
    h = 40
    feeds = []
    for k, (x, w) in enumerate(((0, 500), (380, 420), (700, 400))):
        m = _full(h - k, w)
        m[:4, :9] = 0
        if case == "grey" and k == 1:
            m[:, :5] = np.array([40, 90, 140, 190, 240], np.uint8)
        img = _noise(90 + k, h - k, w)
        if case == "s16" and k == 2:
            img = img.astype(np.int16) * 90 - 9000
        feeds.append((img, m, (x, k)))
    return Scene(SHARDED_BANDS, feeds, {"case": case, "world": 2})


# ---------------------------------------------------------------------------------------------------------------------------------
# Family 9.  Feed order: six int16 images over the same pixels under grey masks (weights k / 255: no dyadic fractions).  fp32 sums of
# such weights depend on the order of the addends; int16 wrap-around and per-product truncation do not.  (int16 values: a quotient of
# thousands shows a last-bit difference of its denominator far more often than one of a few hundred)
# ---------------------------------------------------------------------------------------------------------------------------------
def feed_order():
    rng = np.random.default_rng(95)
    h, w = 24, 88
    feeds = [(rng.integers(-20000, 20001, (h, w, 3)).astype(np.int16), rng.integers(1, 255, (h, w)).astype(np.uint8), (0, 0)) for k in range(6)]
    return Scene(3, feeds, {"grey_everywhere": True})
