"""Inputs with known transforms for the affine-registration tests (tests/test_affine_contract.py, tests/test_gpu_affine_*.py) and
tools/bench_affine.py: (a) grid rigs — landmarks of a plane seen by tiles laid out in a grid, each through its own similarity (a small
turn and scale about the tile's centre), matches and pair transforms made from the noisy projections, no images; (b) four tiles cut
from one texture through such similarities and run through the numpy detector and the affine matcher.  Features and match entries are
the contracts' dicts (tests/camera_rigs.to_package makes the package's objects of them).  Everything is computed once."""
import json
import os

import numpy as np

from tests import camera_rigs as CR
from tests import numpy_affine as NA
from tests import numpy_features as NF
from tests import numpy_matches as NM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "affine.json")
TILE = (320, 240)
PITCH = 0.7  # of the tile's size from one tile to the next: neighbours share 30 % of a side


def tile_transform(scale, degrees, at, size=TILE):
    """tile pixels -> plane: a turn and scale about the tile's centre, which lands at `at`"""
    c, s = scale * np.cos(np.deg2rad(degrees)), scale * np.sin(np.deg2rad(degrees))
    cx, cy = (size[0] - 1) / 2, (size[1] - 1) / 2
    return np.array([[c, -s, at[0] - (c * cx - s * cy)], [s, c, at[1] - (s * cx + c * cy)], [0.0, 0.0, 1.0]])


def planted(rs, cols, rows, size=TILE, pitch=PITCH, turn=2.0, scale=0.02):
    """cols * rows transforms, row-major: turns within +- turn degrees, scales within 1 +- scale"""
    return [tile_transform(1.0 + rs.uniform(-scale, scale), rs.uniform(-turn, turn), (c * pitch * size[0], r * pitch * size[1]), size)
            for r in range(rows) for c in range(cols)]


def entries_from_tracks(seen, pts, rs, min_shared=8, max_shared=120, outliers=0.0, full=False):
    """tests/camera_rigs.entries_from_tracks with the affine refit on points that are not centred"""
    n = len(seen)
    out = [NM.empty() for _ in range(n * n)]
    where = [{int(l): k for k, l in enumerate(s)} for s in seen]
    for i in range(n):
        for j in range(i + 1, n):
            both = np.array([l for l in seen[i] if int(l) in where[j]], np.int64)
            if max_shared is not None and len(both) > max_shared:
                both = np.sort(rs.permutation(both)[:max_shared])
            e = NM.empty()
            e["src_img_idx"], e["dst_img_idx"] = i, j
            if len(both) >= min_shared:
                mt = np.array([[where[i][int(l)], where[j][int(l)], 0] for l in both], np.int32).reshape(-1, 3)
                e["H"] = NA.refit(pts[i][mt[:, 0]], pts[j][mt[:, 1]], "affine_full" if full else "affine_partial")
                mask, inliers = np.ones(len(mt), np.uint8), len(mt)
                wrong = int(outliers * inliers)
                if wrong:
                    extra = np.stack([rs.randint(0, len(seen[i]), wrong), rs.randint(0, len(seen[j]), wrong), np.zeros(wrong, np.int64)], axis=1)
                    order = rs.permutation(inliers + wrong)
                    mt = np.concatenate([mt, extra.astype(np.int32)])[order]
                    mask = np.concatenate([mask, np.zeros(wrong, np.uint8)])[order]
                e["matches"], e["inliers_mask"], e["num_inliers"] = np.ascontiguousarray(mt), mask, inliers
                e["confidence"] = NM.confidence(inliers, len(mt))
            out[i * n + j], out[j * n + i] = e, NM.mirrored(e, i, j)
    return out


def grid_rig(seed, cols, rows, per_image=300, noise=0.5, size=TILE, max_shared=120, outliers=0.0):
    """-> features, matches, truth {"T"}: cols * rows tiles at a pitch of 0.7 tiles, each through its own similarity, about per_image
    landmarks in a tile, 0.5 px of noise on the projections, which are then rounded to the pixels features have"""
    rs = np.random.RandomState(seed)
    Ts = planted(rs, cols, rows, size)
    w, h = size
    lo = np.array([-0.6 * w, -0.6 * h])  # the tiles' centres lie at multiples of the pitch
    hi = np.array([(cols - 1) * PITCH * w + 0.6 * w, (rows - 1) * PITCH * h + 0.6 * h])
    count = int(per_image * (hi - lo).prod() / (w * h))
    L = np.concatenate([rs.uniform(lo, hi, (count, 2)), np.ones((count, 1))], axis=1)
    feats, seen, pts = [], [], []
    for T in Ts:
        xy = (L @ np.linalg.inv(T).T)[:, :2] + rs.normal(0.0, noise, (count, 2))
        pix = np.rint(xy)
        ids = np.flatnonzero((pix[:, 0] >= 0) & (pix[:, 0] < w) & (pix[:, 1] >= 0) & (pix[:, 1] < h))
        feats.append(CR._features(pix[ids], size))
        seen.append(ids)
        pts.append(NA.uncentred(feats[-1]))
    return feats, entries_from_tracks(seen, pts, rs, max_shared=max_shared, outliers=outliers), {"T": Ts}


SIMILARITY = tile_transform(1.04, 3.0, (175.0, 101.0), (640, 480)) @ np.array([[1.0, 0.0, -12.0], [0.0, 1.0, 9.0], [0.0, 0.0, 1.0]])
AFFINE = np.array([[1.05, -0.09, 21.0], [0.04, 0.93, 30.0], [0.0, 0.0, 1.0]])  # shear and unequal scales: no similarity


def planted_pair(seed, m, A, outliers=0.3, size=(640, 480), extra=9):
    """two images' features: m landmarks, the second image's through A (level-0 pixels, not centred), rounded to the pixel grid of one of
    two levels; a share of them land at random places instead; `extra` unrelated descriptors per image.  Descriptors are random, a
    landmark's two copies equal"""
    rs = np.random.RandomState(seed)
    w, h = size
    D = rs.randint(0, 256, (m + 2 * extra, 32)).astype(np.uint8)
    c = np.stack([rs.randint(20, w - 20, m), rs.randint(20, h - 20, m)], axis=1)
    d = (np.concatenate([c, np.ones((m, 1))], axis=1) @ np.asarray(A, np.float64).T)[:, :2]
    bad = rs.permutation(m)[:int(round(outliers * m))]
    d[bad] = np.stack([rs.randint(0, w, len(bad)), rs.randint(0, h, len(bad))], axis=1)
    levels = [size, (w // 2, h // 2)]
    la, lb = rs.randint(0, 2, m + extra), rs.randint(0, 2, m + extra)
    pa = np.concatenate([c, np.stack([rs.randint(0, w, extra), rs.randint(0, h, extra)], axis=1)])
    pb = np.concatenate([np.rint(d), np.stack([rs.randint(0, w, extra), rs.randint(0, h, extra)], axis=1)]).astype(np.int64)
    pa, pb = pa // (1 + la[:, None]), pb // (1 + lb[:, None])  # the pixel of the level: half resolution at level 1
    order = rs.permutation(m + extra)
    da, db = np.concatenate([D[:m], D[m:m + extra]]), np.concatenate([D[:m], D[m + extra:]])[order]
    return [features_of(da, pa, size, levels, la), features_of(db, pb[order], size, levels, lb[order])]


def features_of(desc, xy, size=(640, 480), levels=None, level=None):
    """the contract's features dict of descriptors (n, 32) u8 at integer level pixels xy (n, 2)"""
    xy = np.asarray(xy, np.int32).reshape(-1, 2)
    n = len(xy)
    return {"img_size": size, "level_sizes": [size] if levels is None else levels,
            "level": np.zeros(n, np.int32) if level is None else np.asarray(level, np.int32), "x": xy[:, 0].copy(), "y": xy[:, 1].copy(),
            "bin": np.zeros(n, np.int32), "R": np.zeros(n, np.int64), "descriptors": np.ascontiguousarray(np.asarray(desc, np.uint8).reshape(n, 32))}


def package_features(features):
    """the package's ImageFeatures of the contract's dicts"""
    return CR.to_package(features, [])[0]


RIGS = {"grid2x2": (21, 2, 2), "grid3x2": (22, 3, 2), "row5": (23, 5, 1)}
_CACHE = {}


def rig(name):
    if name not in _CACHE:
        _CACHE[name] = grid_rig(*RIGS[name])
    return _CACHE[name]


def corner_error(Rs, truth, centre, size=TILE):
    """the largest distance in pixels between where the transforms Rs (relative to tile `centre`) and the planted ones take a tile's corners"""
    w, h = size
    corners = np.array([[0.0, 0.0, 1.0], [w, 0.0, 1.0], [0.0, h, 1.0], [w, h, 1.0]]).T
    back = np.linalg.inv(truth["T"][centre])
    got0 = np.linalg.inv(np.asarray(Rs[centre], np.float64))
    worst = 0.0
    for R, T in zip(Rs, truth["T"]):
        d = (got0 @ np.asarray(R, np.float64) @ corners - back @ T @ corners)[:2]
        worst = max(worst, float(np.sqrt((d * d).sum(axis=0)).max()))
    return worst


# ---- tiles of a texture --------------------------------------------------------------------------------------------------------------------
TEXTURE_SEED, TILES_SEED = 7, 24


def texture_tiles():
    """-> images (4 u8 BGR of 240 x 320), truth: a 2 x 2 grid of tiles of camera_rigs.texture(460, 600, 7), each through its own similarity
    (turn within +- 2 degrees, scale within +- 2 %), bilinear"""
    if "tiles" not in _CACHE:
        from scipy.ndimage import map_coordinates

        big = CR.texture(460, 600, TEXTURE_SEED)
        Ts = planted(np.random.RandomState(TILES_SEED), 2, 2)
        shift = np.array([[1.0, 0.0, 190.0], [0.0, 1.0, 150.0], [0.0, 0.0, 1.0]])  # the plane's origin (the first tile's centre) in the texture
        ys, xs = np.mgrid[0:TILE[1], 0:TILE[0]].astype(np.float64)
        p = np.stack([xs.ravel(), ys.ravel(), np.ones(xs.size)])
        imgs = []
        for T in Ts:
            q = shift @ T @ p
            img = np.stack([map_coordinates(big[:, :, k].astype(np.float64), [q[1], q[0]], order=1, mode="reflect") for k in range(3)], axis=1)
            imgs.append(np.clip(np.rint(img), 0, 255).astype(np.uint8).reshape(TILE[1], TILE[0], 3))
        _CACHE["tiles"] = (imgs, {"T": Ts})
    return _CACHE["tiles"]


def texture_case():
    """-> features, matches (the numpy detector's and affine matcher's, on the CPU), truth of texture_tiles()"""
    if "case" not in _CACHE:
        imgs, truth = texture_tiles()
        feats = [NF.detect(a) for a in imgs]
        _CACHE["case"] = (feats, NA.match(feats), truth)
    return _CACHE["case"]


CASES = sorted(RIGS) + ["texture"]
_MEASURED = {}


def measure(name):
    """the contract (tests/numpy_affine.py) on a case -> (indices, cameras, info), and what profiles/affine.json records of it"""
    from tests import numpy_cameras as NC

    if name not in _MEASURED:
        feats, matches, truth = texture_case() if name == "texture" else rig(name)
        idx, cams, info = NA.register(feats, matches)
        _, centre = NC.spanning_tree(NC.subset_matches(matches, idx), len(idx))
        kept = {"T": [truth["T"][i] for i in idx]}
        err = corner_error([c["R"] for c in cams], kept, centre)
        rms = float(np.sqrt(info["last_E"] / max(info["matches"], 1)))
        _MEASURED[name] = ((idx, cams, info), {"tiles": len(feats), "kept": len(idx), "edges": info["edges"], "matches": info["matches"],
                                               "evaluations": info["evaluations"], "accepted": info["accepted"],
                                               "rms_px": round(rms, 4), "corner_error_px": round(err, 4)})
    return _MEASURED[name]


def recorded(name):
    """the corner error profiles/affine.json holds for a case (tools/bench_affine.py --contract-only wrote it)"""
    with open(PROFILE) as f:
        return float(json.load(f)["contract"][name]["corner_error_px"])
