"""Inputs with known cameras for the camera-registration tests (tests/test_cameras_contract.py, tests/test_gpu_cameras.py) and
tools/bench_cameras.py: (a) point rigs — unit-vector landmarks seen by rotated cameras, matches and homographies made from the noisy
projections, no images; (b) four views of one texture rendered through K_big R K^-1 and run through the numpy detector and matcher.
Features and match entries are the contracts' dicts; to_package() makes the package's objects of them.  Everything is computed once."""
import numpy as np

from tests import numpy_features as NF
from tests import numpy_matches as NM

W, H = 800, 600


def rotation(yaw, pitch, roll):
    """camera-to-world rotation from degrees: yaw about y, then pitch about x, then roll about z"""
    a, b, c = np.deg2rad([yaw, pitch, roll])
    Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    Rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    return Ry @ Rx @ Rz


def angle_deg(Ra, Rb):
    """the angle of the rotation between two rotations"""
    D = np.asarray(Ra, np.float64).T @ np.asarray(Rb, np.float64)
    s = np.sqrt((D[2, 1] - D[1, 2]) ** 2 + (D[0, 2] - D[2, 0]) ** 2 + (D[1, 0] - D[0, 1]) ** 2) * 0.5
    return float(np.rad2deg(np.arctan2(s, (np.trace(D) - 1.0) * 0.5)))  # exact for small angles, where arccos of the trace is not


def _features(xy, size):
    n = len(xy)
    return {"img_size": size, "level_sizes": [size], "level": np.zeros(n, np.int32), "x": xy[:, 0].astype(np.int32).copy(),
            "y": xy[:, 1].astype(np.int32).copy(), "bin": np.zeros(n, np.int32), "R": np.zeros(n, np.int64),
            "descriptors": np.zeros((n, 32), np.uint8)}


def entries_from_tracks(seen, pts, rs, min_shared=8, max_shared=120, outliers=0.0):
    """n * n match entries of images that see landmarks: seen[i] the landmark ids of image i's features in feature order, pts[i] their
    centred points.  A pair shares the landmarks both see (at most max_shared, drawn at random; None: all); with min_shared or more it
    gets all of them as inliers, H by the normalised DLT and the matcher's confidence.  outliers: that many wrong matches per inlier are
    mixed in (random features, not inliers), as a matcher leaves them — they lower the confidence, which is 0 above 3."""
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
                e["H"] = NM.refit(pts[i][mt[:, 0]], pts[j][mt[:, 1]])
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


def point_rig(seed, n, rows=1, per_image=150, noise=0.5, size=(W, H), focal=700.0, step=(20.0, 35.0), jitter=3.0, max_shared=120, outliers=0.0):
    """-> features, matches, truth {"focals", "R"}: n cameras in `rows` rows (n a multiple of rows), focal 700 +- 5 %, yaw steps of
    20 - 35 degrees (`step`), +- 3 degrees (`jitter`) of pitch and roll (rows 22 degrees apart), 0.5 px of noise on the projections, which are then rounded
    to the pixels features have."""
    rs = np.random.RandomState(seed)
    cols = n // rows
    yaws = np.cumsum(rs.uniform(step[0], step[1], cols))
    yaws -= yaws.mean()
    Rs, focals = [], []
    for r in range(rows):
        for c in range(cols):
            Rs.append(rotation(yaws[c] + (rs.uniform(-3, 3) if rows > 1 else 0.0), (r - (rows - 1) / 2.0) * 22.0 + rs.uniform(-jitter, jitter),
                               rs.uniform(-jitter, jitter)))
            focals.append(focal * rs.uniform(0.95, 1.05))
    w, h = size
    half_x, half_y = np.rad2deg(np.arctan(w / 2 / focal)), np.rad2deg(np.arctan(h / 2 / focal))
    yaw_lo, yaw_hi = yaws[0] - half_x - 8, yaws[-1] + half_x + 8
    pit = (rows - 1) * 11.0 + half_y + 8
    count = int(per_image * (yaw_hi - yaw_lo) * 2 * pit / (4 * half_x * half_y))
    ly, lp = np.deg2rad(rs.uniform(yaw_lo, yaw_hi, count)), np.deg2rad(rs.uniform(-pit, pit, count))
    L = np.stack([np.sin(ly) * np.cos(lp), np.sin(lp), np.cos(ly) * np.cos(lp)], axis=1)
    feats, seen, pts = [], [], []
    for R, f in zip(Rs, focals):
        X = L @ R  # rows R^T l: world -> camera
        with np.errstate(all="ignore"):
            xy = f * X[:, :2] / X[:, 2:3] + rs.normal(0.0, noise, (count, 2))
        pix = np.rint(xy + (w / 2, h / 2))
        ok = (X[:, 2] > 0.1) & (pix[:, 0] >= 0) & (pix[:, 0] < w) & (pix[:, 1] >= 0) & (pix[:, 1] < h)
        ids = np.flatnonzero(ok)
        feats.append(_features(pix[ids], size))
        seen.append(ids)
        pts.append(NM.centred(feats[-1]))
    return feats, entries_from_tracks(seen, pts, rs, max_shared=max_shared, outliers=outliers), {"focals": focals, "R": Rs}


RIGS = {"row3": (11, 3, 1), "row5": (12, 5, 1), "row8": (13, 8, 1), "two_rows6": (14, 6, 2)}
_CACHE = {}


def rig(name):
    if name not in _CACHE:
        _CACHE[name] = point_rig(*RIGS[name])
    return _CACHE[name]


VIEW_W, VIEW_H, VIEW_F = 320, 240, 400.0
VIEW_YAWS = (-22.0, -8.0, 7.0, 21.0)


def texture(h, w, seed):
    """blobs of several sizes, steepened into edges and corners: the recipe of tests/test_features_contract._texture, value for value
    (tests/test_cameras_contract.py compares them)"""
    from scipy.ndimage import gaussian_filter

    rs = np.random.RandomState(seed)
    t = sum(gaussian_filter(rs.standard_normal((h, w)), s) * s for s in (1.5, 3.0, 6.0))
    t = (t - t.min()) / (t.max() - t.min())
    g = (255 * (0.5 + 0.5 * np.sign(t - 0.5) * np.abs(2 * t - 1) ** 0.5)).astype(np.uint8)
    return np.repeat(g[:, :, None], 3, axis=2)


def texture_views():
    """-> images (4 u8 BGR of 240 x 320), truth: views of texture(420, 900, 7), a plane at focal 400, through
    K_big R K^-1: yaws -22, -8, 7, 21 degrees, pitch +- 2, roll 1.5 (i - 1)"""
    if "views" not in _CACHE:
        from scipy.ndimage import map_coordinates

        big = texture(420, 900, 7)
        Kbig = np.array([[VIEW_F, 0, 450.0], [0, VIEW_F, 210.0], [0, 0, 1]])
        Kinv = np.linalg.inv(np.array([[VIEW_F, 0, VIEW_W / 2], [0, VIEW_F, VIEW_H / 2], [0, 0, 1]]))
        ys, xs = np.mgrid[0:VIEW_H, 0:VIEW_W].astype(np.float64)
        p = np.stack([xs.ravel(), ys.ravel(), np.ones(xs.size)])
        imgs, Rs = [], []
        for i, yaw in enumerate(VIEW_YAWS):
            R = rotation(yaw, 2.0 if i % 2 == 0 else -2.0, 1.5 * (i - 1))
            q = Kbig @ R @ Kinv @ p
            at = [q[1] / q[2], q[0] / q[2]]
            img = np.stack([map_coordinates(big[:, :, k].astype(np.float64), at, order=1, mode="reflect") for k in range(3)], axis=1)
            imgs.append(np.clip(np.rint(img), 0, 255).astype(np.uint8).reshape(VIEW_H, VIEW_W, 3))
            Rs.append(R)
        _CACHE["views"] = (imgs, {"focals": [VIEW_F] * 4, "R": Rs})
    return _CACHE["views"]


def texture_case():
    """-> features, matches (the numpy detector's and matcher's, on the CPU), truth of texture_views()"""
    if "case_b" not in _CACHE:
        imgs, truth = texture_views()
        feats = [NF.detect(a) for a in imgs]
        _CACHE["case_b"] = (feats, NM.match(feats), truth)
    return _CACHE["case_b"]


def to_package(features, matches):
    """the package's ImageFeatures and MatchesInfo of the contracts' dicts"""
    import stitching_amd as S

    F = []
    for k, f in enumerate(features):
        size = f.get("img_size") or f["level_sizes"][0]
        F.append(S.ImageFeatures(k, size, f["level_sizes"], f["level"], f["x"], f["y"], f["bin"], f["R"], f["descriptors"]))
    M = [S.MatchesInfo(e["src_img_idx"], e["dst_img_idx"], e["matches"], e["inliers_mask"], e["num_inliers"], e["H"], e["confidence"],
                       e["H_sample"], e["hypothesis"]) for e in matches]
    return F, M


def errors(cameras, truth, centre):
    """(largest rotation error relative to camera `centre` in degrees, largest focal error in per cent) of cameras [(focal, R)]"""
    rot = max(angle_deg(np.asarray(cameras[centre][1], np.float64).T @ np.asarray(R, np.float64), truth["R"][centre].T @ Rt)
              for (_, R), Rt in zip(cameras, truth["R"]))
    foc = max(abs(f - ft) / ft * 100.0 for (f, _), ft in zip(cameras, truth["focals"]))
    return rot, foc


CASES = sorted(RIGS) + ["texture"]
_MEASURED = {}


def measure(name):
    """the contract (tests/numpy_cameras.py) on a case -> (indices, cameras, info), and what profiles/cameras.json records of it"""
    from tests import numpy_cameras as NC

    if name not in _MEASURED:
        feats, matches, truth = texture_case() if name == "texture" else rig(name)
        idx, cams, info = NC.register(feats, matches)
        _, centre = NC.spanning_tree(matches, len(feats))
        rot, foc = errors([(c["focal"], c["R"]) for c in cams], truth, centre)
        _MEASURED[name] = ((idx, cams, info), {"cameras": len(feats), "edges": info["edges"], "matches": info["matches"],
                                               "evaluations": info["evaluations"], "accepted": info["accepted"],
                                               "rotation_error_deg": round(rot, 4), "focal_error_percent": round(foc, 4)})
    return _MEASURED[name]


def parameters_agree(got, want, centre, rel=1e-9):
    """(n, 4) rows focal, Rodrigues vector.  Every focal within rel of its own size.  The vectors themselves are not comparable: a turn
    common to all cameras changes no residual (the gauge; only the damping holds it, and the solver divides it out by R_centre^-1), so a
    difference of one rounding at the start stays as a common turn of that size.  What is compared is what the gauge leaves: every
    camera's turn relative to the centre camera, whose difference in angle must be within rel of the turn's own angle — no absolute
    allowance."""
    from tests import numpy_cameras as NC

    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if not (np.abs(got[:, 0] - want[:, 0]) <= rel * np.abs(want[:, 0])).all():
        return False
    Rg, Rw = [NC.rodrigues(p[1:]) for p in got], [NC.rodrigues(p[1:]) for p in want]
    for i in range(len(got)):
        if i != centre:
            dg, dw = Rg[centre].T @ Rg[i], Rw[centre].T @ Rw[i]
            if not angle_deg(dg, dw) <= rel * angle_deg(np.eye(3), dw):
                return False
    return True
