"""Point rigs with a planted principal-point offset and aspect for the reprojection adjustment's tests (tests/test_reproj_contract.py,
tests/test_gpu_reproj_cameras.py) and tools/bench_cameras.py: tests/camera_rigs.point_rig with K = [[f, 0, cx], [0, f a, cy], [0, 0, 1]]
in place of diag(f, f, 1).  Features and match entries are the contracts' dicts.  Everything is computed once."""
import numpy as np

from tests import camera_rigs as CR
from tests import numpy_cameras as NC
from tests import numpy_matches as NM
from tests import numpy_reproj as NR

OFFSET, ASPECT = (12.0, -9.0), 1.02
MASKS = ("xxxxx", "x_x_x", "x____")


def point_rig(seed, n, rows=1, per_image=150, noise=0.5, size=(CR.W, CR.H), focal=700.0, step=(20.0, 35.0), jitter=3.0, max_shared=120,
              outliers=0.0, offset=OFFSET, aspect=ASPECT):
    """-> features, matches, truth {"focals", "R", "offset", "aspect"}: camera_rigs.point_rig's cameras and landmarks, the same draws
    in the same order; a landmark X in camera coordinates lands on (f X0 / X2 + cx, f a X1 / X2 + cy) + noise relative to the image
    centre, rounded to a pixel."""
    rs = np.random.RandomState(seed)
    cols = n // rows
    yaws = np.cumsum(rs.uniform(step[0], step[1], cols))
    yaws -= yaws.mean()
    Rs, focals = [], []
    for r in range(rows):
        for c in range(cols):
            Rs.append(CR.rotation(yaws[c] + (rs.uniform(-3, 3) if rows > 1 else 0.0), (r - (rows - 1) / 2.0) * 22.0 + rs.uniform(-jitter, jitter),
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
            xy = X[:, :2] / X[:, 2:3] * (f, f * aspect) + offset + rs.normal(0.0, noise, (count, 2))
        pix = np.rint(xy + (w / 2, h / 2))
        ok = (X[:, 2] > 0.1) & (pix[:, 0] >= 0) & (pix[:, 0] < w) & (pix[:, 1] >= 0) & (pix[:, 1] < h)
        ids = np.flatnonzero(ok)
        feats.append(CR._features(pix[ids], size))
        seen.append(ids)
        pts.append(NM.centred(feats[-1]))
    truth = {"focals": focals, "R": Rs, "offset": tuple(offset), "aspect": aspect}
    return feats, CR.entries_from_tracks(seen, pts, rs, max_shared=max_shared, outliers=outliers), truth


RIGS = {"row5": (21, 5, 1), "row8": (22, 8, 1), "two_rows6": (23, 6, 2)}
_CACHE, _MEASURED = {}, {}


def rig(name):
    if name not in _CACHE:
        _CACHE[name] = point_rig(*RIGS[name])
    return _CACHE[name]


def truth_parameters(truth):
    """(n, 7) rows focal, cx, cy, aspect, Rodrigues vector of the planted cameras"""
    return np.array([[f, truth["offset"][0], truth["offset"][1], truth["aspect"]] + list(NC.rodrigues_vector(R))
                     for f, R in zip(truth["focals"], truth["R"])], np.float64)


def start_cameras(name):
    """[(focal, R, ppx, ppy, aspect)] to start from: 1.03 x the planted focal, the principal point at the image centre, aspect 1, every
    rotation off by a turn of up to 1 degree about a random axis"""
    feats, _, truth = rig(name)
    rs = np.random.RandomState(1000 + RIGS[name][0])
    out = []
    for f, R, feat in zip(truth["focals"], truth["R"], feats):
        axis = rs.standard_normal(3)
        turn = NC.rodrigues(axis / np.sqrt((axis * axis).sum()) * np.deg2rad(rs.uniform(0.0, 1.0)))
        w0, h0 = feat["img_size"]
        out.append((1.03 * f, R @ turn, w0 / 2, h0 / 2, 1.0))
    return out


def rms(E, matches_count):
    return float(np.sqrt(E / matches_count))


def measure(name, mask):
    """the contract (tests/numpy_reproj.py) on a rig from start_cameras under a mask -> (cameras, info), and what profiles/reproj.json
    records of it"""
    if (name, mask) not in _MEASURED:
        feats, matches, truth = rig(name)
        n = len(feats)
        cams, info = NR.adjust(feats, matches, start_cameras(name), mask)
        _, centre = NC.spanning_tree(matches, n)
        rot, foc = CR.errors([(c[0], c[1]) for c in cams], truth, centre)
        m = info["matches"]
        E_truth = float(np.sum(NR.normal_equations(feats, matches, truth_parameters(truth))[0]))
        p = info["parameters"]
        rec = {"cameras": n, "edges": info["edges"], "matches": m, "evaluations": info["evaluations"], "accepted": info["accepted"],
               "rms_start_px": round(rms(info["first_E"], m), 4), "rms_end_px": round(rms(info["last_E"], m), 4),
               "rms_truth_px": round(rms(E_truth, m), 4), "rotation_error_deg": round(rot, 4), "focal_error_percent": round(foc, 4),
               "offset_px": [[round(float(v), 3) for v in q[1:3]] for q in p], "aspect": [round(float(q[3]), 5) for q in p],
               "planted_offset_px": list(truth["offset"]), "planted_aspect": truth["aspect"]}
        _MEASURED[(name, mask)] = ((cams, info), rec, E_truth)
    return _MEASURED[(name, mask)]
