"""Frames in, panorama out for scans and flat tiles on the MI355X: stitching_amd.AffineComposer.stitch on four tiles of one texture
(tests/affine_rigs.texture_tiles: a 2 x 2 grid of 320 x 240 tiles at a pitch of 0.7, turns within 2 degrees, scales within 2 %).  Its
registration equals the numpy chain tests/numpy_features.py -> tests/numpy_affine.py, recovers the planted transforms within twice the
contract's own error on this case (profiles/affine.json, measured on the CPU), and its panorama is the composition of the kept frames
with those cameras byte for byte."""
import numpy as np
import pytest

import stitching_amd as S
from tests import affine_rigs as AR
from tests import numpy_cameras as NC

pytestmark = pytest.mark.gpu


def test_affine_composer_stitch():
    imgs, truth = AR.texture_tiles()
    before = [a.copy() for a in imgs]
    composer = S.AffineComposer(finder="voronoi")
    pano = composer.stitch(imgs)
    reg = composer.registration
    assert reg["indices"] == [0, 1, 2, 3] and len(reg["cameras"]) == 4 and reg["info"]["accepted"] >= 1
    # the numpy chain: detector, affine matcher, affine registration (MEDIUM is the tiles' own size: 0.08 megapixels)
    (widx, wcams, winfo), rec = AR.measure("texture")
    assert reg["indices"] == list(widx)
    for key in ("edges", "matches", "evaluations", "accepted"):
        assert reg["info"][key] == winfo[key], (key, reg["info"][key], winfo[key])
    extent = max(np.abs(np.asarray(c["R"], np.float64)[:2, 2]).max() for c in wcams) + max(AR.TILE)
    for cam, want in zip(reg["cameras"], wcams):
        assert cam.R.dtype == np.float32 and (cam.focal, cam.aspect, cam.ppx, cam.ppy) == (1.0, 1.0, 0.0, 0.0)
        assert np.allclose(cam.R[:2, :2], want["R"][:2, :2], rtol=0, atol=1e-9), (cam.R, want["R"])
        assert np.allclose(cam.R[:2, 2], want["R"][:2, 2], rtol=0, atol=1e-9 * extent), (cam.R, want["R"])
    _, centre = NC.spanning_tree(AR.texture_case()[1], 4)
    err = AR.corner_error([c.R for c in reg["cameras"]], truth, centre)
    print(f"stitch: corner error {err:.4f} px (contract {rec['corner_error_px']}, bound {2.0 * AR.recorded('texture')}), "
          f"{reg['info']['evaluations']} evaluations")
    assert err <= 2.0 * AR.recorded("texture")
    # the panorama is the composition of the kept frames with the registration's cameras
    out = np.asarray(pano.numpy())
    again = np.asarray(S.AffineComposer(finder="voronoi").compose([imgs[i] for i in reg["indices"]], reg["cameras"]).numpy())
    assert out.shape == again.shape and np.array_equal(out, again)
    assert out.ndim == 3 and out.shape[2] == 3 and out.shape[1] > AR.TILE[0] and out.shape[0] > AR.TILE[1] and out.any()
    assert all(np.array_equal(a, b) for a, b in zip(imgs, before))
    # the default models of the parent class are what they were: its stitch() registers rotations
    assert S.Composer.REGISTRATION_MODELS == ("homography", "rotation")
