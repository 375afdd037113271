"""CPU: the reference marginal covariances of ba_covariance (tests/covariance_reference.py) against the dense inverse of the
free Gauss-Newton matrix, and the host-side pieces of the feature that need no GPU."""
import numpy as np
import pytest

from bundle_adjustment_amd import hip_backend
from tests import covariance_reference as cr
from tests.held_reference import Reduced
from tests.schur_cases import bal_case, pinhole_case


def _gauge_fixed(case, rng=None):
    """fixed_cam 0 plus t[0] of camera 1 (the scale); with rng, random extra masks and held points on top."""
    m = np.zeros(case.n_cams, np.uint16)
    if rng is not None:
        case.hold(rng)
        m = case.cam_mask.copy()
        m[0] = 0
    m[1] |= np.uint16(1 << 3)
    case.cam_mask = m
    return case


def _reduced(case):
    return Reduced(case.cams, case.pts, case.ci, case.pi, case.uv, case.K4, case.fixed, case.cam_mask, case.pt_held)


@pytest.mark.parametrize("model", ["pinhole", "bal"])
@pytest.mark.parametrize("loss", ["linear", "huber"])
@pytest.mark.parametrize("held", [False, True])
def test_schur_formula_equals_the_dense_inverse(model, loss, held):
    rng = np.random.default_rng(3)
    case = (pinhole_case if model == "pinhole" else bal_case)(6, 60, 4, seed=11)
    _gauge_fixed(case, rng if held else None)
    red = _reduced(case)
    ref = cr.schur_covariance(red, case.cams, case.pts, loss)
    assert not ref["onecam"].any()
    H, _ = cr.dense_information(red, case.cams, case.pts, loss)
    cam_full, pt_blocks = cr.embed(red, np.linalg.inv(H))
    scale = np.abs(cam_full).max()
    np.testing.assert_allclose(ref["full"], cam_full, rtol=0, atol=1e-7 * scale)
    free_pts = ~red.held_pt
    np.testing.assert_allclose(ref["points"][free_pts], pt_blocks[free_pts], rtol=0, atol=1e-7 * np.abs(pt_blocks).max())
    assert np.all(ref["points"][red.held_pt] == 0.0)
    held_cols = red.held_cam.ravel()
    assert np.all(ref["full"][held_cols] == 0.0) and np.all(ref["full"][:, held_cols] == 0.0)


@pytest.mark.parametrize("model", ["pinhole", "bal"])
def test_one_camera_points_match_the_pseudo_inverse(model):
    """Extra points seen by one camera only (one observation, or two by the same camera): H is singular in their depth
    only, so the camera blocks of pinv(H) are the reference's, which leaves those points out of S."""
    case = (pinhole_case if model == "pinhole" else bal_case)(5, 50, 4, seed=5)
    _gauge_fixed(case)
    rng = np.random.default_rng(0)
    new_pts, ci, pi, uv = [], list(case.ci), list(case.pi), list(case.uv)
    for k, (c, nobs) in enumerate([(2, 1), (3, 2)]):
        o = int(np.nonzero(case.ci == c)[0][0])
        p = case.pts[case.pi[o]] + rng.normal(0, 0.05, 3)
        new_pts.append(p)
        for _ in range(nobs):
            ci.append(c); pi.append(len(case.pts) + k); uv.append(case.uv[o] + rng.normal(0, 1.0, 2))
    case.pts = np.concatenate([case.pts, np.array(new_pts)])
    case.ci, case.pi, case.uv = np.array(ci, np.int32), np.array(pi, np.int32), np.array(uv)
    red = _reduced(case)
    ref = cr.schur_covariance(red, case.cams, case.pts, "linear")
    assert ref["onecam"][-2:].all() and not ref["onecam"][:-2].any()
    assert np.isnan(ref["points"][-2:]).all()
    H, _ = cr.dense_information(red, case.cams, case.pts, "linear")
    ev, vec = np.linalg.eigh(H)
    null = vec[:, ev < ev[-1] * 1e-13]
    assert null.shape[1] == 2
    ncam_free = int(red.free[:red.ncol].sum())
    assert np.abs(null[:ncam_free]).max() < 1e-9          # the null space lies in point coordinates only
    cam_full, _ = cr.embed(red, np.linalg.pinv(H, rcond=1e-13, hermitian=True))
    np.testing.assert_allclose(ref["full"], cam_full, rtol=0, atol=1e-7 * np.abs(cam_full).max())


def test_covariance_needs_a_second_fixed_keyframe():
    from bundle_adjustment_amd import BundleAdjuster
    with pytest.raises(ValueError, match="fixed_keyframes"):
        BundleAdjuster(np.eye(3), covariance=True, fixed_keyframes=1)
    ba = BundleAdjuster(np.eye(3), covariance=True, fixed_keyframes=2)
    assert ba._solver is None and ba.last_covariance is None


@pytest.mark.parametrize("nb", [3, 6, 9])
def test_unpack_round_trip(nb):
    rng = np.random.default_rng(nb)
    a = rng.normal(size=(4, nb, nb))
    a = a + np.swapaxes(a, 1, 2)
    packed = hip_backend.pack_sym(a, nb)
    assert packed.shape == (4, nb * (nb + 1) // 2)
    assert np.array_equal(hip_backend.unpack_sym(packed, nb), a)
    assert np.array_equal(hip_backend.pack_sym(hip_backend.unpack_sym(packed, nb), nb), packed)
    # packed order is Hcc's: row by row of the upper triangle
    assert packed[0, 1] == a[0, 0, 1] and packed[0, nb] == a[0, 1, 1]
