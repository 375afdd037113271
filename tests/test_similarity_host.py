"""CPU: the host side of the similarity transform -- the quaternion log map at every angle, similarity.apply against the
projections, the numpy yardstick of ba_align on known answers, compose / inverse, the ctypes structs and the option
checks that need no GPU."""
import ctypes as C
import math

import numpy as np
import pytest

from bundle_adjustment_amd import similarity
from bundle_adjustment_amd.bal import BALProblem, from_pinhole
from bundle_adjustment_amd.rotations import matrices_to_rvecs, rvecs_to_matrices
from bundle_adjustment_amd.synthetic import _project, bal_project, make_problem
from tests import similarity_reference as sr

ANGLES = (0.0, 1e-12, 1e-9, 1e-6, 1e-3, 1.0, math.pi - 1e-3, math.pi - 1e-5, math.pi - 1e-7, math.pi - 1e-9, math.pi)


def axes():
    rng = np.random.default_rng(3)
    out = [np.eye(3)[i] * sgn for i in range(3) for sgn in (1.0, -1.0)]
    out += [np.array([1.0, 1.0, 0.0]) / math.sqrt(2.0), np.array([1.0, -1.0, 1.0]) / math.sqrt(3.0)]
    for _ in range(8):
        v = rng.normal(size=3)
        out.append(v / np.linalg.norm(v))
    return out


def test_log_map_round_trip_at_every_angle():
    """R(rvec(Q)) - Q <= 1e-13 from 0 to pi, for the package's log map and the yardstick's; |rvec| <= pi."""
    worst = 0.0
    for th in ANGLES:
        for k in axes():
            Q = sr.rodrigues(k * th)
            for rv in (sr.log_map(Q), similarity._log_map(Q[None])[0]):
                assert np.linalg.norm(rv) <= math.pi + 1e-12
                worst = max(worst, np.abs(sr.rodrigues(rv) - Q).max(), np.abs(rvecs_to_matrices(rv[None])[0] - Q).max())
    print(f"log map: largest round-trip error {worst:.3e}")
    assert worst <= 1e-13


def test_cv2_style_log_map_is_not_good_enough():
    """What the quaternion form is for: rotations.matrices_to_rvecs (cv2.Rodrigues' branches) loses 1e-6 below 1e-5 rad."""
    Q = sr.rodrigues(np.array([0.0, 0.0, 1e-6]))
    assert np.abs(rvecs_to_matrices(matrices_to_rvecs(Q[None]))[0] - Q).max() > 1e-7
    assert np.abs(rvecs_to_matrices(similarity._log_map(Q[None]))[0] - Q).max() <= 1e-15


def sims():
    rng = np.random.default_rng(9)
    t1 = rng.normal(size=3)
    return [(1.0, np.eye(3), np.zeros(3)), (37.5, sr.random_rotation(rng), 100.0 * t1 / np.linalg.norm(t1)),
            (0.02, sr.random_rotation(rng, math.pi - 1e-4), np.array([-40.0, 3.0, 60.0]))]


@pytest.mark.parametrize("k", range(3))
def test_apply_keeps_the_residuals(k):
    """similarity.apply moves no pinhole / BAL projection by more than 1e-9 px for |t| <= 100, and agrees with the
    yardstick's transform."""
    s, R, t = sims()[k]
    prob = make_problem(12, 150, 4, seed=2, K4=np.array([900.0, 900.0, 640.0, 360.0]))
    uv0 = _project(prob.cams, prob.pts, prob.cam_idx, prob.pt_idx, prob.K4)[0]
    moved = similarity.apply(prob, s, R, t)
    uv1 = _project(moved.cams, moved.pts, prob.cam_idx, prob.pt_idx, prob.K4)[0]
    assert np.abs(uv1 - uv0).max() <= 1e-9
    cams_y, pts_y, _ = sr.transform(prob.cams, prob.pts, s, R, t)
    assert np.abs(moved.pts - pts_y).max() <= 1e-13 * max(1.0, np.abs(pts_y).max())
    assert np.abs(moved.cams - cams_y).max() <= 1e-13 * max(1.0, np.abs(cams_y).max())
    b = from_pinhole(prob)
    b.cams[:, 6:9] = (880.0, -0.03, 0.002)
    bm = similarity.apply(b, s, R, t)
    assert isinstance(bm, BALProblem) and np.array_equal(bm.cams[:, 6:9], b.cams[:, 6:9])
    assert np.abs(bal_project(bm.cams, bm.pts, b.cam_idx, b.pt_idx) - bal_project(b.cams, b.pts, b.cam_idx, b.pt_idx)).max() <= 1e-9
    assert np.abs(similarity._centres(moved.cams) - (s * similarity._centres(prob.cams) @ R.T + t)).max() <= 1e-12 * max(1.0, s * 20 + 100)


def test_apply_refuses_priors_and_bad_similarities():
    prob = make_problem(4, 30, 3, seed=1)
    with pytest.raises(ValueError):
        similarity.apply(prob, 0.0)
    with pytest.raises(ValueError):
        similarity.apply(prob, 1.0, np.diag([1.0, 1.0, -1.0]))
    with pytest.raises(ValueError):
        similarity.apply(prob, 1.0, 1.001 * np.eye(3))
    prob.pt_prior = {0: (np.zeros(3), np.eye(3))}
    with pytest.raises(ValueError, match="priors"):
        similarity.apply(prob, 2.0)


def test_compose_and_inverse():
    for x in sims():
        s, R, t = similarity.compose(similarity.inverse(x), x)
        assert abs(s - 1.0) <= 1e-15 and np.abs(R - np.eye(3)).max() <= 1e-15 and np.abs(t).max() <= 1e-12
    a, b = sims()[1], sims()[2]
    X = np.random.default_rng(0).normal(size=(5, 3))
    s, R, t = similarity.compose(b, a)
    want = b[0] * (a[0] * X @ a[1].T + a[2]) @ b[1].T + b[2]
    assert np.abs(s * X @ R.T + t - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("with_scale", [True, False])
def test_yardstick_recovers_a_known_similarity(with_scale):
    rng = np.random.default_rng(4)
    a = rng.normal(size=(40, 3)) * (3.0, 2.0, 5.0)
    s0, R0, t0 = (12.5 if with_scale else 1.0), sr.random_rotation(rng), np.array([4.1e5, 5.2e6, 310.0])
    b = s0 * a @ R0.T + t0
    for loss, iters in (("linear", 0), ("huber", 10)):
        out = sr.align(a, b, loss=loss, iters=iters, f_scale=0.1, with_scale=with_scale)
        assert out["status"] == sr.OK and out["n_used"] == 40
        assert abs(out["s"] - s0) <= 1e-9 * s0 and np.abs(out["R"] - R0).max() <= 1e-9
        assert np.abs(out["t"] - t0).max() <= 1e-9 * np.linalg.norm(t0) and out["max"] <= 1e-6


def test_yardstick_reflection_guard_statuses_and_weights():
    rng = np.random.default_rng(5)
    a = rng.normal(size=(30, 3))
    out = sr.align(a, a * (1.0, 1.0, -1.0))                      # mirrored references: still a proper rotation
    assert out["status"] == sr.OK and abs(np.linalg.det(out["R"]) - 1.0) <= 1e-12
    assert sr.align(a[:2], a[:2])["status"] == sr.TOO_FEW
    line = np.outer(np.arange(9.0), (1.0, 2.0, 3.0))
    assert sr.align(line, line)["status"] == sr.DEGENERATE
    assert sr.align(np.ones((8, 3)), a[:8])["status"] == sr.DEGENERATE
    flat = a * (1.0, 1.0, 0.0)
    out = sr.align(flat, 2.0 * flat @ sr.rodrigues(np.array([0.3, -0.2, 0.9])).T + 1.0)
    assert out["status"] == sr.OK and abs(np.linalg.det(out["R"]) - 1.0) <= 1e-12 and abs(out["s"] - 2.0) <= 1e-12
    w = np.ones(30)
    w[::3] = 0.0
    b = 3.0 * a + 1.0
    b[::3] = np.nan
    out = sr.align(a, b, w)
    assert out["status"] == sr.OK and out["n_used"] == 20 and np.isnan(out["err"][::3]).all() and abs(out["s"] - 3.0) <= 1e-12
    with pytest.raises(ValueError):
        sr.align(a, b, -w)


def test_struct_sizes_and_defaults():
    from bundle_adjustment_amd import hip_backend as hb
    assert C.sizeof(hb.BASimilarity) == 104 and C.sizeof(hb.BAAlignOptions) == 24 and C.sizeof(hb.BAAlignResult) == 128
    assert hb.ALIGN_STATUS == {"ok": 0, "too_few": 1, "degenerate": 2}
    import __graft_entry__ as g
    g.build()
    lib = hb.load_library()
    o = hb.BAAlignOptions()
    assert lib.ba_default_align_options(C.byref(o)) == 0
    assert (o.loss, o.iters, o.f_scale, o.with_scale, o.apply) == (0, 10, 1.0, 1, 0)
    assert lib.ba_default_align_options(None) == -1


def test_option_validation_without_a_gpu():
    """What can be checked without a device: NULL arguments are refused by the library, an unknown loss name is a ValueError
    (f_scale, iters and the weights are validated behind the state check: tests/test_gpu_similarity.py)."""
    from bundle_adjustment_amd import hip_backend as hb
    import __graft_entry__ as g
    g.build()
    lib = hb.load_library()
    res, sim, o = hb.BAAlignResult(), hb.BASimilarity(), hb.BAAlignOptions()
    assert lib.ba_transform(None, C.byref(sim)) == -1 and b"null" in lib.ba_last_error()
    assert lib.ba_align(None, C.byref(o), None, None, None, None, C.byref(res), None, None) == -1
    assert lib.ba_get_centres(None, None) == -1
    s = hb.Solver.__new__(hb.Solver)              # no handle: the name check comes before the library call
    s._lib, s._h, s.n_cams, s.n_pts = lib, None, 3, 4
    with pytest.raises(ValueError, match="unknown loss"):
        s.align(cam_ref=np.zeros((3, 3)), loss="tukey")


def test_grid_border_scenes_notice_their_last_rows():
    """The scenes of tests/similarity_cases.py: their block counts are the ones named, and the yardstick with the last 40
    (heavy) rows dropped differs from the full one by more than 100 x the device tests' tolerance in s or t -- a fold that
    lost the last partial row, or a grid-stride loop that lost its second trip, would be seen."""
    from bundle_adjustment_amd.hip_backend import ALIGN_MAX_BLOCKS
    from tests import similarity_cases as sc
    assert [sc.partial_rows(nn) for nn in sc.BORDER_COUNTS] == [(64, 1), (65, 1), (ALIGN_MAX_BLOCKS, 1), (ALIGN_MAX_BLOCKS, 2)]
    for nn in sc.BORDER_COUNTS:
        _, a, b, w, (s0, R0, t0) = sc.border_scene(nn)
        assert a.shape == (nn, 3) and (w[-sc.HEAVY:] == sc.HEAVY_WEIGHT).all() and (w[:-sc.HEAVY] == 1.0).all()
        for loss, iters in (("linear", 0), ("cauchy", 5)):
            full = sr.align(a, b, w, loss=loss, f_scale=0.15, iters=iters)
            cut = sr.align(a[:-sc.HEAVY], b[:-sc.HEAVY], w[:-sc.HEAVY], loss=loss, f_scale=0.15, iters=iters)
            assert full["status"] == cut["status"] == 0 and full["n_used"] == nn
            d_s = abs(full["s"] - cut["s"]) / full["s"]
            d_t = np.abs(full["t"] - cut["t"]).max() / max(1.0, float(np.linalg.norm(t0)))
            print(f"{nn} correspondences, {loss}: without the last {sc.HEAVY} rows s moves by {d_s:.2e}, t by {d_t:.2e}")
            assert max(d_s, d_t) > 100.0 * sc.TOL
            assert abs(full["s"] - s0) / s0 < 1e-2                     # (the fit is the planted similarity, to the noise of the heavy rows)
