"""CPU: the yardstick of the RANSAC resection tests (tests/ransac_reference.py) against planted truth, and the Python surface
of ba_resect_ransac that needs no device: option names, the options struct's layout, filter_observations."""
import ctypes as C

import numpy as np
import pytest

from bundle_adjustment_amd import hip_backend
from bundle_adjustment_amd.bal import from_pinhole
from bundle_adjustment_amd.synthetic import make_problem
from bundle_adjustment_amd.triangulation import filter_observations
from tests import ransac_reference as R
from tests import resect_reference as rr


def test_reference_p3p_reproduces_every_observation():
    """8 cameras x 250 seeds of single random triples, noise-free unrounded pixels: the best solution of every triple
    reproduces all of the camera's observations within 1e-3 px (measured: 2000 of 2000, and 2000 of 2000 at 1e-6 px)."""
    base, cams_true, pts_true = make_problem(8, 400, 4, K4=R.K4, return_truth=True)
    prob, truth = R.in_model("pinhole", cams_true, pts_true, base.cam_idx, base.pt_idx, base.cams, pts_true,
                             np.random.default_rng(0), sigma=0.0, rounded=False)
    worst, tight = 0.0, 0
    for c in range(8):
        o = rr.obs_of(prob, c)
        y = R.unit_rays(o.bearings()[0], False)
        for seed in range(250):
            idx = list(R.sample3(seed, c, 0, len(o.uv)))
            best = np.inf
            for Rm, t in R.p3p(y[idx], o.X[idx]):
                e2, depth = R.errors_at(o, Rm, t)
                if (depth > 0.0).all():
                    best = min(best, float(np.sqrt(e2.max())))
            worst = max(worst, best)
            tight += best <= 1e-6
    print(f"worst best-solution error over 2000 triples {worst:.3e} px; {tight} of 2000 within 1e-6 px")
    assert worst <= 1e-3


@pytest.mark.parametrize("share", [0.3, 0.5])
def test_reference_ransac_recovers_the_planted_inliers(share):
    prob, truth, planted, yard = R.outlier_problem("pinhole", share)
    ref = R.resect_ransac(prob, n_hyp=256)
    d = rr.pose_diff(ref["poses"], yard)
    print(f"{share}: reference RANSAC + LO against the yardstick {d.max():.3e}")
    assert (ref["status"] == R.OK).all()
    assert np.array_equal(ref["obs_inlier"], ~planted)
    assert np.array_equal(ref["n_inliers"], np.bincount(prob.cam_idx[~planted], minlength=prob.n_cams))
    assert d.max() <= 1e-12


def test_generator_draws_distinct_indices_and_depends_on_every_argument():
    seen = set()
    for n in (3, 4, 5, 64, 1000):
        for h in range(200):
            i = R.sample3(7, 2, h, n)
            assert len(set(i)) == 3 and min(i) >= 0 and max(i) < n
            seen.add((n,) + i)
    assert R.sample3(0, 0, 0, 1000) != R.sample3(1, 0, 0, 1000) != R.sample3(1, 1, 0, 1000) != R.sample3(1, 1, 1, 1000)
    assert {R.sample3(0, 0, h, 3) for h in range(64)} == {(a, b, c) for a in range(3) for b in range(3) for c in range(3)
                                                          if len({a, b, c}) == 3}
    assert R.mix64(0) == 0 and R.mix64(R.GOLDEN) == 0xE220A8397B1DCDAF      # splitmix64's first output from state 0


def test_python_surface():
    # struct ba_ransac_options of include/ba_hip.h: int32 x 2, uint64, double, int32 x 2, double, int32 x 2, double x 2
    assert C.sizeof(hip_backend.BARansacOptions) == 64
    off = {k: getattr(hip_backend.BARansacOptions, k).offset for k, _ in hip_backend.BARansacOptions._fields_}
    assert off == dict(n_hyp=0, lo_rounds=4, seed=8, max_reproj_px=16, loss=24, refine_iters=28, f_scale=32, min_inliers=40,
                       write_cams=44, max_rms_px=48, min_depth=56)
    assert "ba_resect_ransac" in hip_backend.SYMBOLS and "ba_default_ransac_options" in hip_backend.SYMBOLS
    assert hip_backend.K_RESECT_RANSAC == 15

    class Lib:                                   # ransac_options needs the defaults only
        @staticmethod
        def ba_default_ransac_options(ref):
            o = ref._obj
            o.n_hyp, o.lo_rounds, o.max_reproj_px, o.refine_iters, o.f_scale, o.min_inliers = 256, 2, 4.0, 20, 1.0, 6
            return 0
    s = hip_backend.Solver.__new__(hip_backend.Solver)
    s._lib = Lib()
    o = s.ransac_options(loss="cauchy", n_hyp=64, seed=2 ** 63 + 5)
    assert (o.loss, o.n_hyp, o.seed, o.lo_rounds) == (hip_backend.loss_code("cauchy"), 64, 2 ** 63 + 5, 2)
    with pytest.raises(ValueError):
        s.ransac_options(loss="nope")
    with pytest.raises(TypeError):
        s.ransac_options(no_such_option=1)


@pytest.mark.parametrize("model", ["pinhole", "bal"])
def test_filter_observations_keeps_order_and_indices(model):
    prob = make_problem(5, 60, 3, K4=R.K4, seed=4)
    if model == "bal":
        prob = from_pinhole(prob)
    rng = np.random.default_rng(1)
    keep = rng.random(prob.n_obs) < 0.7
    new, old = filter_observations(prob, keep)
    assert type(new) is type(prob) and new.n_obs == keep.sum() and np.array_equal(old, np.nonzero(keep)[0])
    assert np.array_equal(new.cam_idx, prob.cam_idx[old]) and np.array_equal(new.pt_idx, prob.pt_idx[old])
    assert np.array_equal(new.uv, prob.uv[old])
    assert new.n_cams == prob.n_cams and new.n_pts == prob.n_pts and new.cams is prob.cams and new.pts is prob.pts
    with pytest.raises(ValueError):
        filter_observations(prob, keep[:-1])
    with pytest.raises(ValueError):
        filter_observations(prob, keep.astype(np.uint8))
