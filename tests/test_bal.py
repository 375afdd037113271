"""Row f2: BAL text reader / writer and the 9-parameter BAL camera.
CPU: exact round trip through the text format, parser errors, the oracle's analytic 2x9 / 2x3 blocks against central
finite differences, the pinhole conversion.  GPU: the BAL residual kernel (ba_residuals_bal) against the oracle,
<= 1e-9 px, and a BAL problem with shared focal length / no distortion solved through the reference's model."""
import os

import numpy as np
import pytest

from bundle_adjustment_amd.bal import BALProblem, from_pinhole, read_bal, to_pinhole, write_bal
from oracle import ba_oracle as o
from tests.helpers import GOLDEN
from tests.lm_trace import check_self_consistent

TINY = os.path.join(GOLDEN, "tiny_bal.txt")


def test_reader_parses_the_committed_fixture_and_round_trips_exactly(tmp_path):
    p = read_bal(TINY)
    assert (p.n_cams, p.n_pts, p.n_obs) == (6, 40, 160)
    assert p.cams.shape == (6, 9) and p.uv.shape == (160, 2) and p.cam_idx.dtype == np.int32
    r = o.bal_residuals(p.cams, p.pts, p.cam_idx, p.pt_idx, p.uv)
    assert 0.3 < np.sqrt((r * r).sum() / p.n_obs) < 1.2          # the fixture's pixels carry 0.5 px noise
    out = tmp_path / "again.txt"
    write_bal(out, p)
    q = read_bal(out)
    for a, b in ((p.cams, q.cams), (p.pts, q.pts), (p.cam_idx, q.cam_idx), (p.pt_idx, q.pt_idx), (p.uv, q.uv)):
        np.testing.assert_array_equal(a, b)
    import gzip
    with open(out, "rb") as f, gzip.open(str(out) + ".gz", "wb") as g:
        g.write(f.read())
    np.testing.assert_array_equal(read_bal(str(out) + ".gz").cams, p.cams)


def test_reader_rejects_malformed_files(tmp_path):
    bad = tmp_path / "bad.txt"
    bad.write_text("2 1 1\n0 0 1.0 2.0\n" + "0.0\n" * 10)                  # too few numbers
    with pytest.raises(ValueError, match="expected"):
        read_bal(bad)
    bad.write_text("1 1 1\n0.5 0 1.0 2.0\n" + "0.0\n" * 12)                # fractional index
    with pytest.raises(ValueError, match="non-integer"):
        read_bal(bad)
    bad.write_text("1 1 1\n3 0 1.0 2.0\n" + "0.0\n" * 12)                  # camera index out of range
    with pytest.raises(ValueError, match="out of range"):
        read_bal(bad)


def test_bal_analytic_blocks_match_finite_differences():
    p = read_bal(TINY)
    Jc, Jp = o.bal_jacobian_blocks(p.cams, p.pts, p.cam_idx, p.pt_idx)
    h = 1e-6
    for k in range(9):
        d = np.zeros_like(p.cams); d[:, k] = h
        fd = (o.bal_residuals(p.cams + d, p.pts, p.cam_idx, p.pt_idx, p.uv)
              - o.bal_residuals(p.cams - d, p.pts, p.cam_idx, p.pt_idx, p.uv)) / (2 * h)
        assert np.abs(fd - Jc[:, :, k]).max() <= 1e-6 * max(1.0, np.abs(Jc[:, :, k]).max()), k
    for k in range(3):
        d = np.zeros_like(p.pts); d[:, k] = h
        fd = (o.bal_residuals(p.cams, p.pts + d, p.cam_idx, p.pt_idx, p.uv)
              - o.bal_residuals(p.cams, p.pts - d, p.cam_idx, p.pt_idx, p.uv)) / (2 * h)
        assert np.abs(fd - Jp[:, :, k]).max() <= 1e-6 * max(1.0, np.abs(Jp[:, :, k]).max()), k


def test_pinhole_conversion_keeps_every_residual():
    p = read_bal(TINY)
    cams = p.cams.copy()
    cams[:, 6], cams[:, 7:] = 820.0, 0.0                                    # one focal length, no distortion
    q = BALProblem(cams, p.pts, p.cam_idx, p.pt_idx, p.uv)
    pin = to_pinhole(q)
    r_bal = o.bal_residuals(q.cams, q.pts, q.cam_idx, q.pt_idx, q.uv)
    r_pin = o.residuals(pin.cams, pin.pts, pin.cam_idx, pin.pt_idx, pin.uv, pin.K4)
    assert np.abs(r_bal - r_pin).max() <= 1e-8          # (one rotation matrix -> vector -> matrix round trip)
    back = from_pinhole(pin)
    assert np.abs(o.bal_residuals(back.cams, back.pts, back.cam_idx, back.pt_idx, back.uv) - r_bal).max() <= 1e-8
    with pytest.raises(ValueError):
        to_pinhole(p)                                                       # distinct f, non-zero k1 / k2


@pytest.mark.gpu
def test_device_bal_residuals_match_the_oracle():
    from bundle_adjustment_amd import hip_backend
    p = read_bal(TINY)
    with hip_backend.Solver(0) as s:
        r, sse, cost = s.residuals_bal(p, "huber")
        ref = o.bal_residuals(p.cams, p.pts, p.cam_idx, p.pt_idx, p.uv)
        assert np.abs(r - ref).max() <= 1e-9
        assert abs(sse - float((ref * ref).sum())) <= 1e-10 * sse
        assert abs(cost - o.robust_cost(ref, "huber")) <= 1e-10 * cost
        # a larger synthetic problem in the BAL convention
        rng = np.random.default_rng(5)
        big = BALProblem(np.tile(p.cams, (40, 1)) + rng.normal(0, 1e-3, (240, 9)), np.tile(p.pts, (50, 1)) + rng.normal(0, 0.01, (2000, 3)),
                         rng.integers(0, 240, 30000).astype(np.int32), rng.integers(0, 2000, 30000).astype(np.int32),
                         rng.normal(0, 100, (30000, 2)))
        r, sse, _ = s.residuals_bal(big, "linear")
        assert np.abs(r - o.bal_residuals(big.cams, big.pts, big.cam_idx, big.pt_idx, big.uv)).max() <= 1e-9 * max(1.0, np.abs(r).max())


@pytest.mark.gpu
def test_undistorted_bal_problem_is_adjusted_through_the_reference_model():
    """A BAL file whose cameras share f and have k1 = k2 = 0 converts to the reference's pinhole (negative fy for BAL's
    axis convention) and goes through the LM / Schur / PCG solver; the BAL residuals of the result drop to the noise."""
    from bundle_adjustment_amd import hip_backend
    p = read_bal(TINY)
    cams = p.cams.copy()
    cams[:, 6], cams[:, 7:] = 820.0, 0.0
    truth = BALProblem(cams, p.pts, p.cam_idx, p.pt_idx, np.zeros_like(p.uv))
    uv = -o.bal_residuals(truth.cams, truth.pts, truth.cam_idx, truth.pt_idx, truth.uv) + np.random.default_rng(1).normal(0, 0.3, p.uv.shape)
    rng = np.random.default_rng(2)
    start = BALProblem(cams + np.concatenate([rng.normal(0, 2e-3, (6, 6)), np.zeros((6, 3))], axis=1) * (np.arange(6)[:, None] > 0),
                       p.pts + rng.normal(0, 0.03, p.pts.shape), p.cam_idx, p.pt_idx, uv)
    pin = to_pinhole(start)
    with hip_backend.Solver(0) as s:
        s.set_problem(pin)
        out = s.solve(loss="linear", max_iters=40, ftol=1e-12, xtol=1e-12, gtol=0.0)
        c6, pts = s.get_params()
        assert out["final_sse"] < 0.05 * out["initial_sse"]
        done = from_pinhole(type(pin)(c6, pts, pin.cam_idx, pin.pt_idx, pin.uv, pin.K4, 0))
        r = o.bal_residuals(done.cams, done.pts, done.cam_idx, done.pt_idx, done.uv)
        assert abs(float((r * r).sum()) - out["final_sse"]) <= 1e-8 * out["final_sse"]
        assert np.sqrt((r * r).sum() / start.n_obs) < 0.45


def _perturbed(p, seed, pose=1e-3, pt=0.02, focal=0.01):
    rng = np.random.default_rng(seed)
    cams = p.cams.copy()
    cams[:, :6] += rng.normal(0, pose, (p.n_cams, 6))
    cams[:, 6] *= 1.0 + focal * rng.normal(size=p.n_cams)
    return BALProblem(cams, p.pts + rng.normal(0, pt, p.pts.shape), p.cam_idx, p.pt_idx, p.uv)


def _synthetic_bal(n_cams, n_pts, k, seed, return_truth=False):
    """A BAL-convention problem with distinct (f, k1, k2) per camera, pixel noise 0.5, and a perturbed start."""
    rng = np.random.default_rng(seed)
    rvec = rng.normal(0, 0.05, (n_cams, 3))
    centre = np.stack([np.linspace(0, 0.4 * n_cams, n_cams), 0.1 * rng.normal(size=n_cams), 0.1 * rng.normal(size=n_cams)], 1)
    R = o.rodrigues_batch(rvec)
    t = -np.einsum("nij,nj->ni", R, centre)
    cams = np.concatenate([rvec, t, (800.0 + 40.0 * rng.normal(size=n_cams))[:, None], (-0.05 + 0.02 * rng.normal(size=n_cams))[:, None],
                           (0.01 * rng.normal(size=n_cams))[:, None]], axis=1)
    pts = np.stack([rng.uniform(-2, 0.4 * n_cams + 2, n_pts), rng.uniform(-1.5, 1.5, n_pts), rng.uniform(-14, -6, n_pts)], 1)
    # every point is seen by k of the 2k cameras nearest to it along the track (a camera far down the track would see it at a
    # grazing angle, where the radial polynomial is meaningless)
    near = np.argsort(np.abs(pts[:, :1] - centre[None, :, 0]), axis=1)[:, :min(2 * k, n_cams)]
    cam_idx = np.concatenate([np.sort(rng.choice(near[j], size=k, replace=False)) for j in range(n_pts)]).astype(np.int32)
    pt_idx = np.repeat(np.arange(n_pts, dtype=np.int32), k)
    proj = -o.bal_residuals(cams, pts, cam_idx, pt_idx, np.zeros((len(cam_idx), 2)))
    start = _perturbed(BALProblem(cams, pts, cam_idx, pt_idx, proj + rng.normal(0, 0.5, proj.shape)), seed + 1)
    return (start, cams) if return_truth else start


def test_oracle_bal_lm_dense_and_pcg_agree():
    """CPU: oracle.lm_solve(model='bal') -- the checker of ba_solve_bal -- with the explicit 9-block reduced system solved
    exactly against the matrix-free operator with PCG driven to round-off."""
    p = _perturbed(read_bal(TINY), 3)
    kw = dict(fixed_cam=-1, loss="huber", max_iters=6, ftol=0.0, xtol=0.0, gtol=0.0, model="bal", precond="jacobi")
    a = o.lm_solve(p.cams, p.pts, p.cam_idx, p.pt_idx, p.uv, None, linear_solver="dense", **kw)
    b = o.lm_solve(p.cams, p.pts, p.cam_idx, p.pt_idx, p.uv, None, pcg_tol=1e-13, pcg_max_iters=5000, pcg_model_tol=0.0, **kw)
    assert a["cost"] < 0.1 * a["cost0"]
    for ha, hb in zip(a["history"], b["history"]):
        assert abs(ha["cost_new"] - hb["cost_new"]) <= 1e-8 * hb["cost_new"]


@pytest.mark.gpu
@pytest.mark.parametrize("loss,fixed", [("linear", -1), ("huber", 2)])
def test_device_bal_linearisation_matches_the_oracle_blocks(loss, fixed):
    """ba_linearize_bal (2x9 camera blocks, K2 of row f2) against oracle.bal_normal_equations, whose blocks are tested
    against central differences above."""
    from bundle_adjustment_amd import hip_backend
    p = _synthetic_bal(12, 300, 4, seed=4)
    ne = o.bal_normal_equations(p.cams, p.pts, p.cam_idx, p.pt_idx, p.uv, fixed, loss)
    iu9, iu3 = np.triu_indices(9), np.triu_indices(3)
    with hip_backend.Solver(0) as s:
        out = s.linearize_bal(p, loss, fixed_cam=fixed)
    for dev, ref in ((out["Hcc"], ne["Hcc"][:, iu9[0], iu9[1]]), (out["bc"], ne["bc"]), (out["Hpp"], ne["Hpp"][:, iu3[0], iu3[1]]),
                     (out["bp"], ne["bp"])):
        assert np.abs(dev - ref).max() <= 1e-10 * np.abs(ref).max()
    if fixed >= 0:
        assert not out["Hcc"][fixed].any() and not out["bc"][fixed].any()


@pytest.mark.gpu
@pytest.mark.parametrize("case,precond", [("tiny_huber", "jacobi"), ("synthetic_linear_fixed", "jacobi"),
                                          ("tiny_huber", "schur_jacobi"), ("synthetic_huber_fixed", "schur_jacobi")])
def test_device_bal_solve_follows_the_oracle_lm(case, precond):
    """ba_solve_bal against oracle.lm_solve(model='bal') with the same preconditioner: every LM iteration (PCG iteration
    count, trial cost, damping, acceptance), then the adjusted cameras (f, k1, k2 included) and points."""
    from bundle_adjustment_amd import hip_backend
    if case == "tiny_huber":
        p, loss, fixed = _perturbed(read_bal(TINY), 3), "huber", -1
    else:
        p, loss, fixed = _synthetic_bal(20, 600, 5, seed=8), case.split("_")[1], 0
    iters = 8
    ref = o.lm_solve(p.cams, p.pts, p.cam_idx, p.pt_idx, p.uv, None, fixed_cam=fixed, loss=loss, max_iters=iters, ftol=0.0, xtol=0.0,
                     gtol=0.0, pcg_tol=1e-2, pcg_max_iters=300, precond=precond, model="bal")
    with hip_backend.Solver(0) as s:
        out, cams, pts = s.solve_bal(p, fixed_cam=fixed, loss=loss, max_iters=iters, ftol=0.0, xtol=0.0, gtol=0.0, pcg_tol=1e-2,
                                     pcg_max_iters=300, pcg_min_iters=0, preconditioner=precond)
        tr = s.trace()
    check_self_consistent(out, tr, dict(pcg_max_iters=300))
    assert out["iterations"] == iters == len(ref["history"])
    assert abs(out["initial_cost"] - ref["cost0"]) <= 1e-10 * ref["cost0"]
    compared = 0
    for t, h in zip(tr, ref["history"]):
        if abs(h["cost"] - h["cost_new"]) <= 1e-8 * h["cost"]:
            break                      # converged: accept / reject is decided by round-off from here on, the paths may part
        # (the PCG stopping test is a threshold on a residual norm: round-off moves the crossing by an iteration or so,
        #  a few at the long solves near the end)
        assert abs(t["pcg_iterations"] - h["pcg"]) <= max(1, 0.1 * h["pcg"]), (t, h)
        assert abs(t["cost_trial"] - h["cost_new"]) <= 1e-6 * h["cost_new"], (t, h)
        assert bool(t["accepted"]) == bool(h["rho"] > 0)
        compared += 1
    assert compared >= 3
    assert abs(out["final_cost"] - ref["cost"]) <= 1e-6 * ref["cost"]
    assert out["final_cost"] < 0.1 * out["initial_cost"]
    assert np.abs(cams - ref["cams"]).max() <= 1e-4 * np.abs(ref["cams"]).max()
    assert np.abs(pts - ref["pts"]).max() <= 1e-4 * np.abs(ref["pts"]).max()
    if fixed >= 0:
        assert np.array_equal(cams[fixed], p.cams[fixed])
    # the summary's cost is the BAL residual of what the handle returned
    r = o.bal_residuals(cams, pts, p.cam_idx, p.pt_idx, p.uv)
    assert abs(o.robust_cost(r, loss) - out["final_cost"]) <= 1e-9 * out["final_cost"]


@pytest.mark.gpu
def test_device_bal_solve_converges_on_a_larger_problem():
    """120 cameras / 6000 points / 36 k observations, poses, points and focal lengths perturbed, no camera held: the solve
    stops on the reference's kind of tolerance with the reprojection RMSE at the pixel noise (0.5 px per coordinate), and the
    summary's SSE is the oracle's BAL residual of the returned parameters."""
    from bundle_adjustment_amd import hip_backend
    p = _synthetic_bal(120, 6000, 6, seed=10)
    with hip_backend.Solver(0) as s:
        out, cams, pts = s.solve_bal(p, loss="huber", max_iters=60, ftol=1e-8, xtol=1e-10, gtol=1e-10, pcg_tol=1e-1, pcg_max_iters=300)
    assert out["status_name"] in ("ftol", "xtol", "gtol")
    assert np.sqrt(out["initial_sse"] / p.n_obs) > 2.0 and np.sqrt(out["final_sse"] / p.n_obs) < 0.7
    assert np.abs(cams[:, 6:] - p.cams[:, 6:]).max() > 0                  # f, k1, k2 were adjusted with the poses
    r = o.bal_residuals(cams, pts, p.cam_idx, p.pt_idx, p.uv)
    assert abs(float((r * r).sum()) - out["final_sse"]) <= 1e-9 * out["final_sse"]


# ---- BASELINE config 5 as stated: the BAL camera at full size (1723 cameras / 156 502 points / ~662 k observations) -------------
def _config5():
    from bundle_adjustment_amd.synthetic import make_bal_problem
    p = make_bal_problem(seed=0)
    assert p.n_cams == 1723 and p.n_pts == 156502 and p.n_obs > 600000
    assert np.ptp(p.cams[:, 6]) > 10.0 and np.abs(p.cams[:, 7]).min() > 0.0          # distinct f, non-zero k1 everywhere
    return p


@pytest.mark.gpu
def test_config5_bal_residuals_and_blocks_at_full_size():
    """ba_residuals_bal on all ~662 k observations <= 1e-9 px and ba_linearize_bal (2x9 / 2x3 blocks, Huber weights) <= 1e-9
    relative against the vectorised oracle; camera 0 held.  More cameras than the LDS table holds: the point passes run
    on camera windows (26-double rows), long tracks on 16-lane rows."""
    from bundle_adjustment_amd import hip_backend
    p = _config5()
    ref = o.bal_residuals(p.cams, p.pts, p.cam_idx, p.pt_idx, p.uv)
    ne = o.bal_normal_equations(p.cams, p.pts, p.cam_idx, p.pt_idx, p.uv, 0, "huber")
    iu9, iu3 = np.triu_indices(9), np.triu_indices(3)
    with hip_backend.Solver(0) as s:
        r, sse, cost = s.residuals_bal(p, "huber")
        assert np.abs(r - ref).max() <= 1e-9
        assert abs(sse - float((ref * ref).sum())) <= 1e-10 * sse and abs(cost - o.robust_cost(ref, "huber")) <= 1e-10 * cost
        out = s.linearize_bal(p, "huber", fixed_cam=0)
    for name, dev, want in (("Hcc", out["Hcc"], ne["Hcc"][:, iu9[0], iu9[1]]), ("bc", out["bc"], ne["bc"]),
                            ("Hpp", out["Hpp"], ne["Hpp"][:, iu3[0], iu3[1]]), ("bp", out["bp"], ne["bp"])):
        assert np.abs(dev - want).max() <= 1e-9 * np.abs(want).max(), name
    assert not out["Hcc"][0].any() and not out["bc"][0].any()


@pytest.mark.gpu
@pytest.mark.parametrize("extra,budget", [(dict(), 40), (dict(pcg_model_tol=0.5), 30)])
def test_config5_bal_solve_reaches_the_noise_floor_at_full_size(extra, budget):
    """ba_solve_bal on config 5: poses, points, f, k1, k2 adjusted from a 6.8 px start to the pixel noise (0.5 px per
    coordinate; with ~4 views per point the fit sits at ~0.56 px per observation); the summary's SSE and cost are the
    oracle's BAL residual of the returned parameters; the held camera did not move; a second solve gives the same bits.
    The solve must END ON A CONVERGENCE TEST (ftol = 1e-7) inside its budget: with the library's defaults (measured: 32 LM
    iterations, the last twenty at ~165 PCG iterations each once the cap-aware damping floor has settled) and with the
    PCG model test on (21 LM iterations; round 3's budget of 30)."""
    from bundle_adjustment_amd import hip_backend
    p = _config5()
    kw = dict(fixed_cam=0, loss="huber", max_iters=budget, ftol=1e-7, xtol=1e-10, gtol=1e-10, pcg_tol=0.1, pcg_max_iters=300, **extra)
    with hip_backend.Solver(0) as s:
        out, cams, pts = s.solve_bal(p, **kw)
        tr = s.trace()
        st = s.stats()
        again, cams2, pts2 = s.solve_bal(p, **kw)
    assert np.sqrt(out["initial_sse"] / p.n_obs) > 5.0 and np.sqrt(out["final_sse"] / p.n_obs) < 0.60
    # The solve has to STOP ON A CONVERGENCE TEST within its budget.  (Round 3 could not: the late inner solves of this chain
    # ran into the PCG cap at ever smaller dampings and the run ended on max_iters; what stops it now is the cap-aware
    # damping floor -- an inner solve that hits pcg_max_iters keeps the damping from falling any further.  The PCG model
    # test, automatic on band-structured problems at loose outer tolerances, is off at this ftol.)
    assert out["status_name"] in ("ftol", "xtol", "gtol") and out["accepted"] >= 5, (out, [t["pcg_iterations"] for t in tr])
    assert st["banded"] == 1
    assert len(tr) == out["iterations"] and all(t["pcg_iterations"] >= 1 for t in tr)
    r = o.bal_residuals(cams, pts, p.cam_idx, p.pt_idx, p.uv)
    assert abs(float((r * r).sum()) - out["final_sse"]) <= 1e-9 * out["final_sse"]
    assert abs(o.robust_cost(r, "huber") - out["final_cost"]) <= 1e-9 * out["final_cost"]
    assert np.array_equal(cams[0], p.cams[0])
    assert np.abs(cams[1:, 6] / p.cams[1:, 6] - 1).max() > 1e-4 and np.abs(cams[1:, 8]).max() > 0      # f and k2 moved
    assert again["final_cost"] == out["final_cost"] and np.array_equal(cams2, cams) and np.array_equal(pts2, pts)


@pytest.mark.gpu
def test_config5_bal_fp32_jacobian_mode_follows_the_fp64_descent():
    """BASELINE config 5's precision mode on the BAL camera: Jacobian blocks of the two PCG passes recomputed in fp32
    (radial terms included), every sum, the gradient, the cost, the right-hand side, the back substitution and the update
    in fp64.  Only the quasi-Newton operator changes: the descent follows the fp64 run -- same accepted steps, costs equal
    to fp32 operator accuracy -- and the residual of the result (fp64 kernel) is the oracle's."""
    from bundle_adjustment_amd import hip_backend
    p = _config5()
    kw = dict(fixed_cam=0, loss="huber", max_iters=10, ftol=1e-9, xtol=1e-12, gtol=0.0, pcg_tol=0.1, pcg_max_iters=400)
    with hip_backend.Solver(0) as s:
        ref, _, _ = s.solve_bal(p, **kw)
        tr_ref = s.trace()
        out, cams, pts = s.solve_bal(p, jacobian_precision=1, **kw)
        tr_out = s.trace()
    check_self_consistent(ref, tr_ref, kw)
    check_self_consistent(out, tr_out, kw)
    # same verdicts while the steps still matter (past the noise floor accept / reject is decided by round-off)
    compared = 0
    for a, b in zip(tr_out, tr_ref):
        if abs(b["cost"] - b["cost_trial"]) <= 1e-6 * b["cost"]:
            break
        assert a["accepted"] == b["accepted"], (a, b)
        compared += 1
    assert compared >= 5
    # the premise: where the two runs first part ways on accept / reject, both are past the noise floor
    for it, (a, b) in enumerate(zip(tr_out, tr_ref)):
        if a["accepted"] != b["accepted"]:
            for name, t in (("fp32", a), ("fp64", b)):
                assert abs(t["cost"] - t["cost_trial"]) <= 1e-6 * t["cost"], (f"iteration {it}: the runs disagree on accept / "
                                                                              f"reject while the {name} run's step still matters", a, b)
            break
    assert out["final_cost"] < 0.05 * out["initial_cost"]
    assert abs(out["final_cost"] - ref["final_cost"]) <= 2e-3 * ref["final_cost"], (out["final_cost"], ref["final_cost"])
    assert np.sqrt(out["final_sse"] / p.n_obs) < 0.75
    r = o.bal_residuals(cams, pts, p.cam_idx, p.pt_idx, p.uv)
    assert abs(float((r * r).sum()) - out["final_sse"]) <= 1e-9 * out["final_sse"]


@pytest.mark.gpu
def test_bal_fp32_jacobian_mode_reaches_the_fp64_solution():
    """Small problem, driven to convergence in both precision modes: the same minimiser."""
    from bundle_adjustment_amd import hip_backend
    p = _synthetic_bal(40, 2000, 5, seed=12)
    kw = dict(fixed_cam=0, loss="huber", max_iters=60, ftol=1e-12, xtol=1e-12, gtol=0.0, pcg_tol=1e-2, pcg_max_iters=400)
    with hip_backend.Solver(0) as s:
        a, ca, pa = s.solve_bal(p, **kw)
        check_self_consistent(a, s.trace(), kw)
        b, cb, pb = s.solve_bal(p, jacobian_precision=1, **kw)
        check_self_consistent(b, s.trace(), kw)
    assert abs(a["final_cost"] - b["final_cost"]) <= 1e-10 * a["final_cost"]
    # (only camera 0 is held: the scale of the scene is free, the minimiser is a one-parameter family and the two runs
    # stop at different members of it -- rotations, focal lengths and distortion are scale-free and agree)
    # Tolerances = about ten times what TWO FP64 RUNS of this very problem differ by when only a solver setting changes
    # (initial damping 1e-3, PCG tolerance 1e-3, kept preconditioner blocks off; tools/fp32_spread.py, round 4:
    # rotations 2e-9 .. 3e-8, intrinsics 2e-7 .. 7e-7 relative, scale 3e-6 .. 1e-3, points after removing the scale
    # 1e-8 .. 5e-6 relative; the fp32-Jacobian run sits inside that spread at 5e-9 / 2e-7 / 3e-4 / 2e-6).
    assert np.abs(ca[:, :3] - cb[:, :3]).max() <= 3e-7 and np.abs(ca[:, 6:] / cb[:, 6:] - 1).max() <= 1e-5
    sc = np.linalg.norm(ca[1:, 3:6]) / np.linalg.norm(cb[1:, 3:6])
    assert abs(sc - 1) < 1e-2 and np.abs(sc * pb - pa).max() <= 5e-5 * np.abs(pa).max()


@pytest.mark.gpu
def test_bal_handle_serves_pinhole_calls_after_a_bal_solve():
    """ba_solve_bal switches the handle to the 9-parameter kernels for the call only: the reference's pinhole entry points
    on the same handle, before and after, give the same bits."""
    from bundle_adjustment_amd import hip_backend
    from bundle_adjustment_amd.synthetic import make_problem
    q = make_problem(12, 900, 5, seed=4)
    p = _synthetic_bal(12, 900, 5, seed=4)
    with hip_backend.Solver(0) as s:
        s.set_problem(q)
        want = s.solve(loss="huber", max_iters=6, ftol=0.0, xtol=0.0, gtol=0.0)
        want_params = s.get_params()
        out, _, _ = s.solve_bal(p, loss="huber", max_iters=6, ftol=0.0, xtol=0.0, gtol=0.0)
        assert out["final_cost"] < out["initial_cost"]
        s.set_problem(q)
        got = s.solve(loss="huber", max_iters=6, ftol=0.0, xtol=0.0, gtol=0.0)
        got_params = s.get_params()
    assert got["final_cost"] == want["final_cost"]
    assert np.array_equal(got_params[0], want_params[0]) and np.array_equal(got_params[1], want_params[1])
