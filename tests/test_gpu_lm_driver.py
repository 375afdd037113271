"""GPU: the LM driver of the multi-kernel solve behind the reduced system -- the step's scalar fold (scalars_body), the
device-side verdict (lm_decide), the host half (apply_verdict, LmState, the damping floor of capped inner solves) -- against
oracle.lm_solve, iteration by iteration: equal PCG counts and verdicts; damping, gain ratio and trial cost to 1e-6, step
norm to 1e-7 (tests/lm_trace.py); then the exit: status, iteration, accepted steps, final_lambda.  Every trace is also
held to the driver's own rules (check_self_consistent).

The cases (tests/lm_driver_cases.py) are built so that the demand is fair and the driver's faults show: rejection streaks
(the same linearisation damped again with nu doubling, speculated buffers discarded, nu back at 2 afterwards), inner solves
that run into pcg_max_iters (the floor raises the damping against Nielsen's update), both through the BAL entry point as
well, and every way out of the loop with a factor two between the tested quantity and its threshold on either side.
tests/test_lm_trace_host.py checks those conditions with the oracle alone, and that a driver with a halved model decrease,
a dropped point share of g^T d, a nu that is not reset or an ignored floor fails these very comparisons by >= 1e3 x the
tolerance.  Each case: a fresh handle, well under a second of GPU time, a few seconds of oracle."""
import numpy as np
import pytest

from bundle_adjustment_amd import hip_backend
from bundle_adjustment_amd.bal import BALProblem
from tests import lm_driver_cases as cases
from tests import lm_trace

pytestmark = pytest.mark.gpu


def _solve(name):
    """The case on a fresh handle: (summary, trace, stats, parameters)."""
    p, opts = cases.problem(name), cases.options(name)
    cm, pm = cases.held(name)
    with hip_backend.Solver(0) as s:
        if isinstance(p, BALProblem):
            out, cams, pts = s.solve_bal(p, fixed_cam=cases.fixed_cam(name), held_cameras=cm, held_points=pm, **opts)
        else:
            assert p.fixed_cam == cases.fixed_cam(name)
            s.set_problem(p)
            if cm is not None:
                s.set_held(cm, pm)
            out = s.solve(**opts)
            cams, pts = s.get_params()
        return out, s.trace(), s.stats(), (cams, pts)


def _follow(name, exit_under_test=False):
    ref = cases.mirror(name)
    out, tr, st, params = _solve(name)
    lm_trace.check_self_consistent(out, tr, cases.options(name))
    assert abs(out["initial_cost"] - ref["cost0"]) <= 1e-10 * ref["cost0"]
    compared, _ = lm_trace.check_follows(out, tr, ref, exit_under_test=exit_under_test)
    return ref, out, tr, st, params, compared


@pytest.mark.parametrize("name", ["rejections", "rejections_jacobi", "rejections_lag0", "bal_rejections_fixed", "bal_rejections_free"])
def test_rejected_steps_follow_the_mirror(name):
    """Rejection streaks: two of them in 12 iterations (Jacobi: one of four), each followed by an accepted step."""
    ref, out, tr, st, _, compared = _follow(name)
    assert compared == 12 == out["iterations"]
    assert cases.streaks([dict(rho=1.0 if t["accepted"] else -1.0) for t in tr]) == cases.streaks(ref["history"])
    assert st["cap_floor_raises"] == 0
    if name == "rejections_lag0":
        assert st["precond_reuses"] == 0 and st["precond_builds"] == 12


@pytest.mark.parametrize("name", ["capped", "bal_capped_fixed", "bal_capped_free"])
def test_capped_inner_solves_raise_the_damping_through_the_floor(name):
    """Every inner solve runs into pcg_max_iters = 2: accepted steps with gain ratios above 1 (Nielsen: a third of the damping),
    and the damping triples instead, 1e-4 -> 2.43e-2."""
    ref, out, tr, st, _, compared = _follow(name)
    assert compared == 6 == out["iterations"] == out["accepted"] and out["pcg_iterations"] == 12
    assert st["cap_floor_raises"] == 6
    assert [t["damping"] for t in tr] == [h["lam"] for h in ref["history"]]        # products of 3.0: exact


@pytest.mark.parametrize("name", ["exit_ftol", "exit_xtol", "exit_gtol", "exit_gtol_at_once", "exit_max_iters", "exit_xtol_held",
                                  "exit_xtol_mostly_held"])
def test_every_exit_fires_at_the_mirrors_iteration(name):
    """status, the exit iteration, accepted steps and final_lambda are the mirror's (check_follows, having compared every
    iteration); the held cases: |x| of the xtol test without the masks' share."""
    ref, out, tr, st, (cams, pts), compared = _follow(name, exit_under_test=True)
    assert ref["status"] == cases.EXIT_STATUS[name] == out["status_name"]
    assert compared == ref["iterations"] == out["iterations"] == len(tr)
    if name == "exit_gtol_at_once":
        assert (out["status"], out["iterations"], out["pcg_iterations"]) == (3, 0, 0) and out["final_cost"] == out["initial_cost"]
        assert out["final_lambda"] == cases.options(name)["initial_lambda"]
    cm, pm = cases.held(name)
    if cm is not None:
        p = cases.problem(name)
        bits = ((cm[:, None] >> np.arange(6)[None]) & 1).astype(bool)
        assert np.array_equal(cams[bits], p.cams[bits]) and np.array_equal(pts[pm], p.pts[pm])
        assert np.abs(cams - ref["cams"]).max() <= 1e-6 * np.abs(ref["cams"]).max()
