"""GPU: every way out of the multi-kernel LM driver leaves the handle as a fresh one.  One handle goes through each exit
in turn -- every parameter held, no iterations allowed, the gtol / ftol / xtol stops, the iteration limit, inner solves
cut off at pcg_max_iters, a failing solve -- each time with the per-solve modes switched on (profile = 1, fp32 Jacobian
blocks).  Behind each exit the same plain solve (fp64, Huber, no profile) from the start parameters must give the bits it
gives on a fresh handle, and must leave nothing in the profile: no mode of the solve before it is still on."""
import numpy as np
import pytest

from bundle_adjustment_amd import hip_backend
from bundle_adjustment_amd.synthetic import make_problem

pytestmark = pytest.mark.gpu
# small_solver=1: the multi-kernel loop, not the single-launch window solver a problem of this size goes to by default
PLAIN = dict(loss="huber", max_iters=8, ftol=1e-12, xtol=1e-12, gtol=0.0, small_solver=1, profile=0, jacobian_precision=0)
MODES = dict(loss="huber", small_solver=1, profile=1, jacobian_precision=1)
OFF = dict(ftol=0.0, xtol=0.0, gtol=0.0)
COUNTS = ("iterations", "status", "accepted", "pcg_iterations", "initial_sse", "initial_cost", "final_sse", "final_cost", "final_lambda")


def _plain(s, p):
    s.set_params(p.cams, p.pts)
    s.profile(reset=True)
    out = s.solve(**PLAIN)
    trace = [{k: v for k, v in r.items() if k != "seconds"} for r in s.trace()]
    return s.get_params(), {k: out[k] for k in COUNTS}, trace, s.profile()


def test_every_exit_of_the_driver_leaves_no_per_solve_mode_behind(monkeypatch):
    p = make_problem(6, 60, 4, seed=0)
    with hip_backend.Solver(0) as fresh:
        fresh.set_problem(p)
        (cams0, pts0), counts0, trace0, prof0 = _plain(fresh, p)
    assert prof0 == {} and counts0["iterations"] > 1 and counts0["final_cost"] < counts0["initial_cost"]

    def all_held(s):
        s.set_held(cams=np.ones(p.n_cams, bool), points=np.ones(p.n_pts, bool))
        out = s.solve(**MODES, max_iters=5, **OFF)
        s.set_held()
        assert (out["status"], out["iterations"]) == (0, 0) and out["final_cost"] == out["initial_cost"]

    def no_iterations(s):
        out = s.solve(**MODES, max_iters=0, **OFF)
        assert (out["status"], out["iterations"]) == (0, 0) and out["final_cost"] == out["initial_cost"]

    def gtol_stop(s):
        out = s.solve(**MODES, max_iters=5, ftol=0.0, xtol=0.0, gtol=1e30)
        assert (out["status"], out["iterations"], out["pcg_iterations"]) == (3, 0, 0)

    def ftol_stop(s):
        out = s.solve(**MODES, max_iters=50, ftol=1e-2, xtol=0.0, gtol=0.0)
        assert out["status"] == 1 and 0 < out["iterations"] < 50

    def xtol_stop(s):
        out = s.solve(**MODES, max_iters=50, ftol=0.0, xtol=1e-3, gtol=0.0)
        assert out["status"] == 2 and 0 < out["iterations"] < 50

    def iteration_limit(s):
        out = s.solve(**MODES, max_iters=2, **OFF)
        assert (out["status"], out["iterations"]) == (0, 2)

    def capped_inner_solves(s):
        before = s.stats()["cap_floor_raises"]
        out = s.solve(**MODES, max_iters=3, pcg_max_iters=1, **OFF)
        assert (out["status"], out["iterations"], out["pcg_iterations"]) == (0, 3, 3)
        assert s.stats()["cap_floor_raises"] - before == 3

    def poisoned_trial(s):
        monkeypatch.setenv("BA_DEBUG_POISON_TRIAL", "1")          # every trial cost NaN: rejected until the damping is at its cap
        with pytest.raises(hip_backend.BAHipError, match="error -4: non-finite cost at the trial point"):
            s.solve(**MODES, max_iters=50, **OFF)
        monkeypatch.delenv("BA_DEBUG_POISON_TRIAL")

    with hip_backend.Solver(0) as s:
        s.set_problem(p)
        for leave in (all_held, no_iterations, gtol_stop, ftol_stop, xtol_stop, iteration_limit, capped_inner_solves, poisoned_trial):
            s.set_params(p.cams, p.pts)
            leave(s)
            (cams, pts), counts, trace, prof = _plain(s, p)
            assert np.array_equal(cams, cams0) and np.array_equal(pts, pts0), leave.__name__
            assert counts == counts0 and trace == trace0, leave.__name__
            assert prof == {}, (leave.__name__, prof)
