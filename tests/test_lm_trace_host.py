"""CPU: the two checkers of tests/lm_trace.py on traces built from the oracle's own LM mirror, and the conditions that make
the cases of tests/test_gpu_lm_driver.py (tests/lm_driver_cases.py) a fair demand on the device.

The clean mirror passes both checkers.  Each of the four effective faults of the driver (oracle.lm_solve(mutate=...): a
model decrease without its 0.5, the points' share of g^T d dropped, nu not reset, the cap floor ignored -- all of which
still converge) fails check_follows on the case meant for it by >= 1e3 x the tolerance, and corrupted traces fail
check_self_consistent.  Conditions on the cases (oracle alone):
  PCG stop margin   every inner solve ended by the residual test stops with sqrt(rz / rz0) <= (1 - 1e-6) pcg_tol and had
                    >= (1 + 1e-6) pcg_tol one iteration before: round-off does not move the count, so equal counts are fair
  exit margin       the quantity of the exit under test is <= 1/2 its threshold at the mirror's exit iteration and >= 2 x
                    the threshold at every earlier one
  sensitivity       with every pixel perturbed by 1e-13 relative the mirror keeps every PCG count and moves each compared
                    quantity by <= 1e-2 of its tolerance
  coverage          the rejections cases have >= 2 streaks of rejected steps, each followed by an accepted step, the second
                    one starting from nu = 2 again; every case compares >= 6 iterations (the exit at once apart: it has none)"""
import copy

import numpy as np
import pytest

from tests import lm_driver_cases as cases
from tests import lm_trace

ALL = sorted(cases.CASES)
EXITS = sorted(cases.EXIT_STATUS)


def _compared(name):
    """How many iterations of the case get compared, and whether a tolerance exit is under test."""
    ref = cases.mirror(name)
    exit_test = name in EXITS
    return lm_trace.deviations(lm_trace.from_oracle(ref)[1], ref, exit_test)[0], exit_test


@pytest.mark.parametrize("name", ALL)
def test_the_clean_mirror_passes_both_checkers(name):
    ref = cases.mirror(name)
    summary, trace = lm_trace.from_oracle(ref)
    lm_trace.check_self_consistent(summary, trace, cases.options(name))
    compared, exit_test = _compared(name)
    got, dev = lm_trace.check_follows(summary, trace, ref, exit_under_test=exit_test)
    assert got == compared and max(dev.values()) == 0.0
    if name in cases.SHORT_CASES:
        assert compared == ref["iterations"] == cases.SHORT_CASES[name]
    else:
        assert compared >= 6
    if exit_test:
        assert compared == ref["iterations"] and ref["status"] == cases.EXIT_STATUS[name]


@pytest.mark.parametrize("name", ALL)
def test_every_compared_inner_solve_stops_with_a_margin(name):
    ref = cases.mirror(name)
    tol = cases.options(name)["pcg_tol"]
    for h in ref["history"][:_compared(name)[0]]:
        if h["pcg_stop"] == "residual":
            assert h["pcg_ratio_last"] * tol <= (1 - 1e-6) * tol and h["pcg_ratio_prev"] * tol >= (1 + 1e-6) * tol, h
        else:
            assert h["pcg_stop"] == "cap" and h["pcg"] == cases.options(name)["pcg_max_iters"], h


@pytest.mark.parametrize("name", ALL)
def test_noise_of_1e_13_in_the_pixels_moves_nothing_that_is_compared(name):
    ref, noisy = cases.mirror(name), cases.mirror(name, noise_seed=7)
    compared, exit_test = _compared(name)
    got, dev = lm_trace.deviations(lm_trace.from_oracle(noisy)[1], ref, exit_test)
    assert got == compared
    assert [h["pcg"] for h in noisy["history"]] == [h["pcg"] for h in ref["history"]]
    assert (noisy["status"], noisy["iterations"], noisy["accepted"]) == (ref["status"], ref["iterations"], ref["accepted"])
    for k, v in dev.items():
        assert v <= 1e-2 * lm_trace.TOL[k], (k, v)


@pytest.mark.parametrize("name", cases.REJECTION_CASES)
def test_rejection_cases_have_two_streaks_and_the_second_restarts_nu(name):
    hist = cases.mirror(name)["history"][:_compared(name)[0]]
    runs = cases.streaks(hist)
    assert len(runs) >= 2 and max(runs) >= 3, runs
    # the first rejection of every streak doubles the damping (nu = 2), the second multiplies it by 4
    for a, b, c in zip(hist, hist[1:], hist[2:]):
        if a["rho"] > 0 and b["rho"] <= 0:
            assert c["lam"] == 2.0 * b["lam"]


def test_the_jacobi_variant_has_one_long_streak():
    """(Jacobi on the same problem: four rejections in a row and no second streak within 12 iterations -- nu goes 2, 4, 8, 16.)"""
    assert cases.streaks(cases.mirror("rejections_jacobi")["history"]) == [4]


@pytest.mark.parametrize("name", cases.CAPPED_CASES)
def test_capped_cases_hit_the_cap_every_time_and_the_floor_raises_the_damping(name):
    hist = cases.mirror(name)["history"]
    assert len(hist) == 6 and all(h["pcg"] == 2 and h["pcg_stop"] == "cap" and h["rho"] > 0 for h in hist)
    # Nielsen's update alone would lower the damping after each of these steps (gain ratio > 0.5): what raises it is the floor
    assert all(h["rho"] > 0.5 for h in hist)
    lam = 1e-4
    for h in hist:
        assert h["lam"] == lam
        lam = 3.0 * lam
    if name == "capped":
        assert all(1.25 <= h["rho"] <= 1.78 for h in hist), [h["rho"] for h in hist]


@pytest.mark.parametrize("name", EXITS)
def test_exits_have_a_factor_two_on_either_side_of_the_threshold(name):
    ref, opts = cases.mirror(name), cases.options(name)
    hist = ref["history"]
    assert ref["status"] == cases.EXIT_STATUS[name]
    if name == "exit_max_iters":
        assert ref["iterations"] == opts["max_iters"] == 6 and [h["rho"] > 0 for h in hist] == [True] * 3 + [False] * 3
        return
    if name == "exit_gtol_at_once":
        assert ref["iterations"] == 0 and ref["gmax"] <= 0.5 * opts["gtol"]
        return
    if ref["status"] == "ftol":
        q = [(h["cost"] - h["cost_new"]) / h["cost_new"] for h in hist if h["rho"] > 0]
        thr = opts["ftol"]
    elif ref["status"] == "xtol":
        q = [h["step"] / (opts["xtol"] + h["xnorm"]) for h in hist]
        thr = opts["xtol"]
    else:
        q = [h["gmax"] for h in hist] + [ref["gmax"]]
        thr = opts["gtol"]
    assert q[-1] <= 0.5 * thr and min(q[:-1]) >= 2.0 * thr, (q, thr)
    assert ref["iterations"] >= 12 or name in cases.SHORT_CASES


def test_a_driver_that_miscounts_the_held_share_of_x_leaves_at_another_iteration():
    """exit_xtol_mostly_held: |x| runs over the entries the masks leave free (include/ba_hip.h, ba_set_held), a quarter of the
    whole.  With the whole |x| the test would pass one iteration early, with the held share subtracted twice (nothing left
    of the points) not at the mirror's exit iteration: either fault shows in the exit iteration, beyond the exit margin."""
    name = "exit_xtol_mostly_held"
    ref, p, xtol = cases.mirror(name), cases.problem(name), cases.options(name)["xtol"]
    hist = ref["history"]
    x_all = float(np.sqrt((p.cams ** 2).sum() + (p.pts ** 2).sum()))
    assert hist[0]["xnorm"] < 0.26 * x_all
    assert hist[-2]["step"] <= xtol * (xtol + 0.98 * x_all)                                 # (0.98: the points move a little)
    cam_only = float(np.sqrt((ref["cams"] ** 2).sum()))
    assert hist[-1]["step"] >= 2.0 * xtol * (xtol + cam_only)


MUTANTS = [("model_half", "rejections"), ("model_half", "capped"), ("gtd_points", "rejections"), ("gtd_points", "capped"),
           ("nu_kept", "rejections"), ("nu_kept", "bal_rejections_fixed"), ("no_floor", "capped"), ("no_floor", "bal_capped_free")]


@pytest.mark.parametrize("mutant,name", MUTANTS)
def test_every_effective_mutant_fails_check_follows_by_a_wide_margin(mutant, name):
    ref = cases.mirror(name)
    summary, trace = lm_trace.from_oracle(cases.mirror(name, mutate=mutant))
    _, dev = lm_trace.deviations(trace, ref)
    assert any(dev[k] >= 1e3 * lm_trace.TOL[k] for k in dev), dev
    with pytest.raises(AssertionError):
        lm_trace.check_follows(summary, trace, ref)


def _clean(name):
    summary, trace = lm_trace.from_oracle(cases.mirror(name))
    return copy.deepcopy(summary), copy.deepcopy(trace)


def test_self_consistency_sees_one_damping_off_by_1e_9():
    summary, trace = _clean("rejections")
    for i in (1, 5, 8, 11):                   # behind an accepted step, inside a streak, behind a streak
        bad = copy.deepcopy(trace)
        bad[i]["damping"] *= 1.0 + 1e-9
        with pytest.raises(AssertionError, match="damping"):
            lm_trace.check_self_consistent(summary, bad, cases.options("rejections"))
    with pytest.raises(AssertionError, match="final_lambda"):
        lm_trace.check_self_consistent(dict(summary, final_lambda=summary["final_lambda"] * (1.0 + 1e-9)), trace, cases.options("rejections"))


def test_self_consistency_sees_a_swapped_verdict():
    summary, trace = _clean("rejections")
    for i in (2, 4):
        bad = copy.deepcopy(trace)
        bad[i]["accepted"] = not bad[i]["accepted"]
        with pytest.raises(AssertionError):
            lm_trace.check_self_consistent(summary, bad, cases.options("rejections"))


@pytest.mark.parametrize("mutant,name", [("nu_kept", "rejections"), ("no_floor", "capped")])
def test_self_consistency_sees_a_nu_that_is_not_reset_and_a_floor_that_is_not_applied(mutant, name):
    """The faulty drivers' own records: every cost, verdict and sum in them is coherent, only the damping breaks the rule."""
    summary, trace = lm_trace.from_oracle(cases.mirror(name, mutate=mutant))
    with pytest.raises(AssertionError, match="damping"):
        lm_trace.check_self_consistent(summary, trace, cases.options(name))


def test_self_consistency_sees_a_cost_that_is_not_carried_over_and_wrong_sums():
    summary, trace = _clean("capped")
    opts = cases.options("capped")
    bad = copy.deepcopy(trace)
    bad[3]["cost"] = float.fromhex((bad[3]["cost"] * (1 + 2 ** -52)).hex())      # one ulp
    assert bad[3]["cost"] != trace[3]["cost"]
    with pytest.raises(AssertionError, match="carried over"):
        lm_trace.check_self_consistent(summary, bad, opts)
    for key in ("iterations", "accepted", "pcg_iterations"):
        with pytest.raises(AssertionError):
            lm_trace.check_self_consistent(dict(summary, **{key: summary[key] + 1}), trace, opts)
    with pytest.raises(AssertionError, match="final_cost"):
        lm_trace.check_self_consistent(dict(summary, final_cost=trace[-1]["cost"]), trace, opts)
