"""CPU: what entitles tests/test_gpu_window_held.py to its demands.  The window kernels (csrc/ba_small.hpp,
csrc/ba_small_mw.hpp) are followed there iteration by iteration against tests/window_reference.window_lm, a dense LM over
the free columns; here, with numpy alone,

  * that reference follows oracle.lm_solve(linear_solver='dense') where the oracle can go (no masks, linear / huber);
  * every case of tests/window_cases.py is conditioned well enough: the first damped step, solved a second way (block
    elimination, as the device does it), moves by at most 1 / 100 of the GPU test's tolerances, and the whole run
    driven that second way drifts by at most 1 / 10 of them;
  * no iteration of a case is decided by round-off, so the GPU test's `compared == iterations` can hold;
  * the comparison has power: a reference with a window kernel's fault built in (window_lm's mutants) fails it within
    two iterations, or at the exit; and what the end-point check the suite had for held windows makes of the same
    mutants (it sees the coupled ones after 30 iterations, and cannot see a stopping test that counts held entries)."""
import numpy as np
import pytest

from bundle_adjustment_amd.synthetic import make_problem
from oracle import ba_oracle as o
from tests import lm_trace
from tests import window_cases as wc
from tests import window_reference as wr
from tests.held_reference import Reduced

STEP_IDS = [f"{s}-{l}-{f}" for s, l, f in wc.STEP_CASES]


# ---------------------------------------------------------------- the reference against the oracle
@pytest.mark.parametrize("n_cams,n_pts,k,loss,dups", [
    (2, 37, 2, "huber", 0), (3, 130, 3, "linear", 5), (5, 129, 4, "huber", 0), (6, 300, 4, "linear", 9), (7, 256, 5, "huber", 0),
    (8, 200, 6, "linear", 0)])
def test_reference_follows_the_oracles_dense_lm_without_masks(n_cams, n_pts, k, loss, dups):
    """test_gpu_small.py's problems (same generator, seeds and repeated pairs; the two largest with fewer points), six
    iterations, all tolerances off: full normal equations with LU here, the explicit Schur complement there.
    Measured, the largest over the six cases and the iterations round-off does not decide (4 to 6 of the 6), relative:
    trial cost 1.3e-14, damping 0 (the same bits), step norm 4.3e-10, gain ratio 2.6e-8 -- that one is the trial cost's
    1e-14 over the relative cost change of the iteration, which falls to 2e-7 in the linear cases: gain ratio deviation x
    relative cost change is 1.9e-14 at most.  Final cameras 2.3e-13, points 1.3e-12 (absolute).  What the stopping tests
    see: |x| 7.2e-14 relative, max |g| 8.2e-14 of its value at the start.  Asserted with a decade of margin."""
    p = make_problem(n_cams, n_pts, min(k, n_cams), seed=17 + n_cams, outlier_frac=0.03 if loss == "huber" else 0.0)
    if dups:
        p = wc.with_duplicates(p, dups, seed=n_cams)
    ref = o.lm_solve(p.cams, p.pts, p.cam_idx, p.pt_idx, p.uv, p.K4, fixed_cam=p.fixed_cam, loss=loss, max_iters=6,
                     linear_solver="dense", **wc.OFF)
    got = wr.window_lm(p, loss=loss, max_iters=6, **wc.OFF)
    summary, trace = lm_trace.from_oracle(got)
    tol = dict(cost_trial=2e-13, damping=1e-12, gain_ratio=3e-7, step_norm=5e-9)
    compared, dev = lm_trace.check_follows(summary, trace, ref, tol=tol)
    assert compared >= 4
    for a, b in list(zip(got["history"], ref["history"]))[:compared]:
        assert abs(a["rho"] - b["rho"]) / abs(b["rho"]) * abs(b["cost"] - b["cost_new"]) / b["cost"] <= 2e-13
    g0 = ref["history"][0]["gmax"]
    print("final: cams %.2e pts %.2e; max |g| %.2e of the first" % (
        np.abs(got["cams"] - ref["cams"]).max(), np.abs(got["pts"] - ref["pts"]).max(),
        max(abs(a["gmax"] - b["gmax"]) for a, b in zip(got["history"], ref["history"])) / g0))
    assert np.abs(got["cams"] - ref["cams"]).max() <= 3e-12 and np.abs(got["pts"] - ref["pts"]).max() <= 2e-11
    assert abs(got["cost"] - ref["cost"]) <= 2e-13 * ref["cost"] and abs(got["cost0"] - ref["cost0"]) <= 2e-13 * ref["cost0"]
    for a, b in zip(got["history"], ref["history"]):            # what the stopping tests see
        assert abs(a["gmax"] - b["gmax"]) <= 1e-12 * g0 and abs(a["xnorm"] - b["xnorm"]) <= 1e-12 * b["xnorm"]


# ---------------------------------------------------------------- the reference against itself
def _spread(p, cm, pm, loss, f_scale, lam):
    """The first damped step two ways -> (largest entry difference over max(1, |x|), relative difference of the norms)."""
    red = Reduced(p.cams, p.pts, p.cam_idx, p.pt_idx, p.uv, p.K4, p.fixed_cam, cm, pm)
    H, g = wr.linearise(red, red.cams, red.pts, loss, f_scale)
    d_full, _ = wr.damped_step(H, g, lam)
    d_elim = wr.first_step_by_elimination(p, cm, pm, loss, f_scale, lam)
    xmax = max(1.0, np.abs(red.x(red.cams, red.pts)).max())
    return np.abs(d_full - d_elim).max() / xmax, abs(np.linalg.norm(d_full) - np.linalg.norm(d_elim)) / np.linalg.norm(d_full)


@pytest.mark.parametrize("shape,loss,f_scale", wc.STEP_CASES, ids=STEP_IDS)
def test_step_cases_are_well_conditioned(shape, loss, f_scale):
    """The spread between LU on the full damped normal equations and block elimination + back substitution is the case's
    conditioning: at most 1 / 100 of the GPU test's 1e-7 max(1, |x|) on parameters and 1e-7 on the step norm.  Measured:
    largest entry spread 6.1e-13, largest norm spread 1.6e-12."""
    entry, norm = _spread(wc.step_problem(shape, loss), *wc.step_masks(shape), loss, f_scale, 1e-4)
    print(f"spread: entry {entry:.2e} norm {norm:.2e}")
    assert entry <= wc.PARAM_TOL / 100 and norm <= wc.TOL["step_norm"] / 100


def test_rejected_and_exit_cases_are_well_conditioned():
    """The rejected-steps start (a step of 270 m in all) at every damping of its streak of rejections.  Measured: cauchy
    entry spread 1.4e-11, norm 4.4e-13; soft_l1 1.6e-12, 2.3e-14.  (arctan, the contrast the GPU test does not run: 1e-7 and
    2e-9 -- it would not be entitled to the tolerances.)  Exit problem: 1.2e-15, 3.5e-15."""
    for loss in wc.REJECTED_GPU_LOSSES:
        lam, nu = wc.REJECTED_LAMBDA, 2.0
        for _ in range(6):
            entry, norm = _spread(wc.rejected_problem(loss), *wc.rejected_masks(), loss, 2.0, lam)
            print(f"rejected {loss} damping {lam:.1e}: entry {entry:.2e} norm {norm:.2e}")
            assert entry <= wc.PARAM_TOL / 100 and norm <= wc.TOL["step_norm"] / 100
            lam, nu = lam * nu, 2 * nu
    entry, norm = _spread(*wc.exit_problem(), wc.EXIT_LOSS, 1.0, 1e-4)
    print(f"exit: entry {entry:.2e} norm {norm:.2e}")
    assert entry <= wc.PARAM_TOL / 100 and norm <= wc.TOL["step_norm"] / 100


def _drift(ref, run, exit_under_test=False, sse=True):
    """Largest deviation of `run` from `ref` per quantity, each as a fraction of the GPU test's tolerance."""
    compared, dev = lm_trace.deviations(lm_trace.from_oracle(run)[1], ref, exit_under_test)
    assert compared == ref["iterations"] == run["iterations"]
    out = {k: v / wc.TOL[k] for k, v in dev.items()}
    out["cost"] = max(abs(a["cost"] - b["cost"]) / b["cost"] for a, b in zip(run["history"], ref["history"])) / wc.COST_TOL
    out["params"] = wc.params_agree(run["cams"], run["pts"], ref)
    if sse:
        out["sse"] = abs(run["sse"] - ref["sse"]) / ref["sse"] / wc.COST_TOL
    print("drift / tolerance: " + ", ".join(f"{k} {v:.1e}" for k, v in out.items()))
    return out


@pytest.mark.parametrize("shape,loss,f_scale", wc.STEP_CASES, ids=STEP_IDS)
def test_step_cases_stay_conditioned_along_the_whole_run(shape, loss, f_scale):
    """The first step says little about the eighth: the damping falls by three per accepted step (1e-4 -> 5e-8) and the
    system's conditioning with it, and what one step is off by the next ones start from.  So the WHOLE run a second way,
    every step by block elimination (window_lm(by_elimination=True)): each of the two drivers is backward stable, so
    their drift apart estimates the forward error either one has on this case -- and the device's, a third arrangement of
    the same elimination.  Every compared quantity must drift by at most 1 / 10 of the GPU test's tolerance for it.
    Measured, the largest over the cases, as fractions of the tolerances: step norm 4.3e-2 (c2_p37 huber 0.5; 3e-3 and
    less from four cameras up), gain ratio 3.3e-3, damping 8.5e-4, trial cost 5.2e-4, parameters 4.5e-5.
    What this keeps out (window_cases.start): arctan from four times the default start distance drifts by 0.86 of the step
    norm's tolerance on c4_p65, the two-camera case by 0.12 under cauchy."""
    ref = wc.step_reference(shape, loss, f_scale)
    run = wr.window_lm(wc.step_problem(shape, loss), *wc.step_masks(shape), loss=loss, f_scale=f_scale, max_iters=wc.iters(loss),
                       by_elimination=True, **wc.OFF)
    assert max(_drift(ref, run).values()) <= 0.1


def test_rejected_and_exit_cases_stay_conditioned_along_the_whole_run():
    """Measured, as fractions of the tolerances: rejected cauchy (6 iterations) trial cost 2.2e-3, soft_l1 5.3e-2 (the last
    rejected step, at 26 times the model's decrease above the start); exits 1.9e-5 and less.  The final SSE is left out for
    the rejected cases, as in the GPU test: under cauchy it is 9.4e9 px^2, a few landmarks far out that the loss has given
    up, and drifts by 0.13 of the tolerance (every other case: 2.5e-3 and less)."""
    for loss in wc.REJECTED_GPU_LOSSES:
        run = wr.window_lm(wc.rejected_problem(loss), *wc.rejected_masks(), loss=loss, f_scale=2.0, max_iters=wc.REJECTED_ITERS[loss],
                           lam0=wc.REJECTED_LAMBDA, by_elimination=True, **wc.OFF)
        assert max(_drift(wc.rejected_reference(loss), run, sse=False).values()) <= 0.1
    p, cm, pm = wc.exit_problem()
    run = wr.window_lm(p, cm, pm, loss=wc.EXIT_LOSS, f_scale=1.0, max_iters=wc.EXIT_ITERS, by_elimination=True, **wc.OFF)
    assert max(_drift(wc.exit_reference(), run, exit_under_test=True).values()) <= 0.1


# ---------------------------------------------------------------- comparability
@pytest.mark.parametrize("shape,loss,f_scale", wc.STEP_CASES, ids=STEP_IDS)
def test_no_iteration_of_a_step_case_is_decided_by_round_off(shape, loss, f_scale):
    """Every iteration within the case's count changes the cost by more than 10 x lm_trace.ROUND_OFF_STOP of it (measured:
    1.2e-7 at the least, c4_p65 linear), so check_follows compares as many iterations as the table says; and every case
    runs its full count."""
    ref = wc.step_reference(shape, loss, f_scale)
    assert ref["iterations"] == wc.iters(loss) and ref["status"] == "max_iters"
    least = min(abs(h["cost"] - h["cost_new"]) / h["cost"] for h in ref["history"])
    print(f"least relative cost change {least:.2e}")
    assert least > 10 * lm_trace.ROUND_OFF_STOP
    compared, _ = lm_trace.deviations(lm_trace.from_oracle(ref)[1], ref)
    assert compared == wc.iters(loss)


def test_rejected_cases_reject_and_are_comparable():
    """cauchy rejects the first four steps, soft_l1 the first five -- the same linearisation damped again, nu doubling --
    and arctan, the contrast, none; no verdict near round-off."""
    want = dict(cauchy=[False] * 4 + [True] * 2, soft_l1=[False] * 5 + [True] * 5, arctan=[True] * 10)
    for loss in wc.REJECTED_LOSSES:
        ref = wc.rejected_reference(loss)
        assert [h["rho"] > 0 for h in ref["history"]] == want[loss], loss
        assert min(abs(h["cost"] - h["cost_new"]) / h["cost"] for h in ref["history"]) > 1e-3
        assert lm_trace.deviations(lm_trace.from_oracle(ref)[1], ref)[0] == wc.REJECTED_ITERS[loss] == ref["iterations"]


def test_exit_thresholds_sit_between_two_iterations():
    """The thresholds come from the reference's history with every tolerance off (window_cases.exit_thresholds asserts a
    factor 1.1 to both neighbours: five decades above the 1e-6 the device may deviate by); with one of them set the
    reference leaves where the table says, having stopped for that reason."""
    th = wc.exit_thresholds()
    print(th)
    g, x, f = wc.exit_reference("gtol"), wc.exit_reference("xtol"), wc.exit_reference("ftol")
    assert (g["status"], g["iterations"]) == ("gtol", wc.GTOL_AFTER)
    assert (x["status"], x["iterations"]) == ("xtol", wc.XTOL_AT)
    assert (f["status"], f["iterations"]) == ("ftol", wc.FTOL_AT)
    # the held entries matter to these exits: their gradient stays above the threshold, and they are 40 % of |x|
    h = wc.exit_reference()["history"]
    all_g = wc.exit_reference(None, "g_all")["history"]
    assert min(r["gmax"] for r in all_g) > 2 * th["gtol"] > 2 * h[wc.GTOL_AFTER]["gmax"]
    all_x = wc.exit_reference(None, "x_all")["history"]
    assert all_x[3]["xnorm"] > 1.3 * h[3]["xnorm"]


# ---------------------------------------------------------------- power
def _fails(mutant, ref, **kw):
    try:
        wc.follow(*lm_trace.from_oracle(mutant), ref, **kw)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("shape,loss,f_scale", wc.STEP_CASES, ids=STEP_IDS)
def test_step_comparison_passes_the_reference_and_fails_its_mutants(shape, loss, f_scale):
    """A held point whose columns stay in the system, a held camera parameter whose row is not the identity, an IRLS weight
    that ignores f_scale: each fails the GPU test's comparison within its first two iterations, on every case it applies
    to (unit_scale: the non-linear losses).  Measured: the largest deviation of a mutant is at least 5e5 x its tolerance
    (pt_coupled; cam_coupled 2e8, unit_scale 2e6), at least 5e-4 in the trial cost.  The unmutated reference passes."""
    ref = wc.step_reference(shape, loss, f_scale)
    wc.follow(*lm_trace.from_oracle(ref), ref)
    two = wc.step_reference(shape, loss, f_scale, None, 2)
    for mutate in ("pt_coupled", "cam_coupled") + (("unit_scale",) if loss != "linear" else ()):
        bad = wc.step_reference(shape, loss, f_scale, mutate, 2)
        summary, trace = lm_trace.from_oracle(bad)
        with pytest.raises(AssertionError):
            lm_trace.check_follows(summary, trace, two, tol=wc.TOL)
        _, dev = lm_trace.deviations(trace, two)
        print(mutate, {k: "%.1e" % v for k, v in dev.items()})
        assert max(dev[k] / wc.TOL[k] for k in dev) >= 100.0, (mutate, dev)        # not a near miss


def test_exit_comparison_passes_the_reference_and_fails_its_mutants():
    """Held entries counted in |x| leave on xtol two iterations early; held entries' gradient counted in max |g| never
    leaves on gtol: both fail by iteration count or status.  The unmutated reference passes each exit case."""
    for which in ("gtol", "xtol", "ftol"):
        ref = wc.exit_reference(which)
        wc.follow(*lm_trace.from_oracle(ref), ref, exit_under_test=True)
    early = wc.exit_reference("xtol", "x_all")
    assert (early["status"], early["iterations"]) == ("xtol", wc.XTOL_AT - 2)
    assert _fails(early, wc.exit_reference("xtol"), exit_under_test=True)
    never = wc.exit_reference("gtol", "g_all")
    assert (never["status"], never["iterations"]) == ("max_iters", wc.EXIT_ITERS)
    assert _fails(never, wc.exit_reference("gtol"), exit_under_test=True)
    # and neither mutant is visible where its exit is not under test
    for m in ("x_all", "g_all"):
        assert not _fails(wc.exit_reference("ftol", m), wc.exit_reference("ftol"), exit_under_test=True)


def test_what_the_end_point_criteria_see_of_the_mutants():
    """The suite's end-point check of held windows -- final cost within 1e-9 relative of a correct solver's after 30
    iterations at tolerances 1e-12, held entries untouched (test_window_solvers_serve_held_windows) -- put to the mutants
    on the 5-camera case, on the CPU.  Measured:
      * 'pt_coupled' and 'cam_coupled' do NOT pass it.  A step computed as if the held entries moved along, applied without
        them, stops lowering the cost after five or six iterations: LM rejects, damps and creeps (16 and 12
        rejections in 30 iterations), and the final costs are 7.7e-3 and 0.70 above the correct one.  The end-point check
        sees these two faults, a third of a second of GPU time later and without saying where; step by step they are off
        by 5e-4 and more in a trial cost of the first two iterations (test_step_comparison_passes_the_reference_and_fails_its_mutants).
      * 'x_all' and 'g_all' pass it with the very same bits: with gtol = 0 and xtol = 1e-12 no stopping test fires in 30
        iterations, so whatever |x| and max |g| count is never looked at.  Only the exit cases can see those."""
    shape, loss, f_scale = "c5_p129", "huber", 2.0
    p = wc.step_problem(shape, loss)
    cm, pm = wc.step_masks(shape)
    kw = dict(loss=loss, f_scale=f_scale, max_iters=30, ftol=1e-12, xtol=1e-12, gtol=0.0)
    good = wr.window_lm(p, cm, pm, **kw)
    red = Reduced(p.cams, p.pts, p.cam_idx, p.pt_idx, p.uv, p.K4, p.fixed_cam, cm, pm)
    held = ~red.free
    for mutate in ("pt_coupled", "cam_coupled"):
        bad = wr.window_lm(p, cm, pm, mutate=mutate, **kw)
        print("%s: final cost %.2e above, %d rejected steps" % (mutate, (bad["cost"] - good["cost"]) / good["cost"], 30 - bad["accepted"]))
        assert np.array_equal(red.x_full(bad["cams"], bad["pts"])[held], red.x_full(p.cams, p.pts)[held])
        assert bad["cost"] - good["cost"] > 1e-3 * good["cost"] and bad["accepted"] < good["accepted"] == 30
    for mutate in ("x_all", "g_all"):
        same = wr.window_lm(p, cm, pm, mutate=mutate, **kw)
        assert same["cost"] == good["cost"] and same["iterations"] == 30
        assert np.array_equal(same["cams"], good["cams"]) and np.array_equal(same["pts"], good["pts"])
