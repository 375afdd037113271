"""GPU: the two single-launch window solvers -- k_small_lm (csrc/ba_small.hpp) and k_small_mw<2|3|4>
(csrc/ba_small_mw.hpp), where every BundleAdjuster.run lands -- under held parameters (ba_set_held), each of the five
losses and f_scale, iteration by iteration against tests/window_reference.window_lm: a float64 dense LM over the free
columns that knows no Schur complement.  Per iteration the verdict is equal, damping and gain ratio agree to 1e-6, the
step norm to 1e-7, cost and trial cost to 1e-9; then the exit (status, iterations, accepted steps, final damping), the
final parameters to 1e-7 max(1, |x|), and the held entries bit for bit.  tests/test_window_reference_host.py shows on
the CPU that every case is conditioned for these tolerances (its first step solved two ways agrees 100 x, its whole run
driven two ways 10 x better than they ask), that none of its iterations is decided by round-off, and that a kernel with
a held point left in the system, a held camera parameter whose row is not the identity, a weight that ignores f_scale,
or a stopping test that counts held entries fails these very comparisons.
Measured on an MI355X, the largest over every case and both kernels: damping 1.2e-9, gain ratio 1.1e-8, step norm 1.0e-8,
trial cost 9.6e-11 (relative), parameters 1.2e-11 max(1, |x|): a decade and more inside each tolerance.

Which case (tests/window_cases.py) reaches which instantiation; every one under both kinds of mask and all of
linear, huber, soft_l1, cauchy, arctan at f_scale 2 and huber at f_scale 0.5:

  case          cameras / points   k_small_lm (BA_SMALL_MW=0)                  k_small_mw (BA_SMALL_MW=1)
  c2_p37        2 / 37             1 tile row, small_syrk<1>                   <2>, 1 workgroup
  c4_p65        4 / 65             2 tile rows, small_syrk<2>                  <2>, 2 workgroups, the second one's only landmark held
  c5_p129       5 / 129            2 tile rows (30 + 1 rows)                   <2>, 3 workgroups
  c3_p130_dup   3 / 130 (+5 obs)   2 tile rows, repeated (camera, point) pairs -- (not its case)
  c7_p200       7 / 200            3 tile rows, small_syrk<3>                  <3>, 4 workgroups
  c6_p520       6 / 520            3 tile rows, more points than threads,      <3>, 9 workgroups, the last one held entirely
                                   held points at 512 .. 519, shuffled observations
  c8_p130       8 / 130            4 tile rows, small_syrk<4> (z row alone)    <4>, 3 workgroups
  rejected      5 / 200            streaks of 4 (cauchy) and 5 (soft_l1) rejected steps on one linearisation      (both)
  exits         6 / 150            gtol, xtol, ftol with 70 % of the points and 9 camera parameters held           (both)
  reuse         5 / 97             masks set, cleared and set again on one handle; V's 16-column padding         (both)

Each solve is one kernel launch of well under a millisecond; the reference runs (numpy, cached in window_cases) are what
the seconds of this file go to."""
import numpy as np
import pytest

from bundle_adjustment_amd import hip_backend
from tests import lm_trace
from tests import window_cases as wc
from tests.held_reference import Reduced

pytestmark = pytest.mark.gpu
KERNELS = [("1", "window_mw_launches"), ("0", "window_lm_launches")]
KERNEL_IDS = ["k_small_mw", "k_small_lm"]
STEP_IDS = [f"{s}-{l}-{f}" for s, l, f in wc.STEP_CASES]


def _solve(s, monkeypatch, mw, stat, **opts):
    """One window solve on handle s through the kernel asked for -> (summary, trace, cams, pts, (residuals, sse, cost))."""
    monkeypatch.setenv("BA_SMALL_MW", mw)
    before = s.stats()
    out = s.solve(**opts)
    after = s.stats()
    assert out["pcg_iterations"] == 0
    for key in ("window_mw_launches", "window_lm_launches", "window_fallbacks"):        # that kernel, once, and no other
        assert after[key] == before[key] + (1 if key == stat else 0), (key, before[key], after[key])
    tr = s.trace()
    cams, pts = s.get_params()
    return out, tr, cams, pts, s.residuals(opts["loss"], opts.get("f_scale", 1.0))


def _held_and_final(p, cm, pm, out, cams, pts, res, ref, sse_too=True):
    """Held entries (the fixed camera included) bit-equal to the input; the summary describes the parameters the handle
    holds; those are the reference's.  sse_too: the final SSE is the reference's as well (not in the rejected-steps cases:
    test_window_reference_host.py shows it is not conditioned for that there)."""
    red = Reduced(p.cams, p.pts, p.cam_idx, p.pt_idx, p.uv, p.K4, p.fixed_cam, cm, pm)
    held = ~red.free
    assert held.sum() > 6
    assert np.array_equal(red.x_full(cams, pts)[held], red.x_full(p.cams, p.pts)[held])
    _, sse, cost = res
    assert abs(sse - out["final_sse"]) <= 1e-10 * sse and abs(cost - out["final_cost"]) <= 1e-10 * cost, (sse, cost, out)
    assert not sse_too or abs(out["final_sse"] - ref["sse"]) <= wc.COST_TOL * ref["sse"]
    worst = wc.params_agree(cams, pts, ref)
    print("parameters: %.2e of the tolerance" % worst)
    assert worst <= 1.0


@pytest.mark.parametrize("shape,loss,f_scale", wc.STEP_CASES, ids=STEP_IDS)
def test_window_kernels_follow_the_dense_reference_step_by_step(monkeypatch, shape, loss, f_scale):
    p = wc.step_problem(shape, loss)
    cm, pm = wc.step_masks(shape)
    ref = wc.step_reference(shape, loss, f_scale)
    opts = dict(loss=loss, f_scale=f_scale, max_iters=wc.iters(loss), **wc.OFF)
    with hip_backend.Solver(0) as s:
        for mw, stat in (KERNELS[1:] if shape in wc.LM_ONLY else KERNELS):
            s.set_problem(p)
            s.set_held(cm, pm)
            out, tr, cams, pts, res = _solve(s, monkeypatch, mw, stat, **opts)
            lm_trace.check_self_consistent(out, tr, opts)
            wc.follow(out, tr, ref)
            assert out["status_name"] == "max_iters" and out["iterations"] == wc.iters(loss)
            _held_and_final(p, cm, pm, out, cams, pts, res, ref)


@pytest.mark.parametrize("mw,stat", KERNELS, ids=KERNEL_IDS)
@pytest.mark.parametrize("loss", wc.REJECTED_GPU_LOSSES)
def test_rejected_steps_under_masks_follow_the_reference(monkeypatch, loss, mw, stat):
    """A start 3 m, 0.2 rad and 1 m from the truth at initial_lambda 1e-6: cauchy rejects the first four steps, soft_l1 the
    first five -- the same linearisation, the point half re-damped, nu doubling -- then the descent starts.  Verdict,
    damping, gain ratio, step norm and trial cost of every iteration (cauchy six, soft_l1 ten)."""
    p = wc.rejected_problem(loss)
    cm, pm = wc.rejected_masks()
    ref = wc.rejected_reference(loss)
    opts = dict(loss=loss, f_scale=2.0, max_iters=wc.REJECTED_ITERS[loss], initial_lambda=wc.REJECTED_LAMBDA, **wc.OFF)
    with hip_backend.Solver(0) as s:
        s.set_problem(p)
        s.set_held(cm, pm)
        out, tr, cams, pts, res = _solve(s, monkeypatch, mw, stat, **opts)
    lm_trace.check_self_consistent(out, tr, opts)
    wc.follow(out, tr, ref)
    assert [t["accepted"] for t in tr] == [h["rho"] > 0 for h in ref["history"]]
    assert not any(t["accepted"] for t in tr[:4]) and out["accepted"] == ref["accepted"] >= 2
    _held_and_final(p, cm, pm, out, cams, pts, res, ref, sse_too=False)


@pytest.mark.parametrize("mw,stat", KERNELS, ids=KERNEL_IDS)
@pytest.mark.parametrize("which", ["gtol", "xtol", "ftol"])
def test_exits_under_masks_fire_at_the_references_iteration(monkeypatch, which, mw, stat):
    """The stopping tests see the free parameters only.  The threshold sits between the tested quantity's values at two
    adjacent iterations of the reference (window_cases.exit_thresholds).  gtol: max |g| over the free entries falls below
    it after 4 iterations while the held entries' gradient stays five times above -- a kernel that counts them never
    leaves; xtol: the reference leaves in iteration 6, with the held 40 % of |x| counted a kernel leaves in iteration 4;
    ftol: iteration 5.  status, iterations, accepted and final_lambda are the reference's, and so is every iteration before."""
    p, cm, pm = wc.exit_problem()
    ref = wc.exit_reference(which)
    opts = dict(loss=wc.EXIT_LOSS, f_scale=1.0, max_iters=wc.EXIT_ITERS, **dict(wc.OFF, **{which: wc.exit_thresholds()[which]}))
    with hip_backend.Solver(0) as s:
        s.set_problem(p)
        s.set_held(cm, pm)
        out, tr, cams, pts, res = _solve(s, monkeypatch, mw, stat, **opts)
    lm_trace.check_self_consistent(out, tr, opts)
    wc.follow(out, tr, ref, exit_under_test=True)
    assert out["status_name"] == ref["status"] == which
    assert out["iterations"] == ref["iterations"] == dict(gtol=wc.GTOL_AFTER, xtol=wc.XTOL_AT, ftol=wc.FTOL_AT)[which]
    assert out["accepted"] == ref["accepted"]
    assert abs(out["final_lambda"] - ref["lam"]) <= wc.TOL["damping"] * ref["lam"]
    _held_and_final(p, cm, pm, out, cams, pts, res, ref)


@pytest.mark.parametrize("mw,stat", KERNELS, ids=KERNEL_IDS)
def test_masks_come_and_go_on_a_reused_handle(monkeypatch, mw, stat):
    """One handle: a held solve, set_held() to clear, the start point again and a free solve -- bit-equal to a fresh handle
    that never had masks; then the masks again -- bit-equal to the first held solve.  97 points: the last slab of V has 15
    columns of padding, which a held solve must leave as a free one needs them (and the other way round)."""
    p = wc.reuse_problem()
    cm, pm = wc.masks(p.n_cams, p.n_pts, p.fixed_cam)
    opts = dict(loss="huber", f_scale=2.0, max_iters=6, **wc.OFF)

    def bits(r):
        out, tr, cams, pts, _ = r
        return (out["final_cost"], out["final_sse"], out["final_lambda"], [(t["accepted"], t["cost_trial"], t["gain_ratio"], t["step_norm"]) for t in tr],
                cams.tobytes(), pts.tobytes())

    with hip_backend.Solver(0) as fresh:
        fresh.set_problem(p)
        free_want = _solve(fresh, monkeypatch, mw, stat, **opts)
    with hip_backend.Solver(0) as s:
        s.set_problem(p)
        s.set_held(cm, pm)
        held_first = _solve(s, monkeypatch, mw, stat, **opts)
        s.set_held()
        s.set_params(p.cams, p.pts)
        free_got = _solve(s, monkeypatch, mw, stat, **opts)
        s.set_held(cm, pm)
        s.set_params(p.cams, p.pts)
        held_again = _solve(s, monkeypatch, mw, stat, **opts)
    assert bits(free_got) == bits(free_want)
    assert bits(held_again) == bits(held_first)
    assert held_first[0]["final_cost"] > free_want[0]["final_cost"]                     # the masks did something
    red = Reduced(p.cams, p.pts, p.cam_idx, p.pt_idx, p.uv, p.K4, p.fixed_cam, cm, pm)
    held = ~red.free
    assert np.array_equal(red.x_full(held_again[2], held_again[3])[held], red.x_full(p.cams, p.pts)[held])
    assert not np.array_equal(red.x_full(free_got[2], free_got[3])[held], red.x_full(p.cams, p.pts)[held])
