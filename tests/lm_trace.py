"""Two checkers of an LM solve's per-iteration records (Solver.trace()) and summary.  Test infrastructure only.

check_self_consistent needs no reference: the records obey the driver's documented rules among themselves (verdict, the
cost carried over, Nielsen's damping with the floor of capped inner solves, the summary's sums).  check_follows compares
them with oracle.lm_solve's history, iteration by iteration and at the exit.  from_oracle turns the mirror's own result
into (summary, trace), so both checkers can be run -- and shown to fail on faulty drivers -- without a GPU."""
import math

DEFAULT_PCG_MAX_ITERS = 200         # ba_default_options
DEFAULT_INITIAL_LAMBDA = 1e-4
STATUS_CODE = {"max_iters": 0, "ftol": 1, "xtol": 2, "gtol": 3}
# relative, from the window solver's comparison (test_gpu_small.py): 1e-6 on the damping, 1e-7 on the step norm (absolute
# floor 1e-12); 1e-6 on the gain ratio and the trial cost
TOL = dict(damping=1e-6, gain_ratio=1e-6, step_norm=1e-7, cost_trial=1e-6)
STEP_FLOOR = 1e-12
ROUND_OFF_STOP = 1e-8               # |cost - cost_new| <= this * cost: accept / reject is decided by round-off from here on


def _ulps(a, b):
    if a == b:
        return 0.0
    if not (math.isfinite(a) and math.isfinite(b)):
        return math.inf
    return abs(a - b) / math.ulp(max(abs(a), abs(b)))


def next_damping(lam, rho, accepted, nu, floor):
    """The driver's rule (LM section): -> (damping of the next iteration, nu of the next rejection)."""
    if accepted:
        t = 2.0 * rho - 1.0
        return max(lam * max(1.0 / 3.0, 1.0 - t * t * t), 1e-12, floor), 2.0
    return min(lam * nu, 1e12), 2.0 * nu


def check_self_consistent(summary, trace, opts):
    """summary / trace: Solver.solve(...) (or solve_bal(...)[0]) and Solver.trace(); opts: the options given to the solve
    (pcg_max_iters and initial_lambda are read; the library's defaults where absent).  Raises AssertionError."""
    cap = opts.get("pcg_max_iters", DEFAULT_PCG_MAX_ITERS)
    lam = opts.get("initial_lambda", DEFAULT_INITIAL_LAMBDA)
    nu, floor = 2.0, 0.0
    cost = summary["initial_cost"]
    for i, r in enumerate(trace):
        where = f"record {i}: {r}"
        assert r["iteration"] == i + 1, where
        assert bool(r["accepted"]) == (r["gain_ratio"] > 0 and math.isfinite(r["cost_trial"])), where
        assert r["cost"] == cost, f"{where}: cost is not the one carried over ({cost!r})"
        if i == 0:
            assert r["damping"] == lam, f"{where}: the first damping is not initial_lambda {lam!r}"
        else:
            assert _ulps(r["damping"], lam) <= 4, f"{where}: the rule gives damping {lam!r} (floor {floor!r})"
        if r["pcg_iterations"] >= cap:
            floor = max(floor, 3.0 * r["damping"])
        lam, nu = next_damping(r["damping"], r["gain_ratio"], r["accepted"], nu, floor)
        if r["accepted"]:
            cost = r["cost_trial"]
    assert _ulps(summary["final_lambda"], lam) <= 4, f"final_lambda {summary['final_lambda']!r}: the rule gives {lam!r}"
    assert summary["iterations"] == len(trace), (summary["iterations"], len(trace))
    assert summary["accepted"] == sum(bool(r["accepted"]) for r in trace)
    assert summary["pcg_iterations"] == sum(r["pcg_iterations"] for r in trace)
    assert summary["final_cost"] == cost, f"final_cost {summary['final_cost']!r}: the last accepted trial cost is {cost!r}"


def _rel(a, b, floor=0.0):
    return abs(a - b) / max(abs(b), floor, 1e-300)


def deviations(trace, ref, exit_under_test=False):
    """-> (compared, dev): how many leading iterations are comparable (all of the shorter sequence, or -- no tolerance exit
    under test -- up to the first the mirror's round-off decides), and the largest relative deviation per quantity there."""
    dev = dict(damping=0.0, gain_ratio=0.0, step_norm=0.0, cost_trial=0.0)
    compared = 0
    for t, h in zip(trace, ref["history"]):
        if not exit_under_test and abs(h["cost"] - h["cost_new"]) <= ROUND_OFF_STOP * h["cost"]:
            break
        dev["damping"] = max(dev["damping"], _rel(t["damping"], h["lam"]))
        dev["gain_ratio"] = max(dev["gain_ratio"], _rel(t["gain_ratio"], h["rho"]))
        dev["step_norm"] = max(dev["step_norm"], _rel(t["step_norm"], h["step"], STEP_FLOOR))
        dev["cost_trial"] = max(dev["cost_trial"], _rel(t["cost_trial"], h["cost_new"]))
        compared += 1
    return compared, dev


def check_follows(summary, trace, ref, tol=TOL, exit_under_test=False):
    """The records against oracle.lm_solve's result `ref`: per iteration the PCG count and the verdict equal, damping, gain
    ratio, step norm and trial cost within tol (relative); where every iteration of the mirror was compared, also the exit:
    status, iteration count, accepted steps and final_lambda.  Returns (compared, dev) as deviations(); prints dev first."""
    compared, dev = deviations(trace, ref, exit_under_test)
    print("lm_trace: compared %d iterations; largest relative deviation: %s" % (compared, ", ".join(f"{k} {v:.2e}" for k, v in dev.items())))
    for t, h in list(zip(trace, ref["history"]))[:compared]:
        where = f"device {t}\nmirror {h}"
        assert t["pcg_iterations"] == h["pcg"], where
        assert bool(t["accepted"]) == bool(h["rho"] > 0 and math.isfinite(h["cost_new"])), where
        assert _rel(t["damping"], h["lam"]) <= tol["damping"], where
        assert _rel(t["gain_ratio"], h["rho"]) <= tol["gain_ratio"], where
        assert _rel(t["step_norm"], h["step"], STEP_FLOOR) <= tol["step_norm"], where
        assert _rel(t["cost_trial"], h["cost_new"]) <= tol["cost_trial"], where
    if compared == len(ref["history"]):
        assert summary["status"] == STATUS_CODE[ref["status"]], (summary["status"], ref["status"])
        assert summary["iterations"] == ref["iterations"], (summary["iterations"], ref["iterations"])
        assert summary["accepted"] == ref["accepted"], (summary["accepted"], ref["accepted"])
        assert summary["pcg_iterations"] == ref["pcg_iters"], (summary["pcg_iterations"], ref["pcg_iters"])
        assert _rel(summary["final_lambda"], ref["lam"]) <= tol["damping"], (summary["final_lambda"], ref["lam"])
    return compared, dev


def from_oracle(ref):
    """oracle.lm_solve's result as the device would report it: (summary, trace)."""
    trace = [dict(iteration=h["it"], accepted=bool(h["rho"] > 0 and math.isfinite(h["cost_new"])), pcg_iterations=h["pcg"], cost=h["cost"],
                  cost_trial=h["cost_new"], damping=h["lam"], gain_ratio=h["rho"], step_norm=h["step"]) for h in ref["history"]]
    summary = dict(iterations=ref["iterations"], accepted=ref["accepted"], pcg_iterations=ref["pcg_iters"], status=STATUS_CODE[ref["status"]],
                   initial_cost=ref["cost0"], final_cost=ref["cost"], final_lambda=ref["lam"])
    return summary, trace
