#!/usr/bin/env python3
"""What each of scipy's losses costs on the device: at C3 (the reference's pinhole, bench.py's headline problem) and at
BASELINE config 5 with the BAL 9-parameter camera (bench.py --config C5 --camera bal), per loss:
  - LM it/s over K forced iterations with bench.py's options (every stopping test off, gtol = 1e-300, pcg_tol 0.1,
    at most 200 PCG iterations; median of R repeats from the same start);
  - time to solution at the reference's tolerances (src/bundle_adjuster.py:170-174: ftol = xtol = 1e-5, 50 iterations);
  - LM / PCG iteration counts of both, and the final reprojection RMSE.
The smooth losses (soft_l1, cauchy, arctan) give almost every observation a weight other than 1, so every index of the
flagged streams is flagged and the Schur passes fetch every weight; Huber flags only its outliers.
    python tools/loss_times.py [K] [R]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bundle_adjustment_amd import hip_backend                      # noqa: E402
from bundle_adjustment_amd.synthetic import make_bal_problem, make_config   # noqa: E402

K = int(sys.argv[1]) if len(sys.argv) > 1 else 20
R = int(sys.argv[2]) if len(sys.argv) > 2 else 5
LOSSES = ("linear", "huber", "soft_l1", "cauchy", "arctan")
FORCED = dict(ftol=0.0, xtol=0.0, gtol=1e-300, pcg_tol=0.1, pcg_max_iters=200, max_iters=K)
REFERENCE = dict(ftol=1e-5, xtol=1e-5, gtol=1e-8, pcg_tol=0.1, pcg_max_iters=200, max_iters=50)


def report(label, n_obs, solve):
    print(f"{label}: {n_obs} observations; forced: {K} LM iterations x {R} repeats (median); to solution: reference tolerances")
    for loss in LOSSES:
        solve(loss, FORCED)                                   # warm-up (first launches, allocations)
        runs = []
        for _ in range(R):
            out = solve(loss, FORCED)
            runs.append(out)
        secs = sorted(r["seconds_total"] for r in runs)[R // 2]
        f = runs[0]
        t0 = time.perf_counter()
        sol = solve(loss, REFERENCE)
        wall = time.perf_counter() - t0
        print(f"  {loss:8s} forced: {K / secs:7.1f} LM it/s ({secs / K * 1e3:6.2f} ms/it, {f['pcg_iterations']} PCG)   "
              f"to solution: {sol['seconds_total'] * 1e3:8.1f} ms (call {wall * 1e3:8.1f} ms), {sol['iterations']:2d} LM / "
              f"{sol['pcg_iterations']:4d} PCG, {sol['status_name']}, RMSE {np.sqrt(sol['initial_sse'] / n_obs):.3f} -> "
              f"{np.sqrt(sol['final_sse'] / n_obs):.4f} px")
    sys.stdout.flush()


with hip_backend.Solver(0) as s:
    p = make_config("C3", seed=0)
    s.set_problem(p)

    def pinhole(loss, kw):
        s.set_params(p.cams, p.pts)
        return s.solve(loss=loss, **kw)

    report(f"C3 pinhole ({p.n_cams} cams / {p.n_pts} pts)", p.n_obs, pinhole)

    bal = make_bal_problem(seed=0)
    intr0 = s.set_problem_bal(bal, fixed_cam=0)

    def balcam(loss, kw):
        s.set_params(bal.cams[:, :6], bal.pts)
        return s.solve_bal_resident(intr0.copy(), loss=loss, **kw)

    report(f"config 5, BAL camera ({bal.n_cams} cams / {bal.n_pts} pts)", bal.n_obs, balcam)
