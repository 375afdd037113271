#!/usr/bin/env python3
"""What holding parameters (ba_set_held) costs on the device: at C3 (the reference's pinhole, bench.py's headline problem)
and at BASELINE config 5 with the BAL 9-parameter camera (bench.py --config C5 --camera bal), per case:
  nothing held; 10 % of the cameras (whole) and 10 % of the points; every camera's f, k1, k2 (BAL only); every point
  (motion-only BA); every camera (structure-only BA).
Reported: LM it/s over K forced iterations with bench.py's options (every stopping test off, gtol = 1e-300, pcg_tol 0.1, at
most 200 PCG iterations; median of R repeats from the same start), time to solution at the reference's tolerances
(src/bundle_adjuster.py:170-174), LM / PCG iteration counts and the final reprojection RMSE.  Huber loss throughout.
    python tools/held_times.py [K] [R]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bundle_adjustment_amd import hip_backend                      # noqa: E402
from bundle_adjustment_amd.synthetic import make_bal_problem, make_config   # noqa: E402

K = int(sys.argv[1]) if len(sys.argv) > 1 else 20
R = int(sys.argv[2]) if len(sys.argv) > 2 else 5
FORCED = dict(ftol=0.0, xtol=0.0, gtol=1e-300, pcg_tol=0.1, pcg_max_iters=200, max_iters=K)
REFERENCE = dict(ftol=1e-5, xtol=1e-5, gtol=1e-8, pcg_tol=0.1, pcg_max_iters=200, max_iters=50)


def cases(nc, npt, bal):
    rng = np.random.default_rng(0)
    some_c, some_p = rng.random(nc) < 0.1, rng.random(npt) < 0.1
    out = [("nothing", None, None), ("10% cams + 10% pts", some_c, some_p)]
    if bal:
        out.append(("all intrinsics", np.full(nc, 0x1C0, np.uint16), None))
    out += [("all points", None, np.ones(npt, bool)), ("all cameras", np.ones(nc, bool), None)]
    return out


def report(label, n_obs, solve, todo):
    print(f"{label}: {n_obs} observations; forced: {K} LM iterations x {R} repeats (median); to solution: reference tolerances")
    for name, cm, pm in todo:
        solve(cm, pm, FORCED)                                  # warm-up (first launches, allocations)
        runs = [solve(cm, pm, FORCED) for _ in range(R)]
        secs = sorted(r["seconds_total"] for r in runs)[R // 2]
        f = runs[0]
        t0 = time.perf_counter()
        sol = solve(cm, pm, REFERENCE)
        wall = time.perf_counter() - t0
        print(f"  {name:20s} forced: {f['iterations'] / secs:7.1f} LM it/s ({secs / max(1, f['iterations']) * 1e3:6.2f} ms/it, "
              f"{f['pcg_iterations']} PCG)   to solution: {sol['seconds_total'] * 1e3:8.1f} ms (call {wall * 1e3:8.1f} ms), "
              f"{sol['iterations']:2d} LM / {sol['pcg_iterations']:4d} PCG, {sol['status_name']}, "
              f"RMSE {np.sqrt(sol['initial_sse'] / n_obs):.3f} -> {np.sqrt(sol['final_sse'] / n_obs):.4f} px")
    sys.stdout.flush()


with hip_backend.Solver(0) as s:
    p = make_config("C3", seed=0)
    s.set_problem(p)

    def pinhole(cm, pm, kw):
        s.set_held(cm, pm)
        s.set_params(p.cams, p.pts)
        return s.solve(loss="huber", **kw)

    report(f"C3 pinhole ({p.n_cams} cams / {p.n_pts} pts)", p.n_obs, pinhole, cases(p.n_cams, p.n_pts, False))

    bal = make_bal_problem(seed=0)
    intr0 = s.set_problem_bal(bal, fixed_cam=0)

    def balcam(cm, pm, kw):
        s.set_held(cm, pm)
        s.set_params(bal.cams[:, :6], bal.pts)
        return s.solve_bal_resident(intr0.copy(), loss="huber", **kw)

    report(f"config 5, BAL camera ({bal.n_cams} cams / {bal.n_pts} pts)", bal.n_obs, balcam, cases(bal.n_cams, bal.n_pts, True))
