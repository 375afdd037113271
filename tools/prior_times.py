#!/usr/bin/env python3
"""What Gaussian priors (ba_set_priors) cost on the device: at C3 (the reference's pinhole, bench.py's headline problem) and
at BASELINE config 5 with the BAL 9-parameter camera (bench.py --config C5 --camera bal), per case:
  (a) no priors; (b) a prior on every camera; (c) on every camera and 5 % of the points; (d) on every point.
The priors are centred on the start values: cameras sigma 0.01 rad / 0.05 m (BAL: and 2 % of f, 0.01 for k1, 0.003 for k2),
points sigma 0.1 m.  Reported: LM it/s over K forced iterations with bench.py's options (every stopping test off,
gtol = 1e-300, pcg_tol 0.1, at most 200 PCG iterations; median of R repeats from the same start), time to solution at the
reference's tolerances (src/bundle_adjuster.py:170-174), LM / PCG iteration counts and the final reprojection RMSE.  Huber loss.
    python tools/prior_times.py [K] [R]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bundle_adjustment_amd import hip_backend                      # noqa: E402
from bundle_adjustment_amd.priors import info_from_sigma           # noqa: E402
from bundle_adjustment_amd.synthetic import make_bal_problem, make_config   # noqa: E402

K = int(sys.argv[1]) if len(sys.argv) > 1 else 20
R = int(sys.argv[2]) if len(sys.argv) > 2 else 5
FORCED = dict(ftol=0.0, xtol=0.0, gtol=1e-300, pcg_tol=0.1, pcg_max_iters=200, max_iters=K)
REFERENCE = dict(ftol=1e-5, xtol=1e-5, gtol=1e-8, pcg_tol=0.1, pcg_max_iters=200, max_iters=50)


def cases(cams, pts):
    nc, nb = cams.shape
    npt = pts.shape[0]
    sig = np.array([0.01] * 3 + [0.05] * 3 + [0.02 * float(np.mean(cams[:, 6])) if nb == 9 else 1.0, 0.01, 0.003])[:nb]
    cam_all = (cams, np.broadcast_to(info_from_sigma(sig), (nc, nb, nb)).copy())
    pt_info = np.broadcast_to(info_from_sigma([0.1, 0.1, 0.1]), (npt, 3, 3)).copy()
    some = pt_info * (np.random.default_rng(0).random(npt) < 0.05)[:, None, None]
    return [("(a) none", None, None), ("(b) every camera", cam_all, None), ("(c) cameras + 5% pts", cam_all, (pts, some)),
            ("(d) every point", None, (pts, pt_info))]


def report(label, n_obs, set_priors, solve, todo):
    print(f"{label}: {n_obs} observations; forced: {K} LM iterations x {R} repeats (median); to solution: reference tolerances")
    for name, cp, pp in todo:
        set_priors(cp, pp)
        solve(FORCED)                                          # warm-up (first launches, allocations)
        runs = [solve(FORCED) for _ in range(R)]
        secs = sorted(r["seconds_total"] for r in runs)[R // 2]
        f = runs[0]
        t0 = time.perf_counter()
        sol = solve(REFERENCE)
        wall = time.perf_counter() - t0
        print(f"  {name:22s} forced: {f['iterations'] / secs:7.1f} LM it/s ({secs / max(1, f['iterations']) * 1e3:6.2f} ms/it, "
              f"{f['pcg_iterations']} PCG)   to solution: {sol['seconds_total'] * 1e3:8.1f} ms (call {wall * 1e3:8.1f} ms), "
              f"{sol['iterations']:2d} LM / {sol['pcg_iterations']:4d} PCG, {sol['status_name']}, "
              f"RMSE {np.sqrt(sol['initial_sse'] / n_obs):.3f} -> {np.sqrt(sol['final_sse'] / n_obs):.4f} px")
        sys.stdout.flush()


with hip_backend.Solver(0) as s:
    p = make_config("C3", seed=0)
    s.set_problem(p)

    def pinhole(kw):
        s.set_params(p.cams, p.pts)
        return s.solve(loss="huber", **kw)

    report(f"C3 pinhole ({p.n_cams} cams / {p.n_pts} pts)", p.n_obs, s.set_priors, pinhole, cases(p.cams, p.pts))

    bal = make_bal_problem(seed=0)
    intr0 = s.set_problem_bal(bal, fixed_cam=0)

    def balcam(kw):
        s.set_params(bal.cams[:, :6], bal.pts)
        return s.solve_bal_resident(intr0.copy(), loss="huber", **kw)

    report(f"config 5, BAL camera ({bal.n_cams} cams / {bal.n_pts} pts)", bal.n_obs, s.set_priors, balcam, cases(bal.cams, bal.pts))
