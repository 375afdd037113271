#!/usr/bin/env python3
"""What shared intrinsics (ba_set_shared_intrinsics) cost on the device, at BASELINE config 5's size with the BAL camera and
data from a shared truth (synthetic.make_shared_bal_problem: 1723 cameras / 156 502 points / ~662 k observations; one problem
per case, the case's own groups in the truth).  Cases: (a) no groups; (b) ONE group of all cameras; (c) 8 interleaved groups
(camera c in group c mod 8).  Camera 0's pose is held by mask in every case.  Reported per case: LM it/s over K forced
iterations with bench.py's options (every stopping test off, gtol = 1e-300, pcg_tol 0.1, at most 200 PCG iterations; median
of R repeats from the same start), PCG iterations per LM iteration, us per PCG iteration (the solve's seconds_pcg over its
PCG iterations), and the time to solution at the reference's tolerances (src/bundle_adjuster.py:170-174).  Huber loss.
    python tools/shared_times.py [K] [R]          -> profiles/shared_times.txt
    python tools/shared_times.py --trace a|b|c K  one forced solve of that case and nothing else (the run rocprofv3 traces)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bundle_adjustment_amd import hip_backend                      # noqa: E402
from bundle_adjustment_amd.synthetic import make_shared_bal_problem   # noqa: E402

SIZE = (1723, 156502, 678718)
REFERENCE = dict(ftol=1e-5, xtol=1e-5, gtol=1e-8, pcg_tol=0.1, pcg_max_iters=200, max_iters=50)


CASES = (("a", None), ("b", True), ("c", np.arange(SIZE[0]) % 8))
NAMES = {"a": "(a) no groups", "b": "(b) one group of all", "c": "(c) 8 interleaved groups"}


def forced(k):
    return dict(ftol=0.0, xtol=0.0, gtol=1e-300, pcg_tol=0.1, pcg_max_iters=200, max_iters=k)


def case(s, groups):
    bal, lab = make_shared_bal_problem(groups, *SIZE, seed=0)
    intr0 = s.set_problem_bal(bal)
    mask = np.zeros(bal.n_cams, np.uint16)
    mask[0] = 0x3F
    s.set_held(mask)
    s.set_shared_intrinsics(lab)

    def solve(kw):
        s.set_params(bal.cams[:, :6], bal.pts)
        return s.solve_bal_resident(intr0.copy(), loss="huber", **kw)

    return bal, solve


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--trace":
        which = sys.argv[2] if len(sys.argv) > 2 else "b"
        k = int(sys.argv[3]) if len(sys.argv) > 3 else 10
        with hip_backend.Solver(0) as s:
            _, solve = case(s, dict(CASES)[which])
            out = solve(forced(k))
            print(f"case ({which}): {out['iterations']} LM / {out['pcg_iterations']} PCG iterations")
        return
    K = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    R = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    lines = []

    def say(t):
        print(t)
        sys.stdout.flush()
        lines.append(t)

    say(f"config 5 size, BAL camera, shared-truth data, Huber; forced: {K} LM iterations x {R} repeats (median); to solution: reference tolerances")
    with hip_backend.Solver(0) as s:
        for which, groups in CASES:
            name = NAMES[which]
            bal, solve = case(s, groups)
            solve(forced(K))                                       # warm-up (first launches, allocations)
            runs = sorted((solve(forced(K)) for _ in range(R)), key=lambda r: r["seconds_total"])
            f = runs[R // 2]
            sol = solve(REFERENCE)
            say(f"  {name:26s} groups {s.stats()['shared_groups']}  forced: {f['iterations'] / f['seconds_total']:7.1f} LM it/s, "
                f"{f['pcg_iterations'] / max(1, f['iterations']):6.1f} PCG/LM, {1e6 * f['seconds_pcg'] / max(1, f['pcg_iterations']):6.1f} us/PCG it   "
                f"to solution: {sol['seconds_total'] * 1e3:8.1f} ms, {sol['iterations']:2d} LM / {sol['pcg_iterations']:4d} PCG, {sol['status_name']}, "
                f"RMSE {np.sqrt(sol['initial_sse'] / bal.n_obs):.3f} -> {np.sqrt(sol['final_sse'] / bal.n_obs):.4f} px")
    with open(os.path.join(ROOT, "profiles", "shared_times.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
