"""Times of ba_resect_ransac (output kept in profiles/ransac_times.txt).

    python tools/ransac_times.py [--out FILE]

At C3 (1 000 cameras / 100 000 points / 1 M observations, pinhole) and at BASELINE config 5 on the BAL camera, 30 % of the
pixels replaced by uniform draws over the image, default options otherwise, after a warm-up call:
  * the three kernels of ba_resect_ransac between two HIP events on the solver's stream (ba_time_kernel's
    BA_K_RESECT_RANSAC slot), median of 11 single calls, for n_hyp = 64, 256, 1024;
  * the kernel of ba_resect (BA_K_RESECT, default options) on the same handle, median of 11;
  * the wall time of the whole call with every output copied back, median of 11.
Recorded, not gated: no ratio is required."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS = 11


def problem(name):
    """-> (solver with the problem resident, intr or None, the problem)."""
    from bundle_adjustment_amd import hip_backend
    rng = np.random.default_rng(0)
    s = hip_backend.Solver(0)
    if name == "C3":
        from bundle_adjustment_amd.synthetic import make_config
        p = make_config("C3")
        lo = np.zeros(2)
    else:
        from bundle_adjustment_amd.synthetic import make_bal_problem
        p = make_bal_problem()
        lo = np.array([-640.0, -360.0])
    idx = rng.choice(p.n_obs, size=int(0.3 * p.n_obs), replace=False)
    p.uv[idx] = lo + rng.uniform(0.0, 1.0, size=(len(idx), 2)) * np.array([1280.0, 720.0])
    if name == "C3":
        s.set_problem(p)
        return s, None, p
    return s, s._set_bal(p, 0), p


def measure(name, lines):
    from bundle_adjustment_amd import hip_backend
    s, intr, p = problem(name)
    per_cam = np.bincount(p.cam_idx, minlength=p.n_cams)
    lines.append(f"{name}: {p.n_cams} cameras, {p.n_pts} points, {p.n_obs} observations, 30 % uniform outliers; observations per "
                 f"camera median {int(np.median(per_cam))}, min {per_cam.min()}, max {per_cam.max()}")
    s.resect(intr=intr)
    res = [s.time_kernel(hip_backend.K_RESECT, 1) for _ in range(REPS)]
    t_res = float(np.median(res))
    lines.append(f"{name}: kernel of ba_resect (defaults) {t_res:.1f} us (min {min(res):.1f}, max {max(res):.1f})")
    for n_hyp in (64, 256, 1024):
        out = s.resect_ransac(intr=intr, n_hyp=n_hyp)                      # warm-up, and the statuses
        t = [s.time_kernel(hip_backend.K_RESECT_RANSAC, 1) for _ in range(REPS)]
        wall = []
        for _ in range(REPS):
            t0 = time.perf_counter()
            s.resect_ransac(intr=intr, n_hyp=n_hyp)
            wall.append(time.perf_counter() - t0)
        t_med = float(np.median(t))
        lines.append(f"{name}: n_hyp {n_hyp}: kernels of ba_resect_ransac {t_med:.1f} us (min {min(t):.1f}, max {max(t):.1f}), "
                     f"{t_med / t_res:.1f}x ba_resect, {1e3 * t_med / (n_hyp * p.n_obs):.4f} ns per hypothesis and observation; "
                     f"wall {1e3 * float(np.median(wall)):.2f} ms; status counts {np.bincount(out['status'], minlength=6).tolist()}, "
                     f"inlier share {out['obs_inlier'].mean():.3f}")
    s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ransac_times.txt"))
    a = ap.parse_args()
    lines = []
    for name in ("C3", "C5-BAL"):
        n0 = len(lines)
        measure(name, lines)
        print("\n".join(lines[n0:]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
