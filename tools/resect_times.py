"""Times of ba_resect (output kept in profiles/resect_times.txt).

    python tools/resect_times.py [--out FILE]

At C3 (1 000 cameras / 100 000 points / 1 M observations, pinhole) and at BASELINE config 5 on the BAL camera, with the
default options (DLT start, linear loss, 20 refinement steps at most, every camera, every point) and after a warm-up call:
  * the kernel of ba_resect between two HIP events on the solver's stream (ba_time_kernel's BA_K_RESECT slot), median of
    11 single calls;
  * ba_time_kernel(BA_K_LINEARIZE_CAM), one pass over the same camera-ordered stream, median of 11;
  * the wall time of the whole call with every output copied back, median of 11;
  * the numpy reference (tests/resect_reference.py) on 20 cameras, per camera and extrapolated to the problem.
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
    s = hip_backend.Solver(0)
    if name == "C3":
        from bundle_adjustment_amd.synthetic import make_config
        p = make_config("C3")
        s.set_problem(p)
        return s, None, p
    from bundle_adjustment_amd.synthetic import make_bal_problem
    b = make_bal_problem()
    return s, s._set_bal(b, 0), b


def measure(name, lines):
    from bundle_adjustment_amd import hip_backend
    from tests import resect_reference as rr
    s, intr, p = problem(name)
    out = s.resect(intr=intr)                                              # warm-up, and the statuses
    per_cam = np.bincount(p.cam_idx, minlength=p.n_cams)
    lines.append(f"{name}: {p.n_cams} cameras, {p.n_pts} points, {p.n_obs} observations; observations per camera median "
                 f"{int(np.median(per_cam))}, min {per_cam.min()}, max {per_cam.max()}; status counts "
                 f"{np.bincount(out['status'], minlength=6).tolist()}; median rms {np.nanmedian(out['rms_px']):.3f} px")
    res = [s.time_kernel(hip_backend.K_RESECT, 1) for _ in range(REPS)]
    lin = [s.time_kernel(hip_backend.K_LINEARIZE_CAM, 1) for _ in range(REPS)]
    wall = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        s.resect(intr=intr)
        wall.append(time.perf_counter() - t0)
    t_res, t_lin = float(np.median(res)), float(np.median(lin))
    lines.append(f"{name}: kernel of ba_resect {t_res:.1f} us (min {min(res):.1f}, max {max(res):.1f}); "
                 f"linearize_cam {t_lin:.1f} us (min {min(lin):.1f}, max {max(lin):.1f}); ratio {t_res / t_lin:.1f}x; "
                 f"{t_res / p.n_cams:.3f} us per camera")
    lines.append(f"{name}: wall time of the whole call, five outputs copied back: {1e3 * float(np.median(wall)):.2f} ms")
    s.close()
    sample = np.random.default_rng(0).choice(p.n_cams, size=20, replace=False)
    t0 = time.perf_counter()
    rr.resect_cameras(p, cams=sample)
    t_ref = (time.perf_counter() - t0) / len(sample)
    lines.append(f"{name}: numpy reference {1e3 * t_ref:.1f} ms per camera -> {t_ref * p.n_cams:.1f} s for the problem, "
                 f"{t_ref * p.n_cams / (1e-6 * t_res):.0f}x the kernel")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resect_times.txt"))
    a = ap.parse_args()
    lines = []
    for name in ("C3", "C5-BAL"):
        measure(name, lines)
        print("\n".join(lines[-4:]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
