"""Times of ba_triangulate_tracks (output kept in profiles/track_times.txt).

    python tools/track_times.py [--out FILE] [--trace]

At C3 (1 000 cameras / 100 000 points / 1 M observations, pinhole) and at BASELINE config 5 on the BAL camera, with the
default options (linear loss, 20 refinement steps at most) and after a warm-up call:
  * the kernels of ba_triangulate_tracks between two HIP events on the solver's stream (ba_time_kernel's BA_K_TRACKS slot:
    camera centres, the short-track launch, the long-track launch), median of 11 single calls;
  * ba_time_kernel(BA_K_LINEARIZE_PT), one pass over the same point-ordered stream, median of 11;
  * the wall time of the whole call with every output copied back, median of 11;
  * the numpy reference (tests/track_reference.py) on 1 000 points, extrapolated to the problem.
--trace: one more run of the same calls in a child process under `rocprofv3 --kernel-trace --stats`, per-kernel totals
appended (where the time goes when the ratio to the linearisation pass is large)."""
import argparse
import csv
import glob
import os
import subprocess
import sys
import tempfile
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


def inner(name):
    s, intr, _ = problem(name)
    for _ in range(3):
        s.triangulate_tracks(intr=intr, want=False)
    s.synchronize()
    s.close()


def measure(name, lines):
    from bundle_adjustment_amd import hip_backend
    from tests import track_reference as tr
    s, intr, p = problem(name)
    out = s.triangulate_tracks(intr=intr)                                  # warm-up, and the statuses
    lay = s.debug_layout("scalars")
    counts = np.bincount(np.bincount(p.pt_idx, minlength=p.n_pts))
    lines.append(f"{name}: {p.n_cams} cameras, {p.n_pts} points, {p.n_obs} observations; track length median "
                 f"{int(np.median(np.bincount(p.pt_idx)))}, max {len(counts) - 1}; long_thr {lay['long_thr']}, {lay['n_long']} long tracks; "
                 f"status counts {np.bincount(out['status'], minlength=6).tolist()}")
    s.triangulate_tracks(intr=intr, want=False)
    trk = [s.time_kernel(hip_backend.K_TRACKS, 1) for _ in range(REPS)]
    lin = [s.time_kernel(hip_backend.K_LINEARIZE_PT, 1) for _ in range(REPS)]
    wall = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        s.triangulate_tracks(intr=intr)
        wall.append(time.perf_counter() - t0)
    t_trk, t_lin = float(np.median(trk)), float(np.median(lin))
    lines.append(f"{name}: kernels of ba_triangulate_tracks {t_trk:.1f} us (min {min(trk):.1f}, max {max(trk):.1f}); "
                 f"linearize_pt {t_lin:.1f} us (min {min(lin):.1f}, max {max(lin):.1f}); ratio {t_trk / t_lin:.1f}x; "
                 f"{1e-3 * p.n_obs / t_trk:.2f} G observations/s")
    lines.append(f"{name}: wall time of the whole call, five outputs copied back: {1e3 * float(np.median(wall)):.2f} ms")
    s.close()
    sample = np.random.default_rng(0).choice(p.n_pts, size=1000, replace=False)
    t0 = time.perf_counter()
    tr.triangulate_tracks(p, points=sample)
    t_ref = time.perf_counter() - t0
    lines.append(f"{name}: numpy reference {1e3 * t_ref:.0f} ms for 1000 points -> {t_ref * p.n_pts / 1000:.0f} s for the problem, "
                 f"{t_ref * p.n_pts / 1000 / (1e-6 * t_trk):.0f}x the kernels")


def trace(name, lines):
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "trk", "--", sys.executable,
               os.path.abspath(__file__), "--inner", name]
        subprocess.run(cmd, check=True, capture_output=True, timeout=600)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise RuntimeError("no kernel_stats.csv from rocprofv3")
        rows = list(csv.DictReader(open(files[0])))
    for r in rows:
        if "track" in r["Name"]:
            lines.append(f"    {name}: {r['Name'][:80]:80s} {int(r['Calls']):4d} calls, mean {float(r['TotalDurationNs']) / int(r['Calls']) * 1e-3:9.1f} us")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_times.txt"))
    a = ap.parse_args()
    if a.inner:
        inner(a.inner)
        return
    lines = []
    for name in ("C3", "C5-BAL"):
        measure(name, lines)
        if a.trace:
            trace(name, lines)
        print("\n".join(lines), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
