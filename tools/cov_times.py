"""Stage times of ba_covariance (output kept in profiles/cov_times.txt).

    python tools/cov_times.py [--out FILE]

For C3 (pinhole, N = 6000) and config 5 on the BAL camera (N = 15507), gauge fixed by fixed_cam 0 plus t[0] of camera 1:
  * per-stage GPU time from one `rocprofv3 --kernel-trace --stats` run of a child process that makes one call
    (assembly: linearisation + S; factorisation: potrf; inverse: trtri + lauum; points; copy-out kernels);
  * wall time of the whole call (mean of 3 after a warm-up, outputs cam_cov + pt_cov + cam_full);
  * the achieved rate of the trailing-update kernel against the v_mfma_f64_16x16x4f64 issue rate measured by
    tools/microbench/mfma_f64_rate.hip (one per 32 shader clocks per SIMD with two waves; 2048 flop each);
  * scipy.linalg.lapack dpotrf + dpotri of the returned Sigma (same N, same flop count) on this host's CPUs.
Then the pivot ratios of the rank test: the smallest rcond at which each problem is refused, found by bisection, for the
tests' gauge-fixed / gauge-free problems and config 5."""
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

MFMA_FLOP, MFMA_CLK_PER_SIMD, SIMD_PER_CU, CLOCK_GHZ = 2048, 32, 4, 2.4
STAGES = [("assembly", ("k_camrow_linearize", "k_lin_finalize", "k_pt_linearize", "k_held_points", "k_cov_points", "k_cov_diag",
                        "k_cov_w", "k_cov_pairs", "k_cov_held", "k_cov_save_diag")),
          ("factorisation", ("k_cov_potrf",)), ("inverse", ("k_cov_trtri", "k_cov_lauum")), ("points", ("k_cov_point_cov",)),
          ("copy-out", ("k_cov_cam_blocks", "k_cov_symmetrize", "k_unpermute_rows"))]


def problem(name):
    from bundle_adjustment_amd import hip_backend
    from bundle_adjustment_amd.problem import BAProblem
    s = hip_backend.Solver(0)
    if name == "C3":
        from bundle_adjustment_amd.synthetic import make_config
        p = make_config("C3")
        s.set_problem(BAProblem(p.cams, p.pts, p.cam_idx, p.pt_idx, p.uv, p.K4, 0))
        intr, nc = None, p.n_cams
    else:
        from bundle_adjustment_amd.synthetic import make_bal_problem
        b = make_bal_problem()
        intr, nc = s._set_bal(b, 0), b.n_cams
    m = np.zeros(nc, np.uint16)
    m[1] = 1 << 3
    s.set_held(cams=m)
    return s, intr


def inner(name):
    s, intr = problem(name)
    s.covariance(intr=intr, full=True)
    s.synchronize()


def wall_and_cpu(name, lines):
    s, intr = problem(name)
    out = s.covariance(intr=intr, full=True)
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        out = s.covariance(intr=intr, full=True)
        ts.append(time.perf_counter() - t0)
    n = out["full"].shape[0]
    lines.append(f"{name}: N = {n}, wall time of ba_covariance (cam_cov + pt_cov + cam_full) {1e3 * np.mean(ts):.1f} ms "
                 f"(min {1e3 * min(ts):.1f})")
    s.close()
    from scipy.linalg import lapack
    held = np.diagonal(out["full"]) == 0
    A = out["full"][~held][:, ~held].copy(order="F")
    t0 = time.perf_counter()
    c, info = lapack.dpotrf(A, lower=1, overwrite_a=1)
    inv, info2 = lapack.dpotri(c, lower=1, overwrite_c=1)
    t_cpu = time.perf_counter() - t0
    lines.append(f"{name}: scipy dpotrf + dpotri of Sigma (N = {A.shape[0]}, OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', '-')}) "
                 f"{1e3 * t_cpu:.0f} ms (info {info}, {info2})")
    return t_cpu, n


def stage_times(name, lines, n, t_cpu):
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "cov", "--", sys.executable, os.path.abspath(__file__),
               "--inner", name]
        subprocess.run(cmd, check=True, capture_output=True, timeout=600)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise RuntimeError("no kernel_stats.csv from rocprofv3: " + " ".join(glob.glob(os.path.join(d, "**"), recursive=True)))
        rows = list(csv.DictReader(open(files[0])))
    per = {}
    for r in rows:
        per[r["Name"]] = (int(r["Calls"]), float(r["TotalDurationNs"]) * 1e-6)
    tot = {}
    for stage, prefixes in STAGES:
        tot[stage] = sum(ms for k, (_, ms) in per.items() if any(k.startswith(p) or ("::" + p) in k or (" " + p) in k
                                                                  for p in prefixes))
    lines.append(f"{name}: GPU time per stage (ms): " + ", ".join(f"{k} {v:.2f}" for k, v in tot.items()))
    fi = tot["factorisation"] + tot["inverse"]
    lines.append(f"{name}: factor + inverse on the GPU {fi:.1f} ms vs {1e3 * t_cpu:.0f} ms on the CPU: {1e3 * t_cpu / fi:.1f}x")
    for k, (calls, ms) in sorted(per.items(), key=lambda kv: -kv[1][1]):
        if "cov" in k:
            lines.append(f"    {k[:90]:90s} {calls:6d} calls {ms:9.3f} ms")
    upd = [(c, ms) for k, (c, ms) in per.items() if "k_cov_potrf_update" in k]
    if upd:
        npad = -(-n // 64) * 64
        nt = npad // 64
        flop = sum((nt - kt - 1) * (nt - kt) // 2 for kt in range(nt)) * 2.0 * 64 ** 3
        rate = flop / (upd[0][1] * 1e-3)
        n_cu = 256                                                    # MI355X compute units
        peak = MFMA_FLOP / MFMA_CLK_PER_SIMD * SIMD_PER_CU * n_cu * CLOCK_GHZ * 1e9
        lines.append(f"{name}: trailing update (k_cov_potrf_update) {rate / 1e12:.2f} TFLOP/s = {100 * rate / peak:.1f} % of the "
                     f"measured MFMA issue rate ({peak / 1e12:.1f} TFLOP/s: {n_cu} CUs x 4 SIMDs x 2048 flop / 32 clocks at "
                     f"{CLOCK_GHZ} GHz)")


def smallest_refused_rcond(s, intr, lo=1e-300, hi=1.0, steps=60):
    """Bisection in log space: the pivot ratio min_k d_k / S_kk of the problem (rcond above it is refused)."""
    from bundle_adjustment_amd import hip_backend
    lib = s._lib
    ip = None if intr is None else hip_backend._dp(intr)

    def ok(r):
        return lib.ba_covariance(s._h, ip, 0, 1.0, r, None, None, None) == 0
    if not ok(lo):
        return 0.0
    for _ in range(steps):
        mid = np.sqrt(lo * hi)
        if ok(mid):
            lo = mid
        else:
            hi = mid
    return lo


def pivots(lines):
    from bundle_adjustment_amd import hip_backend
    from tests.schur_cases import bal_case, pinhole_case
    fixed, free = [], []
    for model in ("pinhole", "bal"):
        for n_cams in (3, 8, 17, 70):
            mk = pinhole_case if model == "pinhole" else bal_case
            k = min(4, n_cams)
            for gauge in (True, False):
                case = mk(n_cams, 12 * n_cams, k, seed=n_cams, fixed_cam=0 if (gauge or model == "pinhole") else -1)
                if gauge:
                    m = np.zeros(n_cams, np.uint16)
                    m[1] = 1 << 3
                    case.cam_mask = m
                with hip_backend.Solver(0) as s:
                    intr = case.upload(s)
                    r = smallest_refused_rcond(s, intr)
                (fixed if gauge else free).append(r)
                lines.append(f"pivot ratio {model:7s} Nc {n_cams:3d} gauge {'fixed' if gauge else 'free '}: {r:.3e}")
    for name in ("C3", "C5-BAL"):
        s, intr = problem(name)
        r = smallest_refused_rcond(s, intr, steps=40)
        fixed.append(r)
        lines.append(f"pivot ratio {name} gauge fixed: {r:.3e}")
        s.set_held(cams=None)
        if intr is None:
            r = smallest_refused_rcond(s, intr, steps=40)
            free.append(r)
            lines.append(f"pivot ratio {name} fixed_cam only (scale free): {r:.3e}")
        s.close()
    lines.append(f"smallest ratio on a gauge-fixed problem {min(fixed):.3e}; largest on a gauge-free one {max(free):.3e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cov_times.txt"))
    ap.add_argument("--skip-pivots", action="store_true")
    a = ap.parse_args()
    if a.inner:
        inner(a.inner)
        return
    lines = []
    for name in ("C3", "C5-BAL"):
        t_cpu, n = wall_and_cpu(name, lines)
        stage_times(name, lines, n, t_cpu)
        print("\n".join(lines), flush=True)
    if not a.skip_pivots:
        pivots(lines)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
