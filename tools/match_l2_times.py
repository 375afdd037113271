"""Times of ba_match_l2 (output kept in profiles/match_l2_times.txt).

    python tools/match_l2_times.py [--out FILE] [--case N] [--trace]

Host wall time of the whole call, median of 21 after 5 warm-up calls, with every output copied back and with no output asked
for (every output pointer NULL: the upload, the pair table and the three kernels remain), 128-byte descriptors, ratio 0.8, with
mutual 0 and 1:
  case 0, 1     one pair of 2000 and of 8000 descriptors per side;
  case 2        32 pairs of 8000 queries each against one shared set of 8000.
Descriptors: SIFT-like rows (non-negative, heavy-tailed, L2-normalised, clipped at 0.2) through quantize_descriptors; half of each
query set is a noisy copy (sigma 0.04) of a train row, so that the ratio test has matches to keep.
Beside each row two floors of k_l2_partial on an MI355X (256 compute units x 4 SIMDs, 2.4 GHz), for r = entries x nq x nt results
(an entry is a pair, or with mutual a pair and its swapped twin):
  MFMA floor   one v_mfma_i32_32x32x32_i8 gives 32 x 32 results over 32 bytes and occupies its SIMD for 32 cycles (the cycles of
               the bf16 32x32x16 form: MI355X_MICROARCH, matrix cores), so 128 bytes cost 4 x 32 = 128 cycles per 1024 results:
               t = r / 1024 x 128 / (1024 SIMDs x 2.4e9 Hz).
  VALU floor   the selection spends 3 VALU instructions per result and lane (v_lshl_add_u32, v_med3_i32, v_min_i32, counted in
               the ISA of k_l2_partial<4>: 48 of them follow every 4 MFMAs); a wave64 instruction occupies the 16-lane SIMD for 4
               cycles and covers 64 results: t = r / 64 x 3 x 4 / (1024 SIMDs x 2.4e9 Hz) = 1.5 x the MFMA floor.
--trace adds, per row, the kernels' own durations from one `rocprofv3 --kernel-trace --stats` run of a child process (a run of its
own, no counters) that makes the row's calls with 2 warm-up and 6 timed repetitions: 8 calls with every output and 8 with none, 16
launches of each kernel, the same kernels either way.  --case N runs one case alone.  Recorded, not gated."""
import argparse
import csv
import ctypes as C
import glob
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS, WARM, WIDTH = 21, 5, 128
CASES = ((1, 2000), (1, 8000), (32, 8000))
SIMDS, HZ = 1024, 2.4e9
DERIVATION = (
    "Floors of k_l2_partial on 256 compute units x 4 SIMDs at 2.4 GHz, r = entries x nq x nt results (mutual doubles the entries):",
    "  MFMA floor: one v_mfma_i32_32x32x32_i8 = 1024 results over 32 bytes in 32 cycles of its SIMD (the cycles of the bf16 32x32x16 form),",
    "              so 128 bytes cost 128 cycles per 1024 results: t = r / 1024 x 128 / (1024 x 2.4e9).",
    "  VALU floor: 3 VALU instructions per result and lane (v_lshl_add_u32, v_med3_i32, v_min_i32: 48 follow every 4 MFMAs in the ISA), a wave64",
    "              instruction = 64 results in 4 cycles of its 16-lane SIMD: t = r / 64 x 3 x 4 / (1024 x 2.4e9) = 1.5 x the MFMA floor.",
    "Kernel lines: mean duration over the 16 launches of a rocprofv3 --kernel-trace --stats run of a child process (no counters) that makes",
    "              the row's call 8 times with every output and 8 times with none.",
)


def sift_like(rng, n):
    x = rng.exponential(1.0, (n, WIDTH)) ** 2
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return np.minimum(x, 0.2)


def descriptors(rng, n_sets, n):
    """One train set of n descriptors and n_sets query sets of n: every second query a noisy copy of a train descriptor."""
    from bundle_adjustment_amd import quantize_descriptors
    train = sift_like(rng, n)
    sets = [quantize_descriptors(train)]
    for _ in range(n_sets):
        q = sift_like(rng, n)
        src = rng.permutation(n)[: n // 2]
        q[::2][: len(src)] = np.maximum(train[src] + rng.normal(0.0, 0.04, (len(src), WIDTH)), 0.0)
        sets.append(quantize_descriptors(q))
    return sets


def floors(pairs, n, mutual):
    r = pairs * (2 if mutual else 1) * n * n
    mfma = r / 1024 * (WIDTH // 32) * 32 / (SIMDS * HZ)
    valu = r / 64 * 3 * 4 / (SIMDS * HZ)
    return 1e3 * mfma, 1e3 * valu


def run_case(s, hb, rng, pairs, n, mutual, reps, warm):
    """-> {name: (median, min, max) ms} and the share of good rows."""
    i64, i32, u8 = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    sets = descriptors(rng, pairs, n)
    pr = np.array([(1 + p, 0) for p in range(pairs)], dtype=np.int32)
    desc = np.ascontiguousarray(np.concatenate(sets))
    off = (np.arange(len(sets) + 1) * n).astype(np.int64)
    pq, pt = np.ascontiguousarray(pr[:, 0]), np.ascontiguousarray(pr[:, 1])
    o = s.match_options(mutual=mutual, ratio=0.8)

    def bare():
        hb._check(s._lib.ba_match_l2(s._h, WIDTH, len(sets), off.ctypes.data_as(i64), desc.ctypes.data_as(u8), pairs, pq.ctypes.data_as(i32),
                                     pt.ctypes.data_as(i32), C.byref(o), None, None, None, None, None, None, None))
    times, share = {}, float("nan")
    for name, fn in (("all outputs", lambda: s.match_l2(sets, pr, mutual=mutual, ratio=0.8)), ("no output", bare)):
        for _ in range(warm):
            out = fn()
        w = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            w.append(time.perf_counter() - t0)
        times[name] = (1e3 * float(np.median(w)), 1e3 * min(w), 1e3 * max(w))
        if out is not None:
            share = float(out["good"].mean())
    return times, share


def trace(case, mutual):
    """{kernel: (launches, mean duration in us)} of the ba_match_l2 kernels in a child process under rocprofv3 that makes the row's
    calls: run_case with 2 warm-up and 6 timed repetitions, with every output and with none."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "l2", "--", sys.executable,
               os.path.abspath(__file__), "--inner", str(case), "--mutual", str(mutual)]
        subprocess.run(cmd, check=True, capture_output=True, timeout=300)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise RuntimeError("no kernel_stats.csv from rocprofv3")
        rows = list(csv.DictReader(open(files[0])))
    return {r["Name"].split("(")[0].replace("void ba::", ""): (int(r["Calls"]), 1e-3 * float(r["TotalDurationNs"]) / int(r["Calls"]))
            for r in rows if "k_l2_" in r["Name"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match_l2_times.txt"))
    ap.add_argument("--case", type=int, default=-1)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--inner", type=int, default=-1)
    ap.add_argument("--mutual", type=int, default=0)
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from bundle_adjustment_amd import hip_backend as hb
    if a.inner >= 0:                                   # the traced child: one row's calls, with and without outputs; nothing written
        pairs, n = CASES[a.inner]
        with hb.Solver(0) as s:
            run_case(s, hb, np.random.default_rng(a.inner), pairs, n, a.mutual, 6, 2)
        return
    lines = [f"ba_match_l2, {WIDTH}-byte descriptors, ratio 0.8; median of {REPS} after {WARM} warm-up calls.  Recorded, not gated."] + list(DERIVATION)
    with hb.Solver(0) as s:
        for case, (pairs, n) in enumerate(CASES):
            if a.case >= 0 and case != a.case:
                continue
            for mutual in (0, 1):
                times, share = run_case(s, hb, np.random.default_rng(case), pairs, n, mutual, REPS, WARM)
                mfma, valu = floors(pairs, n, mutual)
                lines.append(f"{pairs} pair(s) x {n} x {n}, mutual {mutual}: wall with all outputs {times['all outputs'][0]:.3f} ms (min "
                             f"{times['all outputs'][1]:.3f}, max {times['all outputs'][2]:.3f}); with no output {times['no output'][0]:.3f} ms (min "
                             f"{times['no output'][1]:.3f}, max {times['no output'][2]:.3f}); good share {share:.3f}; MFMA floor {mfma:.4f} ms, "
                             f"VALU floor {valu:.4f} ms")
                print(lines[-1], flush=True)
                if a.trace:
                    for name, (calls, mean) in sorted(trace(case, mutual).items()):
                        extra = f" = {1e-3 * mean / valu:.2f} x the VALU floor, {1e-3 * mean / mfma:.2f} x the MFMA floor" if "partial" in name else ""
                        lines.append(f"    {name}: {calls} launches, mean {mean:.2f} us{extra}")
                        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
