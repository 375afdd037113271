"""Times of ba_match_descriptors (output kept in profiles/match_times.txt).

    python tools/match_times.py [--out FILE] [--case N]

Host wall time of the whole call, median of 21 after 5 warm-up calls, with every output copied back and with no output asked
for (every output pointer NULL: the upload, the pair table and the two kernels remain), 32-byte descriptors, default options
and mutual = 1:
  case 0 .. 2   one pair of 500, 3000, 4000 descriptors per side;
  case 3        32 pairs of 3000 queries each against one shared set of 3000 (the exhaustive keyframe loop).
Descriptors: random bytes; half of each query set is a copy of a train descriptor with up to 20 bits flipped, so that the ratio
test has matches to keep.  --case N runs one case alone (what a kernel trace of that case is taken from).  Recorded, not gated."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS, WARM = 21, 5
CASES = ((1, 500), (1, 3000), (1, 4000), (32, 3000))


def descriptors(rng, n_sets, n):
    """One train set of n descriptors and n_sets query sets of n: every second query a noisy copy of a train descriptor."""
    train = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    sets = [train]
    for _ in range(n_sets):
        q = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        src = rng.permutation(n)[: n // 2]
        q[::2][: len(src)] = train[src]
        for r in range(0, 2 * len(src), 2):
            for bit in rng.integers(0, 256, rng.integers(0, 21)):
                q[r, bit // 8] ^= np.uint8(1 << (bit % 8))
        sets.append(q)
    return sets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match_times.txt"))
    ap.add_argument("--case", type=int, default=-1)
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from bundle_adjustment_amd import hip_backend as hb
    rng = np.random.default_rng(0)
    lines = []
    i64, i32, u8 = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    with hb.Solver(0) as s:
        for case, (pairs, n) in enumerate(CASES):
            if a.case >= 0 and case != a.case:
                continue
            sets = descriptors(rng, pairs, n)
            pr = np.array([(1 + p, 0) for p in range(pairs)], dtype=np.int32)
            desc = np.ascontiguousarray(np.concatenate(sets))
            off = (np.arange(len(sets) + 1) * n).astype(np.int64)
            pq, pt = np.ascontiguousarray(pr[:, 0]), np.ascontiguousarray(pr[:, 1])
            for mutual in (0, 1):
                o = s.match_options(mutual=mutual)

                def bare():
                    hb._check(s._lib.ba_match_descriptors(s._h, 32, len(sets), off.ctypes.data_as(i64), desc.ctypes.data_as(u8), pairs,
                                                          pq.ctypes.data_as(i32), pt.ctypes.data_as(i32), C.byref(o), None, None, None,
                                                          None, None, None, None))
                times = {}
                for name, fn in (("all outputs", lambda: s.match_descriptors(sets, pr, mutual=mutual)), ("no output", bare)):
                    for _ in range(WARM):
                        out = fn()
                    w = []
                    for _ in range(REPS):
                        t0 = time.perf_counter()
                        fn()
                        w.append(time.perf_counter() - t0)
                    times[name] = (1e3 * float(np.median(w)), 1e3 * min(w), 1e3 * max(w))
                    if out is not None:
                        share = float(out["good"].mean())
                lines.append(f"{pairs} pair(s) x {n} x {n} descriptors of 32 bytes, mutual {mutual}: wall with all outputs "
                             f"{times['all outputs'][0]:.3f} ms (min {times['all outputs'][1]:.3f}, max {times['all outputs'][2]:.3f}); with no "
                             f"output {times['no output'][0]:.3f} ms (min {times['no output'][1]:.3f}, max {times['no output'][2]:.3f}); "
                             f"good share {share:.3f}")
                print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
