"""Times of ba_match_guided next to ba_match_descriptors on the same data (output kept in
profiles/guided_match_times.txt).

    python tools/guided_match_times.py [--out FILE] [--case N]

Host wall time of the bare C call with every output pointer NULL (the uploads, the pair table and the kernels remain), median of
21 after 5 warm-up calls, 32-byte descriptors, default options, mutual = 0 and 1:
  case 0, 1   1 and 32 pairs of 3000 queries each against one shared set of 3000: the plain matcher, then the window gate, the
              epipolar gate and a window of radius 1e30 (every row admitted: gate and popcounts on every row, the worst case) on
              the same descriptors (sets as tools/match_times.py's);
  case 2      100 000 map points against 3000 keypoints: the plain matcher, then the window gate.
Keypoints: uniform in 1280 x 720.  Windows: centred on the partner's keypoint where the query has one (every second query),
elsewhere on a random pixel, radius 8 px; F: a sideways motion of a few degrees, max_epi_px = 3.  The mean n_cand of each guided
case is printed: it is what the wave-uniform skip of the popcounts depends on.  --case N runs one case alone.  Recorded, not gated."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS, WARM = 21, 5
CASES = ((1, 3000, 3000), (32, 3000, 3000), (1, 100000, 3000))      # pairs, queries per pair, train rows
SIZE = (1280, 720)


def scene(rng, pairs, nq, nt):
    """One train set of nt descriptors with keypoints and `pairs` query sets of nq: every second query a noisy copy of a train
    descriptor, its window centred on that train row's keypoint and its own keypoint on that row's epipolar line."""
    train = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
    kp_t = np.c_[rng.uniform(0, SIZE[0], nt), rng.uniform(0, SIZE[1], nt)].astype(np.float32)
    sets, kps, wins = [train], [kp_t], []
    for _ in range(pairs):
        q = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
        src = rng.integers(0, nt, (nq + 1) // 2)
        q[::2] = train[src]
        flips = rng.integers(0, 256, ((nq + 1) // 2, 20))
        keep = rng.integers(0, 21, (nq + 1) // 2)
        for k in range(20):
            on = keep > k
            q[::2][on, flips[on, k] // 8] ^= (1 << (flips[on, k] % 8)).astype(np.uint8)
        centre = np.c_[rng.uniform(0, SIZE[0], nq), rng.uniform(0, SIZE[1], nq)].astype(np.float32)
        centre[::2] = kp_t[src]
        kp_q = centre.copy()
        kp_q[:, 0] = rng.uniform(0, SIZE[0], nq)                  # F below: the line of (x1, y1) is y = y1
        sets.append(q)
        kps.append(kp_q)
        wins.append(np.c_[centre, np.full(nq, 8.0, dtype=np.float32)])
    return sets, kps, np.ascontiguousarray(np.concatenate(wins), dtype=np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guided_match_times.txt"))
    ap.add_argument("--case", type=int, default=-1)
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from bundle_adjustment_amd import hip_backend as hb
    rng = np.random.default_rng(0)
    lines = []
    i64, i32, u8, f32, f64 = (C.POINTER(t) for t in (C.c_int64, C.c_int32, C.c_uint8, C.c_float, C.c_double))
    with hb.Solver(0) as s:
        for case, (pairs, nq, nt) in enumerate(CASES):
            if a.case >= 0 and case != a.case:
                continue
            sets, kps, win = scene(rng, pairs, nq, nt)
            pr = np.array([(1 + p, 0) for p in range(pairs)], dtype=np.int32)
            desc = np.ascontiguousarray(np.concatenate(sets))
            xy = np.ascontiguousarray(np.concatenate(kps))
            off = np.r_[0, np.cumsum([len(x) for x in sets])].astype(np.int64)
            pq, pt = np.ascontiguousarray(pr[:, 0]), np.ascontiguousarray(pr[:, 1])
            F = np.ascontiguousarray(np.tile(np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], dtype=np.float64), (pairs, 1, 1)))
            win_all = win.copy()
            win_all[:, 2] = 1e30
            head = (s._h, 32, len(sets), off.ctypes.data_as(i64), desc.ctypes.data_as(u8))
            for mutual in (0, 1):
                om = s.match_options(mutual=mutual)
                ow = s.guided_options(mutual=mutual, gate="window")
                oe = s.guided_options(mutual=mutual, gate="epipolar")

                def plain():
                    hb._check(s._lib.ba_match_descriptors(*head, pairs, pq.ctypes.data_as(i32), pt.ctypes.data_as(i32), C.byref(om),
                                                          *([None] * 7)))

                def guided(o, w, f):
                    hb._check(s._lib.ba_match_guided(*head, xy.ctypes.data_as(f32), pairs, pq.ctypes.data_as(i32), pt.ctypes.data_as(i32),
                                                     C.byref(o), w, f, *([None] * 8)))
                runs = [("plain", plain, None), ("window", lambda: guided(ow, win.ctypes.data_as(f32), None), dict(window=win))]
                if case < 2:
                    runs.append(("epipolar", lambda: guided(oe, None, F.ctypes.data_as(f64)), dict(fundamental=F)))
                    runs.append(("window of radius 1e30 (every row admitted: the gate's worst case)",
                                 lambda: guided(ow, win_all.ctypes.data_as(f32), None), dict(window=win_all)))
                base = None
                for name, fn, kw in runs:
                    for _ in range(WARM):
                        fn()
                    w = []
                    for _ in range(REPS):
                        t0 = time.perf_counter()
                        fn()
                        w.append(time.perf_counter() - t0)
                    med = 1e3 * float(np.median(w))
                    base = med if base is None else base
                    extra = ""
                    if kw is not None:
                        out = s.match_guided(sets, kps, pr, mutual=mutual, **kw)
                        extra = f"; {med / base:.2f} x plain; mean n_cand {out['n_cand'].mean():.2f}, good share {out['good'].mean():.3f}"
                    lines.append(f"{pairs} pair(s) x {nq} x {nt} descriptors of 32 bytes, mutual {mutual}, {name}: wall with no output "
                                 f"{med:.3f} ms (min {1e3 * min(w):.3f}, max {1e3 * max(w):.3f}){extra}")
                    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
