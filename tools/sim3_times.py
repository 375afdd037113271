"""Times of ba_sim3 (output kept in profiles/sim3_times.txt).

    python tools/sim3_times.py [--out FILE]

Host wall time of the whole call, median of 11 after 3 warm-up calls, with every output copied back and with no output asked
for (every output pointer NULL: the uploads and the two kernels remain), for 1 pair x 300 correspondences, 1 pair x 2000 and
32 pairs x 300, n_hyp = 256 and 1024, default options otherwise.  Correspondences: points 4 - 10 deep in view 1 under a
similarity of about 10 degrees and a scale in 0.7 .. 1.4, 3D noise of 0.002 on both frames, 30 % of view 2's points replaced by
other points of the volume.  Recorded, not gated: the call has no predecessor to compare with."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS, WARM = 11, 3
K = np.array([[820.0, 0.0, 640.0], [0.0, 790.0, 360.0], [0.0, 0.0, 1.0]])


def points(rng, n):
    z = rng.uniform(4.0, 10.0, n)
    return np.c_[rng.uniform(-0.5, 0.5, n) * z, rng.uniform(-0.4, 0.4, n) * z, z]


def correspondences(rng, n):
    """n correspondences X2 = s R X1 + t with 3D noise of 0.002, 30 % of X2 the images of other points."""
    w = rng.normal(size=3)
    w *= 0.17 / np.linalg.norm(w)
    th = np.linalg.norm(w)
    Wx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    R = np.eye(3) + np.sin(th) / th * Wx + (1 - np.cos(th)) / th ** 2 * Wx @ Wx
    t = np.array([0.8, -0.3, 0.6]) + 0.4 * rng.normal(size=3)
    s = np.exp(rng.uniform(-0.35, 0.35))
    X1 = points(rng, n)
    X2 = s * X1 @ R.T + t
    bad = rng.random(n) < 0.3
    X2[bad] = s * points(rng, int(bad.sum())) @ R.T + t
    return X1 + rng.normal(scale=0.002, size=(n, 3)), X2 + rng.normal(scale=0.002, size=(n, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim3_times.txt"))
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from bundle_adjustment_amd import hip_backend as hb
    rng = np.random.default_rng(0)
    lines = []
    with hb.Solver(0) as s:
        for pairs, n in ((1, 300), (1, 2000), (32, 300)):
            ms = [correspondences(rng, n) for _ in range(pairs)]
            X1 = np.ascontiguousarray(np.concatenate([m[0] for m in ms]))
            X2 = np.ascontiguousarray(np.concatenate([m[1] for m in ms]))
            off = (np.arange(pairs + 1) * n).astype(np.int64)
            for n_hyp in (256, 1024):
                o = s.sim3_options(n_hyp=n_hyp)
                dp = lambda x: x.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731

                def bare():
                    hb._check(s._lib.ba_sim3(s._h, dp(K), pairs, off.ctypes.data_as(C.POINTER(C.c_int64)), dp(X1), dp(X2), C.byref(o),
                                             *([None] * 8)))
                times = {}
                for name, fn in (("all outputs", lambda: s.sim3(K, X1, X2, off, n_hyp=n_hyp)), ("no output", bare)):
                    for _ in range(WARM):
                        out = fn()
                    w = []
                    for _ in range(REPS):
                        t0 = time.perf_counter()
                        fn()
                        w.append(time.perf_counter() - t0)
                    times[name] = (1e3 * float(np.median(w)), 1e3 * min(w), 1e3 * max(w))
                    if out is not None:
                        stat = np.bincount(out["status"], minlength=4).tolist()
                        share = float(out["match_inlier"].mean())
                lines.append(f"{pairs} pair(s) x {n} correspondences, n_hyp {n_hyp}: wall with all outputs {times['all outputs'][0]:.3f} ms "
                             f"(min {times['all outputs'][1]:.3f}, max {times['all outputs'][2]:.3f}); with no output "
                             f"{times['no output'][0]:.3f} ms (min {times['no output'][1]:.3f}, max {times['no output'][2]:.3f}); "
                             f"status counts {stat}, inlier share {share:.3f}")
                print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
