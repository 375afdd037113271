"""Times of ba_fundamental (output kept in profiles/fundamental_times.txt).

    python tools/fundamental_times.py [--out FILE]

Host wall time of the whole call, median of 11 after 3 warm-up calls, with every output copied back and with no output asked
for (every output pointer NULL: the uploads and the four kernels remain), for the shapes of tools/homography_times.py -- 1 pair
x 500 matches, 1 pair x 2000 matches and 32 pairs x 500 matches, n_hyp = 256 and 1024 (1024 is this call's default), default
options otherwise.  Matches: a box 4 .. 8 deep, 0.3 px noise, 30 % uniform mismatches.  Recorded, not gated: the call has no
predecessor to compare with; tools/homography_times.py run in the same session is the context."""
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


def matches(rng, n):
    """n matches of a box 2 .. 4 baselines deep, 0.3 px noise, 30 % of the second view's pixels uniform over the image."""
    w = rng.normal(size=3)
    w *= 0.14 / np.linalg.norm(w)
    th = np.linalg.norm(w)
    Wx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    R = np.eye(3) + np.sin(th) / th * Wx + (1 - np.cos(th)) / th ** 2 * Wx @ Wx
    t = np.array([1.0, 0.0, 0.0]) + 0.3 * rng.normal(size=3)
    t /= np.linalg.norm(t)
    X = np.c_[rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(4.0, 8.0, n)]
    Y = X @ R.T + 2.0 * t
    p1 = ((X / X[:, 2:]) @ K.T)[:, :2] + rng.normal(scale=0.3, size=(n, 2))
    p2 = ((Y / Y[:, 2:]) @ K.T)[:, :2] + rng.normal(scale=0.3, size=(n, 2))
    bad = rng.random(n) < 0.3
    p2[bad] = rng.uniform(0, 1, size=(int(bad.sum()), 2)) * np.array([1280.0, 720.0])
    return p1, p2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fundamental_times.txt"))
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from bundle_adjustment_amd import hip_backend as hb
    rng = np.random.default_rng(0)
    lines = []
    with hb.Solver(0) as s:
        for pairs, n in ((1, 500), (1, 2000), (32, 500)):
            ms = [matches(rng, n) for _ in range(pairs)]
            p1 = np.ascontiguousarray(np.concatenate([m[0] for m in ms]))
            p2 = np.ascontiguousarray(np.concatenate([m[1] for m in ms]))
            off = (np.arange(pairs + 1) * n).astype(np.int64)
            for n_hyp in (256, 1024):
                o = s.fundamental_options(n_hyp=n_hyp)
                dp = lambda x: x.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731

                def bare():
                    hb._check(s._lib.ba_fundamental(s._h, pairs, off.ctypes.data_as(C.POINTER(C.c_int64)), dp(p1), dp(p2), C.byref(o),
                                                    *([None] * 8)))
                times = {}
                for name, fn in (("all outputs", lambda: s.fundamental(p1, p2, off, n_hyp=n_hyp)), ("no output", bare)):
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
                lines.append(f"{pairs} pair(s) x {n} matches, n_hyp {n_hyp}: wall with all outputs {times['all outputs'][0]:.3f} ms "
                             f"(min {times['all outputs'][1]:.3f}, max {times['all outputs'][2]:.3f}); with no output "
                             f"{times['no output'][0]:.3f} ms (min {times['no output'][1]:.3f}, max {times['no output'][2]:.3f}); "
                             f"status counts {stat}, inlier share {share:.3f}")
                print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
