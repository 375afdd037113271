"""Times of ba_pose_graph (output kept in profiles/posegraph_times.txt).

    python tools/posegraph_times.py [--out FILE]

Host wall time of the whole call (uploads, incidence lists, LM loop, every output copied back), median of 5 after 2 warm-up
calls, with the LM and PCG iteration counts and the exit, for a ring of 256 / 2048 / 16384 nodes on a circle: odometry edges
(k, k + 1), three skip edges (k, k + 2), (k, k + 3), (k, k + 4) per node, one loop edge (n - 1, 0), exact measurements,
info = diag(100 x 3, 25 x 3, 50), node 0 held.  Start: odometry integrated with the drift of the tests' 16-node ring spread
over the ring (per step 1 % x 16 / n of scale, (0, 0.01, 0.002) x 16 / n rad, 0.02 x 16 / n in t), Sim(3) and SE(3), default
options.  Recorded, not gated: nobody has measured this before and there is no earlier implementation to compare with."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS, WARM = 5, 2
INFO = np.diag([100.0, 100.0, 100.0, 25.0, 25.0, 25.0, 50.0])


def ring(n, with_scale):
    from bundle_adjustment_amd import posegraph as pg
    a = 2.0 * np.pi * np.arange(n) / n
    radius = 5.0 * n / 16.0                       # the tests' spacing between neighbours
    truth = np.zeros((n, 7))
    truth[:, 1] = np.where(a > np.pi, a - 2.0 * np.pi, a)
    c, s = np.cos(a), np.sin(a)
    centre = radius * np.stack([c, np.zeros(n), s], axis=1)
    # R = rotation about y by a: t = -R centre
    truth[:, 3] = -(c * centre[:, 0] + s * centre[:, 2])
    truth[:, 5] = -(-s * centre[:, 0] + c * centre[:, 2])
    truth[:, 6] = 1.0
    k = np.arange(n)
    ei = np.concatenate([k[:-1], [n - 1]] + [k[:-d] for d in (2, 3, 4)]).astype(np.int32)
    ej = np.concatenate([k[1:], [0]] + [k[d:] for d in (2, 3, 4)]).astype(np.int32)
    meas = pg.relative(truth[ei], truth[ej])
    f = 16.0 / n
    drift = np.array([[0.0, 0.01 * f, 0.002 * f, 0.02 * f, 0.02 * f, 0.02 * f, 1.0 + (0.01 * f if with_scale else 0.0)]])
    start = truth.copy()
    for q in range(n - 1):
        step = pg.compose(drift, meas[q:q + 1])
        start[q + 1] = pg.compose(step, start[q:q + 1])[0]
    if not with_scale:
        start[:, 6] = 1.0
    held = np.zeros(n, np.uint8)
    held[0] = 1
    return start, ei, ej, meas, np.broadcast_to(INFO, (ei.size, 7, 7)).copy(), held, truth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posegraph_times.txt"))
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from bundle_adjustment_amd import hip_backend as hb
    lines = []
    with hb.Solver(0) as s:
        for n in (256, 2048, 16384):
            for with_scale in (True, False):
                start, ei, ej, meas, info, held, truth = ring(n, with_scale)
                w = []
                for r in range(WARM + REPS):
                    t0 = time.perf_counter()
                    out = s.pose_graph(start, ei, ej, meas, info=info, held=held, with_scale=with_scale)
                    if r >= WARM:
                        w.append(time.perf_counter() - t0)
                err = float(np.abs(out["poses"][:, 3:] - truth[:, 3:]).max())
                lines.append(f"ring of {n} nodes / {ei.size} edges, {'Sim(3)' if with_scale else 'SE(3)'}: wall {1e3 * float(np.median(w)):.2f} ms "
                             f"(min {1e3 * min(w):.2f}, max {1e3 * max(w):.2f}), of which the LM loop {1e3 * out['seconds_total']:.2f} ms; "
                             f"{out['iterations']} LM / {out['pcg_iterations']} PCG iterations, exit {out['status_name']}; cost "
                             f"{out['initial_cost']:.4e} -> {out['final_cost']:.4e}; max |t, s - truth| {err:.2e}")
                print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
