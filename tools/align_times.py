"""Wall times of ba_align with apply = 1 (output kept in profiles/align_times.txt).

    python tools/align_times.py [--out FILE]

At C3 (1 000 cameras / 100 000 points, pinhole) and at BASELINE config 5 on the BAL camera: references for every camera
centre and every point (a known similarity of the current positions plus 0.05 noise), Huber loss, 10 IRLS rounds.  Median
of 20 calls after 3 warm-ups of
  * Solver.align(cam_ref, pt_ref, apply=True): upload of the references, every round and the transform on the device, one drain;
  * the same on the camera references alone;
  * the host path it replaces: get_params, numpy (camera centres, a weighted Umeyama + Huber IRLS written out below,
    similarity.apply's arithmetic), set_params.
Recorded, not gated."""
import argparse
import dataclasses
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS, WARMUP = 20, 3


def problem(name):
    from bundle_adjustment_amd import hip_backend
    s = hip_backend.Solver(0)
    if name == "C3":
        from bundle_adjustment_amd.synthetic import make_config
        p = make_config("C3")
        s.set_problem(p)
        return s, p
    from bundle_adjustment_amd.synthetic import make_bal_problem
    b = make_bal_problem()
    s.set_problem_bal(b, 0)
    return s, b


def median_ms(fn):
    for _ in range(WARMUP):
        fn()
    t = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t)), 1e3 * min(t), 1e3 * max(t)


def host_align(a, b, f_scale, iters):
    """What a caller writes in numpy: Umeyama's closed form, re-weighted `iters` times with Huber's rho'."""
    u = np.ones(len(a))
    for _ in range(iters + 1):
        W = u.sum()
        mu_a, mu_b = (u[:, None] * a).sum(0) / W, (u[:, None] * b).sum(0) / W
        x, y = a - mu_a, b - mu_b
        U, D, Vt = np.linalg.svd(np.einsum("n,ni,nj->ij", u, y, x) / W)
        d = np.array([1.0, 1.0, np.sign(np.linalg.det(U) * np.linalg.det(Vt))])
        R = U @ np.diag(d) @ Vt
        sc = (D * d).sum() / ((u * (x * x).sum(1)).sum() / W)
        z = ((y - sc * x @ R.T) ** 2).sum(1) / (f_scale * f_scale)
        u = np.where(z <= 1.0, 1.0, 1.0 / np.sqrt(np.maximum(z, 1.0)))
    return sc, R, mu_b - sc * R @ mu_a


def measure(name, lines):
    from bundle_adjustment_amd import similarity
    from bundle_adjustment_amd.rotations import rvecs_to_matrices
    s, p = problem(name)
    rng = np.random.default_rng(0)
    R0, s0, t0 = rvecs_to_matrices(np.array([[0.7, -1.9, 0.4]]))[0], 12.5, np.array([310.0, -120.0, 45.0])
    cams, pts = s.get_params()
    cam_ref = s0 * s.centres() @ R0.T + t0 + rng.normal(0.0, 0.05, size=(p.n_cams, 3))
    pt_ref = s0 * pts @ R0.T + t0 + rng.normal(0.0, 0.05, size=(p.n_pts, 3))
    kw = dict(loss="huber", f_scale=0.15, iters=10)
    first = s.align(cam_ref=cam_ref, pt_ref=pt_ref, apply=True, **kw)
    lines.append(f"{name}: {p.n_cams} cameras, {p.n_pts} points; first call: status {first['status']}, s {first['s']:.6f}, rms {first['rms']:.4f}, "
                 f"max {first['max']:.4f}, n_used {first['n_used']}")
    both = median_ms(lambda: s.align(cam_ref=cam_ref, pt_ref=pt_ref, apply=True, **kw))
    cams_only = median_ms(lambda: s.align(cam_ref=cam_ref, apply=True, **kw))

    def host_path():
        c, x = s.get_params()
        ctr = -np.einsum("nji,nj->ni", rvecs_to_matrices(c[:, :3]), c[:, 3:6])
        sc, R, t = host_align(np.concatenate([ctr, x]), np.concatenate([cam_ref, pt_ref]), kw["f_scale"], kw["iters"])
        moved = similarity.apply(dataclasses.replace(p, cams=np.concatenate([c, p.cams[:, 6:]], axis=1), pts=x), sc, R, t)
        s.set_params(np.ascontiguousarray(moved.cams[:, :6]), moved.pts)
    host = median_ms(host_path)
    for what, (med, lo, hi) in (("ba_align(apply=1), cameras + points", both), ("ba_align(apply=1), cameras only", cams_only),
                                ("host path: get_params + numpy + set_params", host)):
        lines.append(f"{name}: {what}: {med:.3f} ms (min {lo:.3f}, max {hi:.3f})")
    lines.append(f"{name}: the host path takes {host[0] / both[0]:.0f}x the device call")
    s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_times.txt"))
    a = ap.parse_args()
    lines = []
    for name in ("C3", "C5-BAL"):
        measure(name, lines)
        print("\n".join(lines[-5:]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
