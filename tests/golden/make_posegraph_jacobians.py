"""Writes tests/golden/pg_jacobians.npz: the residual e and the Jacobians A = de/dd_i, B = de/dd_j of nine Sim(3) pose-graph
edges (include/ba_hip.h, ba_pose_graph), computed without the closed form the kernels and tests/posegraph_reference.py share.

The edges.  One per residual rotation |e_rot| in PHI = 0, 1e-9, 1e-5, 0.0099, 0.0101 (the two sides of the `t2 < 1e-4` series
switch of the inverse left Jacobian), 1, 3, pi - 1e-3, pi - 1e-6.  Both nodes of an edge are generic: rotation vectors of
0.3 .. 2.5 rad, |t| in 2 .. 10, scales in 0.5 .. 2 (ratios off 1), the translation and scale residuals of size 0.5 and 0.2.
The measurement's rotation is R_r exp(-phi) formed in fp64, so the residual rotation is phi to 1e-16; for phi = 0 node i
has rvec = 0 and the measurement carries node j's rvec, so that R_ij^T R_r is the identity exactly.

The values.  mpmath at 60 digits evaluates the header's definitions from the fp64 inputs:
  e = [ log(R_ij^T R_r) ; t_j - s_r R_r t_i - t_ij ; ln(s_r / s_ij) ],  R_r = R_j R_i^T,  s_r = s_j / s_i,
with the retraction R <- exp(d_omega) R, t <- t + d_t, s <- s exp(d_sigma), and the Jacobians by central differences of
step 1e-20 (truncation 1e-40 relative, rounding 1e-60 / 1e-20: both far below fp64).  Nothing of the closed form
N = Jl^-1(e_rot) R_ij^T enters.

The tolerance of the tests, TOL.  tests/test_posegraph_host.py measures the fp64 closed form of
posegraph_reference.jacobians_analytic against these values: its largest difference is REF_REL = 5.2e-16 of the largest
entry max |J| (the measured figure is in that test's output; the constant is that figure rounded up).  The device is held
to TOL = 50 x REF_REL: max |A - A_fix|, max |B - B_fix| <= TOL max |J| and max |e - e_fix| <= TOL.  The factor 50 allows for
the device's sin, cos and atan2 being a few ulp off libm's, and for pg_rodrigues forming 1 - cos(theta) directly.  The
bound comes from the reference's own error, never from what the device gives.

Run:  python tests/golden/make_posegraph_jacobians.py   (needs mpmath; the tests that read the fixture do not)."""
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "pg_jacobians.npz")
PHI = (0.0, 1e-9, 1e-5, 0.0099, 0.0101, 1.0, 3.0, math.pi - 1e-3, math.pi - 1e-6)
DIGITS, STEP = 60, "1e-20"
REF_REL = 5.2e-16
TOL = 50.0 * REF_REL


# ---- fp64: the inputs --------------------------------------------------------------------------------------------------
def _rodrigues64(v):
    th = float(np.linalg.norm(v))
    if th == 0.0:
        return np.eye(3)
    k = np.asarray(v) / th
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return math.cos(th) * np.eye(3) + (1.0 - math.cos(th)) * np.outer(k, k) + math.sin(th) * K


def _log64(R):
    """Rotation vector of R through the unit quaternion (any angle up to pi); used for the inputs only."""
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    k = int(np.argmax([tr, R[0, 0], R[1, 1], R[2, 2]]))
    if k == 0:
        q = np.array([1.0 + tr, R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    elif k == 1:
        q = np.array([R[2, 1] - R[1, 2], 1.0 + R[0, 0] - R[1, 1] - R[2, 2], R[0, 1] + R[1, 0], R[0, 2] + R[2, 0]])
    elif k == 2:
        q = np.array([R[0, 2] - R[2, 0], R[0, 1] + R[1, 0], 1.0 + R[1, 1] - R[0, 0] - R[2, 2], R[1, 2] + R[2, 1]])
    else:
        q = np.array([R[1, 0] - R[0, 1], R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], 1.0 + R[2, 2] - R[0, 0] - R[1, 1]])
    q = q / np.linalg.norm(q)
    if q[0] < 0:
        q = -q
    vn = float(np.linalg.norm(q[1:]))
    return 2.0 * q[1:] / q[0] if vn < 1e-10 else q[1:] * (2.0 * math.atan2(vn, q[0]) / vn)


def _unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def inputs():
    """-> poses (18, 7), ei, ej (9,), meas (9, 7): edge k joins nodes 2 k and 2 k + 1."""
    rng = np.random.default_rng(20)
    m = len(PHI)
    poses, meas = np.zeros((2 * m, 7)), np.zeros((m, 7))
    for k, phi in enumerate(PHI):
        i, j = 2 * k, 2 * k + 1
        for node in (i, j):
            poses[node, :3] = _unit(rng) * rng.uniform(0.3, 2.5)
            poses[node, 3:6] = _unit(rng) * rng.uniform(2.0, 10.0)
            poses[node, 6] = rng.uniform(0.5, 2.0)
        axis = _unit(rng)
        if phi == 0.0:
            poses[i, :3] = 0.0
            meas[k, :3] = poses[j, :3]
        else:
            Rr = _rodrigues64(poses[j, :3]) @ _rodrigues64(poses[i, :3]).T
            meas[k, :3] = _log64(Rr @ _rodrigues64(phi * axis).T)
        sr = poses[j, 6] / poses[i, 6]
        Rr = _rodrigues64(poses[j, :3]) @ _rodrigues64(poses[i, :3]).T
        meas[k, 3:6] = poses[j, 3:6] - sr * Rr @ poses[i, 3:6] - 0.5 * _unit(rng)
        meas[k, 6] = sr * math.exp(0.2 * (1.0 if k % 2 else -1.0))
    ei = np.arange(0, 2 * m, 2, dtype=np.int32)
    return poses, ei, ei + 1, meas


# ---- mpmath: the values ------------------------------------------------------------------------------------------------
def _mp():
    import mpmath
    mpmath.mp.dps = DIGITS
    return mpmath


def _exp_so3(mp, v):
    th = mp.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    if th == 0:
        return mp.eye(3)
    k = [x / th for x in v]
    K = mp.matrix([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    kk = mp.matrix(3, 3)
    for a in range(3):
        for b in range(3):
            kk[a, b] = k[a] * k[b]
    return mp.cos(th) * mp.eye(3) + (1 - mp.cos(th)) * kk + mp.sin(th) * K


def _log_so3(mp, R):
    """theta axis with theta = atan2(|v|, (tr - 1) / 2), v = the skew part: exact at 60 digits for every angle below pi."""
    v = [(R[2, 1] - R[1, 2]) / 2, (R[0, 2] - R[2, 0]) / 2, (R[1, 0] - R[0, 1]) / 2]
    s = mp.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    if s == 0:
        return [mp.mpf(0)] * 3
    th = mp.atan2(s, (R[0, 0] + R[1, 1] + R[2, 2] - 1) / 2)
    return [x * th / s for x in v]


def _pose(mp, p):
    return _exp_so3(mp, [mp.mpf(float(x)) for x in p[:3]]), [mp.mpf(float(x)) for x in p[3:6]], mp.mpf(float(p[6]))


def _retract(mp, pose, d):
    R, t, s = pose
    return _exp_so3(mp, d[:3]) * R, [t[a] + d[3 + a] for a in range(3)], s * mp.exp(d[6])


def _residual(mp, pi, pj, ms):
    (Ri, ti, si), (Rj, tj, sj), (Rm, tm, sm) = pi, pj, ms
    Rr = Rj * Ri.T
    sr = sj / si
    q = sr * (Rr * mp.matrix(ti))
    return _log_so3(mp, Rm.T * Rr) + [tj[a] - q[a] - tm[a] for a in range(3)] + [mp.log(sr / sm)]


def values(poses, ei, ej, meas):
    """-> e (m, 7), A, B (m, 7, 7) as float64, from 60-digit arithmetic on the fp64 inputs."""
    mp = _mp()
    h = mp.mpf(STEP)
    m = len(ei)
    e, A, B = np.zeros((m, 7)), np.zeros((m, 7, 7)), np.zeros((m, 7, 7))
    for k in range(m):
        pi, pj, ms = _pose(mp, poses[ei[k]]), _pose(mp, poses[ej[k]]), _pose(mp, meas[k])
        e[k] = [float(x) for x in _residual(mp, pi, pj, ms)]
        for c in range(7):
            dp = [h if a == c else mp.mpf(0) for a in range(7)]
            dm = [-x for x in dp]
            up, dn = _residual(mp, _retract(mp, pi, dp), pj, ms), _residual(mp, _retract(mp, pi, dm), pj, ms)
            A[k, :, c] = [float((up[a] - dn[a]) / (2 * h)) for a in range(7)]
            up, dn = _residual(mp, pi, _retract(mp, pj, dp), ms), _residual(mp, pi, _retract(mp, pj, dm), ms)
            B[k, :, c] = [float((up[a] - dn[a]) / (2 * h)) for a in range(7)]
    return e, A, B


def main():
    poses, ei, ej, meas = inputs()
    e, A, B = values(poses, ei, ej, meas)
    np.savez(OUT, poses=poses, ei=ei, ej=ej, meas=meas, phi=np.array(PHI), e=e, A=A, B=B)
    print(f"wrote {OUT}: {len(ei)} edges, |e_rot| {np.linalg.norm(e[:, :3], axis=1)}, max |J| {max(np.abs(A).max(), np.abs(B).max()):.3f}")


if __name__ == "__main__":
    main()
