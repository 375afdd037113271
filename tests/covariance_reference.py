"""Reference marginal covariances (ba_covariance) on the reduced problem of tests/held_reference.Reduced: the Schur-complement
formulas of include/ba_hip.h in fp64 numpy, and the dense (J^T w J)^-1 they must equal.  Test infrastructure only."""
import numpy as np

from tests import robust_losses as rl
from tests.held_reference import Reduced


def one_camera_points(ci, pi, n_pts, held_pt=None):
    """Points whose observations all come from one camera (or none), held points excluded."""
    first = np.full(n_pts, -1)
    multi = np.zeros(n_pts, bool)
    for c, p in zip(ci, pi):
        if first[p] < 0:
            first[p] = c
        elif first[p] != c:
            multi[p] = True
    out = ~multi
    if held_pt is not None:
        out &= ~np.asarray(held_pt, bool)
    return out


def schur_covariance(red: Reduced, cams, pts, loss="linear", f_scale=1.0):
    """dict(S (N, N) with held rows identity, full (N, N) = S^-1 with held rows / columns 0, cams (Nc, nb, nb),
    points (Np, 3, 3): held 0, one-camera NaN, onecam (Np,) bool, Wobs (Nobs, nb, 3), Vinv (Np, 3, 3))."""
    ne = red.normal_equations(cams, pts, loss, f_scale)
    nc, nb = red.cams.shape
    npt = red.pts.shape[0]
    ci, pi = np.asarray(red.ci), np.asarray(red.pi)
    onecam = one_camera_points(ci, pi, npt, red.held_pt)
    skip = onecam | red.held_pt
    n = nb * nc
    S = np.zeros((n, n))
    for c in range(nc):
        S[nb * c:nb * c + nb, nb * c:nb * c + nb] = ne["Hcc"][c]
    # the one-camera points' observations leave U
    r = red.res(cams, pts)
    w = rl.weights(r, loss, f_scale)
    Jc, _ = red.blocks(cams, pts)
    for o in np.nonzero(onecam[pi])[0]:
        c = ci[o]
        S[nb * c:nb * c + nb, nb * c:nb * c + nb] -= Jc[o].T @ (w[o][:, None] * Jc[o])
    Vinv = np.zeros((npt, 3, 3))
    keep = ~skip
    Vinv[keep] = np.linalg.inv(ne["Hpp"][keep])
    Wd = np.zeros((n, 3 * npt))
    for o in range(len(ci)):
        if skip[pi[o]]:
            continue
        c, p = ci[o], pi[o]
        Wd[nb * c:nb * c + nb, 3 * p:3 * p + 3] += ne["W"][o]
    Hinv = np.zeros((3 * npt, 3 * npt))
    for p in np.nonzero(keep)[0]:
        Hinv[3 * p:3 * p + 3, 3 * p:3 * p + 3] = Vinv[p]
    S -= Wd @ Hinv @ Wd.T
    held = red.held_cam.ravel()
    S[held, :] = 0.0
    S[:, held] = 0.0
    S[held, held] = 1.0
    full = np.linalg.inv(S)
    full[held, :] = 0.0
    full[:, held] = 0.0
    cam_blocks = np.array([full[nb * c:nb * c + nb, nb * c:nb * c + nb] for c in range(nc)])
    Pc = np.zeros((npt, 3, 3))
    Pc[onecam] = np.nan
    for p in np.nonzero(keep)[0]:
        wp = Wd[:, 3 * p:3 * p + 3]
        Pc[p] = Vinv[p] + Vinv[p] @ (wp.T @ full @ wp) @ Vinv[p]
    return dict(S=S, full=full, cams=cam_blocks, points=Pc, onecam=onecam, Wobs=ne["W"], Vinv=Vinv)


def dense_information(red: Reduced, cams, pts, loss="linear", f_scale=1.0):
    """(J_free^T diag(w) J_free, free mask) of the whole reduced problem."""
    r = red.res(cams, pts)
    w = rl.weights(r, loss, f_scale).ravel()
    J = red.jac(red.x(cams, pts)).toarray()
    return J.T @ (w[:, None] * J), red.free


def embed(red: Reduced, Sigma_free):
    """Free-parameter matrix -> full parameter order with held rows / columns 0; returns (cam part (N, N), point blocks)."""
    m = red.free.size
    F = np.zeros((m, m))
    idx = np.nonzero(red.free)[0]
    F[np.ix_(idx, idx)] = Sigma_free
    n = red.ncol
    npt = red.pts.shape[0]
    pts = np.array([F[n + 3 * p:n + 3 * p + 3, n + 3 * p:n + 3 * p + 3] for p in range(npt)])
    return F[:n, :n], pts


def scaled_condition(S):
    """kappa_2 of S scaled by its diagonal, and the 2-norm of the scaled inverse."""
    d = 1.0 / np.sqrt(np.diag(S))
    St = S * d[:, None] * d[None, :]
    ev = np.linalg.eigvalsh(St)
    return float(ev[-1] / ev[0]), float(1.0 / ev[0]), d
