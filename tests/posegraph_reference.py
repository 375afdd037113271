"""Numpy yardstick of ba_pose_graph / ba_pose_graph_system (include/ba_hip.h): the seven residuals of a Sim(3) edge, chi2
and IRLS weights, Jacobians by central differences with their own uncertainty, the dense normal equations, a dense LM
mirror with ba_solve's rules (exact inner solve), and the scenes the tests share.  Test infrastructure: written from the
formulas of the header, independent of the package's posegraph.py and of the kernels (whose Jacobians are analytic)."""
import math

import numpy as np

LOSSES = ("linear", "huber", "soft_l1", "cauchy", "arctan")
STATUS_CODE = {"max_iters": 0, "ftol": 1, "xtol": 2, "gtol": 3}
RING_INFO = np.diag([100.0, 100.0, 100.0, 25.0, 25.0, 25.0, 50.0])


# ---- rotations, batched -------------------------------------------------------------------------------------------------
def rodrigues(rvec):
    """(..., 3) -> (..., 3, 3): cv2.Rodrigues' vector -> matrix, identity below DBL_EPSILON (the library's camera state)."""
    r = np.asarray(rvec, dtype=np.float64)
    th = np.linalg.norm(r, axis=-1)
    small = th < np.finfo(np.float64).eps
    k = r / np.where(small, 1.0, th)[..., None]
    K = np.zeros(r.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0] = -k[..., 2], k[..., 1], k[..., 2]
    K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -k[..., 0], -k[..., 1], k[..., 0]
    c, s = np.cos(th)[..., None, None], np.sin(th)[..., None, None]
    R = c * np.eye(3) + (1.0 - c) * k[..., :, None] * k[..., None, :] + s * K
    R[small] = np.eye(3)
    return R


def log_map(R):
    """(..., 3, 3) -> (..., 3): the Shepperd-quaternion log map of the header, w >= 0, theta = 2 atan2(|v|, w)."""
    R = np.asarray(R, dtype=np.float64)
    shape = R.shape[:-2]
    R = R.reshape(-1, 3, 3)
    tr = R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2]
    which = np.argmax(np.stack([tr, R[:, 0, 0], R[:, 1, 1], R[:, 2, 2]], axis=1), axis=1)
    forms = (
        (1.0 + tr, R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]),
        (R[:, 2, 1] - R[:, 1, 2], 1.0 + R[:, 0, 0] - R[:, 1, 1] - R[:, 2, 2], R[:, 0, 1] + R[:, 1, 0], R[:, 0, 2] + R[:, 2, 0]),
        (R[:, 0, 2] - R[:, 2, 0], R[:, 0, 1] + R[:, 1, 0], 1.0 + R[:, 1, 1] - R[:, 0, 0] - R[:, 2, 2], R[:, 1, 2] + R[:, 2, 1]),
        (R[:, 1, 0] - R[:, 0, 1], R[:, 0, 2] + R[:, 2, 0], R[:, 1, 2] + R[:, 2, 1], 1.0 + R[:, 2, 2] - R[:, 0, 0] - R[:, 1, 1]),
    )
    q = np.empty((R.shape[0], 4))
    for k, form in enumerate(forms):
        sel = which == k
        for j in range(4):
            q[sel, j] = form[j][sel]
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q[q[:, 0] < 0] *= -1.0
    vn = np.linalg.norm(q[:, 1:], axis=1)
    small = vn < 1e-10
    k = np.where(small, 2.0 / np.where(small, q[:, 0], 1.0), 2.0 * np.arctan2(vn, q[:, 0]) / np.where(small, 1.0, vn))
    return (q[:, 1:] * k[:, None]).reshape(shape + (3,))


# ---- similarities rvec | t | s -------------------------------------------------------------------------------------------
def compose(outer, inner):
    """outer o inner of similarities (..., 7): x -> s R x + t."""
    outer, inner = np.asarray(outer, dtype=np.float64), np.asarray(inner, dtype=np.float64)
    Ro, Ri = rodrigues(outer[..., :3]), rodrigues(inner[..., :3])
    out = np.empty(np.broadcast(outer, inner).shape)
    out[..., :3] = log_map(Ro @ Ri)
    out[..., 3:6] = outer[..., 6:7] * np.einsum("...ij,...j->...i", Ro, inner[..., 3:6]) + outer[..., 3:6]
    out[..., 6] = outer[..., 6] * inner[..., 6]
    return out


def inverse(sim):
    sim = np.asarray(sim, dtype=np.float64)
    R = rodrigues(sim[..., :3])
    out = np.empty(sim.shape)
    out[..., :3] = -sim[..., :3]
    out[..., 3:6] = -np.einsum("...ji,...j->...i", R, sim[..., 3:6]) / sim[..., 6:7]
    out[..., 6] = 1.0 / sim[..., 6]
    return out


def relative(pose_i, pose_j):
    """The measurement an edge (i, j) carries when both poses are exact: S_j o S_i^-1."""
    return compose(pose_j, inverse(pose_i))


def retract(poses, d):
    """R <- exp(d_omega) R, t <- t + d_t, s <- s exp(d_sigma); rvec through the log map."""
    poses, d = np.asarray(poses, dtype=np.float64), np.asarray(d, dtype=np.float64)
    out = poses.copy()
    out[..., :3] = log_map(rodrigues(d[..., :3]) @ rodrigues(poses[..., :3]))
    out[..., 3:6] = poses[..., 3:6] + d[..., 3:6]
    out[..., 6] = poses[..., 6] * np.exp(d[..., 6])
    return out


# ---- residuals, losses ---------------------------------------------------------------------------------------------------
def edge_residual(pi, pj, meas):
    """(m, 7) poses of both ends and (m, 7) measurements -> e (m, 7)."""
    Ri, Rj, Rm = rodrigues(pi[:, :3]), rodrigues(pj[:, :3]), rodrigues(meas[:, :3])
    Rr = Rj @ np.swapaxes(Ri, 1, 2)
    sr = pj[:, 6] / pi[:, 6]
    e = np.empty((pi.shape[0], 7))
    e[:, :3] = log_map(np.swapaxes(Rm, 1, 2) @ Rr)
    e[:, 3:6] = pj[:, 3:6] - sr[:, None] * np.einsum("eij,ej->ei", Rr, pi[:, 3:6]) - meas[:, 3:6]
    e[:, 6] = np.log(sr / meas[:, 6])
    return e


def residuals(poses, ei, ej, meas):
    poses = np.asarray(poses, dtype=np.float64)
    return edge_residual(poses[ei], poses[ej], np.asarray(meas, dtype=np.float64))


def _info(info, m):
    return np.broadcast_to(np.eye(7), (m, 7, 7)) if info is None else np.asarray(info, dtype=np.float64).reshape(m, 7, 7)


def chi2(e, info):
    return np.einsum("ei,eij,ej->e", e, _info(info, e.shape[0]), e)


def rho(loss, z):
    z = np.asarray(z, dtype=np.float64)
    if loss == "linear":
        return z.copy()
    if loss == "huber":
        return np.where(z <= 1.0, z, 2.0 * np.sqrt(z) - 1.0)
    if loss == "soft_l1":
        return 2.0 * (np.sqrt(1.0 + z) - 1.0)
    if loss == "cauchy":
        return np.log1p(z)
    if loss == "arctan":
        return np.arctan(z)
    raise ValueError(loss)


def rho_prime(loss, z):
    z = np.asarray(z, dtype=np.float64)
    if loss == "linear":
        return np.ones_like(z)
    if loss == "huber":
        return np.where(z <= 1.0, 1.0, 1.0 / np.sqrt(np.maximum(z, 1.0)))
    if loss == "soft_l1":
        return 1.0 / np.sqrt(1.0 + z)
    if loss == "cauchy":
        return 1.0 / (1.0 + z)
    if loss == "arctan":
        return 1.0 / (1.0 + z * z)
    raise ValueError(loss)


def cost(poses, ei, ej, meas, info=None, loss="linear", f_scale=1.0):
    """-> (cost = 0.5 f_scale^2 sum rho(chi2 / f_scale^2), chi2 (m,), weights (m,))."""
    c2 = chi2(residuals(poses, ei, ej, meas), info)
    z = c2 / f_scale ** 2
    return 0.5 * f_scale ** 2 * float(rho(loss, z).sum()), c2, rho_prime(loss, z)


# ---- Jacobians by central differences ------------------------------------------------------------------------------------
def _jac_fd(pi, pj, meas, h):
    m = pi.shape[0]
    A, B = np.empty((m, 7, 7)), np.empty((m, 7, 7))
    for c in range(7):
        d = np.zeros((m, 7))
        d[:, c] = h
        A[:, :, c] = (edge_residual(retract(pi, d), pj, meas) - edge_residual(retract(pi, -d), pj, meas)) / (2.0 * h)
        B[:, :, c] = (edge_residual(pi, retract(pj, d), meas) - edge_residual(pi, retract(pj, -d), meas)) / (2.0 * h)
    return A, B


def jacobians(poses, ei, ej, meas, h=1e-4):
    """A = de/dd_i, B = de/dd_j (m, 7, 7) at d = 0 by central differences at h and h / 2, Richardson-extrapolated, and d_fd =
    the largest difference between the two steps: the yardstick's own uncertainty."""
    poses, meas = np.asarray(poses, dtype=np.float64), np.asarray(meas, dtype=np.float64)
    pi, pj = poses[ei], poses[ej]
    A1, B1 = _jac_fd(pi, pj, meas, h)
    A2, B2 = _jac_fd(pi, pj, meas, 0.5 * h)
    d_fd = max(float(np.abs(A1 - A2).max()), float(np.abs(B1 - B2).max()))
    return (4.0 * A2 - A1) / 3.0, (4.0 * B2 - B1) / 3.0, d_fd


def _skew(v):
    S = np.zeros(v.shape[:-1] + (3, 3))
    S[..., 0, 1], S[..., 0, 2], S[..., 1, 0] = -v[..., 2], v[..., 1], v[..., 2]
    S[..., 1, 2], S[..., 2, 0], S[..., 2, 1] = -v[..., 0], -v[..., 1], v[..., 0]
    return S


def jacobians_analytic(poses, ei, ej, meas):
    """The closed form of the header's chart, for the LM mirror (central differences carry 1e-8, which a quadratically
    converging iteration squares into the cost): with N = Jl^-1(e_rot) R_ij^T, q = s_r R_r t_i,
    B = [N 0 0; [q]x I -q; 0 0 1], A = [-N R_r 0 0; -[q]x R_r, -s_r R_r, q; 0 0 -1].  test_posegraph_host.py holds it
    against jacobians() within that one's d_fd."""
    poses, meas = np.asarray(poses, dtype=np.float64), np.asarray(meas, dtype=np.float64)
    pi, pj = poses[ei], poses[ej]
    m = pi.shape[0]
    Ri, Rj, Rm = rodrigues(pi[:, :3]), rodrigues(pj[:, :3]), rodrigues(meas[:, :3])
    Rr = Rj @ np.swapaxes(Ri, 1, 2)
    RmT = np.swapaxes(Rm, 1, 2)
    er = log_map(RmT @ Rr)
    sr = pj[:, 6] / pi[:, 6]
    q = sr[:, None] * np.einsum("eij,ej->ei", Rr, pi[:, 3:6])
    t2 = (er * er).sum(axis=1)
    th = np.sqrt(t2)
    big = t2 >= 1e-4
    hh = 0.5 * np.where(big, th, 1.0)
    cc = np.where(big, (1.0 - hh * np.cos(hh) / np.sin(hh)) / np.where(big, t2, 1.0), 1.0 / 12.0 + t2 / 720.0 + t2 * t2 / 30240.0)
    S = _skew(er)
    N = (np.eye(3) - 0.5 * S + cc[:, None, None] * (S @ S)) @ RmT
    Q = _skew(q)
    A, B = np.zeros((m, 7, 7)), np.zeros((m, 7, 7))
    B[:, :3, :3], B[:, 3:6, :3], B[:, 3:6, 3:6], B[:, 3:6, 6], B[:, 6, 6] = N, Q, np.eye(3), -q, 1.0
    A[:, :3, :3], A[:, 3:6, :3], A[:, 3:6, 3:6], A[:, 3:6, 6], A[:, 6, 6] = -N @ Rr, -Q @ Rr, -sr[:, None, None] * Rr, q, -1.0
    return A, B


# ---- the dense system -----------------------------------------------------------------------------------------------------
def held_mask(n, ei, ej, held=None, with_scale=True):
    """(n, 7) bool: whole held nodes, every d_sigma without scale, every node without an incident edge."""
    mk = np.zeros((n, 7), bool)
    if held is not None:
        mk[np.asarray(held, bool)] = True
    if not with_scale:
        mk[:, 6] = True
    deg = np.bincount(np.concatenate([ei, ej]).astype(np.int64), minlength=n)
    mk[deg == 0] = True
    return mk


def dense_system(n, ei, ej, e, A, B, info, w, mask, lam=0.0):
    """-> (H + lam D with the held rows as identity rows, g with zeros there, D): H = sum w [A B]^T info [A B]."""
    m = len(ei)
    info = _info(info, m)
    H = np.zeros((7 * n, 7 * n))
    g = np.zeros(7 * n)
    for q in range(m):
        i, j = 7 * int(ei[q]), 7 * int(ej[q])
        W = w[q] * info[q]
        WA, WB, We = W @ A[q], W @ B[q], W @ e[q]
        H[i:i + 7, i:i + 7] += A[q].T @ WA
        H[j:j + 7, j:j + 7] += B[q].T @ WB
        H[i:i + 7, j:j + 7] += A[q].T @ WB
        H[j:j + 7, i:i + 7] += B[q].T @ WA
        g[i:i + 7] += A[q].T @ We
        g[j:j + 7] += B[q].T @ We
    hm = mask.reshape(-1)
    H[hm, :] = 0.0
    H[:, hm] = 0.0
    g[hm] = 0.0
    D = np.maximum(np.diag(H), 1e-12)
    D[hm] = 0.0
    H = H + lam * np.diag(D)
    H[hm, hm] = 1.0
    return H, g, D


def system(poses, ei, ej, meas, info=None, held=None, loss="linear", f_scale=1.0, with_scale=True, lam=0.0, h=1e-4, analytic=False):
    """Everything ba_pose_graph_system returns, plus d_fd, chi2 and the weights.  analytic: the closed-form Jacobians
    (d_fd = 0) instead of central differences."""
    poses = np.asarray(poses, dtype=np.float64)
    n = poses.shape[0]
    e = residuals(poses, ei, ej, meas)
    if analytic:
        (A, B), d_fd = jacobians_analytic(poses, ei, ej, meas), 0.0
    else:
        A, B, d_fd = jacobians(poses, ei, ej, meas, h)
    c2 = chi2(e, info)
    w = rho_prime(loss, c2 / f_scale ** 2)
    mask = held_mask(n, ei, ej, held, with_scale)
    H, g, D = dense_system(n, ei, ej, e, A, B, info, w, mask, lam)
    return dict(e=e, A=A, B=B, d_fd=d_fd, chi2=c2, w=w, H=H, g=g, D=D, mask=mask)


# ---- the LM mirror --------------------------------------------------------------------------------------------------------
def lm_solve(poses, ei, ej, meas, info=None, held=None, loss="linear", f_scale=1.0, with_scale=True, max_iters=50, ftol=1e-5,
             xtol=1e-5, gtol=1e-8, lam0=1e-4, h=1e-4, analytic=True):
    """Dense mirror of ba_pose_graph with ba_solve's rules (oracle.lm_solve's, linear_solver='dense'): damping matrix
    D = max(diag H, 1e-12), exact solve of (H + lam D) d = -g, model decrease 0.5 (lam d.D d - g.d), Nielsen's update,
    gtol on max |g| before a step, ftol on an accepted step, xtol on |d| against |x| of the free entries.  analytic=False:
    the Jacobians by central differences.
    Returns dict(poses, cost0, cost, sse, iterations, accepted, status, lam, history[it, cost, cost_new, lam, rho, step])."""
    poses = np.array(poses, dtype=np.float64)
    ei, ej = np.asarray(ei, dtype=np.int64), np.asarray(ej, dtype=np.int64)
    meas = np.asarray(meas, dtype=np.float64)
    n = poses.shape[0]
    mask = held_mask(n, ei, ej, held, with_scale)
    free = ~mask.reshape(-1)
    cst, c2, _ = cost(poses, ei, ej, meas, info, loss, f_scale)
    cost0 = cst
    lam, nu = lam0, 2.0
    it = acc = 0
    status = "max_iters"
    hist = []
    sys_ = None
    while it < max_iters:
        if sys_ is None:
            sys_ = system(poses, ei, ej, meas, info, held, loss, f_scale, with_scale, 0.0, h, analytic=analytic)
        H0, g, D = sys_["H"], sys_["g"], sys_["D"]
        if np.abs(g).max() <= gtol:
            status = "gtol"
            break
        d = np.zeros(7 * n)
        Hf = H0[np.ix_(free, free)] + lam * np.diag(D[free])
        d[free] = np.linalg.solve(Hf, -g[free])
        model = 0.5 * (lam * float((D * d * d).sum()) - float(g @ d))
        new = retract(poses, d.reshape(n, 7))
        new[mask[:, :3].all(axis=1), :3] = poses[mask[:, :3].all(axis=1), :3]
        cost_new, c2_new, _ = cost(new, ei, ej, meas, info, loss, f_scale)
        gain = (cst - cost_new) / model if model > 0 else -1.0
        step = math.sqrt(float(d @ d))
        xnorm = math.sqrt(float((poses.reshape(-1)[free] ** 2).sum()))
        it += 1
        hist.append(dict(it=it, cost=cst, cost_new=cost_new, lam=lam, rho=gain, step=step))
        if gain > 0 and np.isfinite(cost_new):
            dcost = cst - cost_new
            poses, cst, c2 = new, cost_new, c2_new
            sys_ = None
            acc += 1
            lam = max(lam * max(1.0 / 3.0, 1.0 - (2.0 * gain - 1.0) ** 3), 1e-12)
            nu = 2.0
            if dcost <= ftol * cst:
                status = "ftol"
                break
        else:
            lam = min(lam * nu, 1e12)
            nu *= 2.0
        if step <= xtol * (xtol + xnorm):
            status = "xtol"
            break
    return dict(poses=poses, cost0=cost0, cost=cst, sse=float(c2.sum()), iterations=it, accepted=acc, status=status, lam=lam,
                history=hist)


# ---- scenes ----------------------------------------------------------------------------------------------------------------
def circle_poses(n, radius=5.0):
    """n world-to-node similarities (s = 1) on a circle in the x-z plane, each turned about y by its angle."""
    poses = np.zeros((n, 7))
    for k in range(n):
        a = 2.0 * math.pi * k / n
        R = rodrigues(np.array([0.0, a, 0.0]))
        c = np.array([radius * math.cos(a), 0.0, radius * math.sin(a)])
        poses[k, :3] = log_map(R)
        poses[k, 3:6] = -R @ c
        poses[k, 6] = 1.0
    return poses


def drifted_start(truth, with_scale=True, scale=1.01, rot=(0.0, 0.01, 0.002), shift=0.02):
    """Odometry integrated from node 0 with a drift per step: scale x 1.01 (Sim(3) only), a rotation of `rot` rad and `shift`
    on every component of t.  The drift is a similarity composed on the LEFT of each exact odometry measurement, i.e. in the
    frame of the node being reached: S_{k+1} = drift o meas_{k,k+1} o S_k.  For the 16-node ring this gives an initial cost of
    15.5 and a loop-edge residual of |e| = 1.06, 5.5 when whitened by the information block."""
    n = truth.shape[0]
    out = truth.copy()
    for k in range(n - 1):
        ms = relative(truth[k], truth[k + 1])
        drift = np.array([rot[0], rot[1], rot[2], shift, shift, shift, scale if with_scale else 1.0])
        out[k + 1] = compose(compose(drift, ms), out[k])
    if not with_scale:
        out[:, 6] = 1.0
    return out


def ring(n=16, with_scale=True, skip_every=3, n_skips=None):
    """The ring of the tests: odometry edges (k, k + 1), the loop edge (n - 1, 0), skip edges (k, k + 2) for k = 0,
    skip_every, ...; exact measurements, info = diag(100 x 3, 25 x 3, 50), node 0 held, the drifted start.
    -> dict(truth, start, ei, ej, meas, info, held)."""
    truth = circle_poses(n)
    pairs = [(k, k + 1) for k in range(n - 1)] + [(n - 1, 0)] + [(k, k + 2) for k in range(0, n - 2, skip_every)]
    ei = np.array([p[0] for p in pairs], dtype=np.int32)
    ej = np.array([p[1] for p in pairs], dtype=np.int32)
    meas = relative(truth[ei], truth[ej])
    info = np.broadcast_to(RING_INFO, (len(pairs), 7, 7)).copy()
    held = np.zeros(n, np.uint8)
    held[0] = 1
    return dict(truth=truth, start=drifted_start(truth, with_scale), ei=ei, ej=ej, meas=meas, info=info, held=held)


def with_false_edge(sc, i=3, j=11):
    """The scene plus one false loop closure (i, j): the true relative pose off by s x 1.3, (0.3, 0, 0.2) rad, t + 1.  The
    false edge is the LAST one."""
    ms = relative(sc["truth"][i], sc["truth"][j])
    bad = compose(np.array([0.3, 0.0, 0.2, 0.0, 0.0, 0.0, 1.0]), ms)
    bad[3:6] = ms[3:6] + 1.0
    bad[6] = ms[6] * 1.3
    out = dict(sc)
    out["ei"] = np.append(sc["ei"], np.int32(i)).astype(np.int32)
    out["ej"] = np.append(sc["ej"], np.int32(j)).astype(np.int32)
    out["meas"] = np.vstack([sc["meas"], bad])
    out["info"] = np.concatenate([sc["info"], RING_INFO[None]])
    return out


def pose_distance(a, b):
    """Largest absolute difference of two pose arrays, rotations compared through R_a R_b^T (rvec is two-valued at pi)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    rot = np.abs(log_map(rodrigues(a[:, :3]) @ np.swapaxes(rodrigues(b[:, :3]), 1, 2))).max()
    return max(float(rot), float(np.abs(a[:, 3:] - b[:, 3:]).max()))


# ---- large rings, vectorised ------------------------------------------------------------------------------------------------
def big_ring(n, chord_every=97, held_every=64, seed=0):
    """A ring of n nodes for the node and edge grids (n in the thousands; no Python loop over the nodes): odometry edges
    (k, k + 1 mod n), n // chord_every chords (chord_every c, chord_every c + n // 3 mod n), info = RING_INFO, measurements
    with N(0, 3e-3 rad | 2e-2 | 3e-3) noise.  The minimiser absorbs most of that noise -- 7 n unknowns against
    7 (n + n // chord_every) residuals -- and leaves chi2 of 6e-4 per edge on average, so a robust loss needs an f_scale of
    about 0.02 for its weights to differ at the end.  Every held_every-th node is held, from node held_every // 2 on: the
    last node of a ring of a multiple of held_every nodes, plus one, is free.  The start is the truth moved by a similarity
    that grows along the ring (0.02 rad, 0.05 in t, 2 % in scale at its end: the loop edge sees all of it) and by
    N(0, 1e-3 rad | 1e-2 | 1e-3) per node; held nodes start at the truth.  Every node has degree 2 to 4.
    -> dict(truth, start, ei, ej, meas, info, held)."""
    rng = np.random.default_rng(seed)
    k = np.arange(n)
    a = 2.0 * math.pi * k / n
    Rt = rodrigues(np.stack([np.zeros(n), a, np.zeros(n)], axis=1))
    c = np.stack([5.0 * np.cos(a), np.zeros(n), 5.0 * np.sin(a)], axis=1)
    truth = np.concatenate([log_map(Rt), -np.einsum("nij,nj->ni", Rt, c), np.ones((n, 1))], axis=1)
    chords = np.arange(n // chord_every) * chord_every
    ei = np.concatenate([k, chords]).astype(np.int32)
    ej = np.concatenate([(k + 1) % n, (chords + n // 3) % n]).astype(np.int32)
    f = (k / n)[:, None]
    drift = np.concatenate([f * np.array([[0.0, 0.02, 0.004]]), f * 0.05 * np.ones((1, 3)), 1.0 + 0.02 * f], axis=1)
    noise = np.concatenate([rng.normal(0.0, 1e-3, (n, 3)), rng.normal(0.0, 1e-2, (n, 3)), rng.normal(0.0, 1e-3, (n, 1))], axis=1)
    start = retract(compose(drift, truth), noise)
    held = (k % held_every == held_every // 2).astype(np.uint8)
    start[held != 0] = truth[held != 0]
    m = len(ei)
    mnoise = np.concatenate([rng.normal(0.0, 3e-3, (m, 3)), rng.normal(0.0, 2e-2, (m, 3)), np.exp(rng.normal(0.0, 3e-3, (m, 1)))], axis=1)
    return dict(truth=truth, start=start, ei=ei, ej=ej, meas=compose(mnoise, relative(truth[ei], truth[ej])),
                info=np.broadcast_to(RING_INFO, (m, 7, 7)).copy(), held=held)


def gradient(poses, ei, ej, meas, info, w, mask):
    """g = sum_e w_e [A B]^T info e scattered to the nodes with np.add.at (held entries 0), and the same sum of absolute
    values: (g (n, 7), sum |terms| (n, 7))."""
    poses = np.asarray(poses, dtype=np.float64)
    n, m = poses.shape[0], len(ei)
    A, B = jacobians_analytic(poses, ei, ej, meas)
    We = w[:, None] * np.einsum("eij,ej->ei", _info(info, m), residuals(poses, ei, ej, meas))
    g, ga = np.zeros((n, 7)), np.zeros((n, 7))
    for J, idx in ((A, ei), (B, ej)):
        np.add.at(g, idx, np.einsum("eai,ea->ei", J, We))
        np.add.at(ga, idx, np.einsum("eai,ea->ei", np.abs(J), np.abs(We)))
    g[mask] = 0.0
    return g, ga
