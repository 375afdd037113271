"""Numpy yardstick of ba_transform / ba_align (include/ba_hip.h): the similarity X' = s R X + t applied to cameras and
points, the quaternion log map, weighted Umeyama with two-pass centring, the IRLS loop, errors and statuses.  Test
infrastructure: written from the formulas of the header, independent of the package's similarity.py and of the kernels.
Every sum is a plain loop-free numpy sum; `order` lets a caller permute the summation order to see what it is worth."""
import math

import numpy as np

OK, TOO_FEW, DEGENERATE = 0, 1, 2
LOSSES = ("linear", "huber", "soft_l1", "cauchy", "arctan")


def rodrigues(rvec):
    """(3,) -> (3, 3), cv2.Rodrigues' vector -> matrix (identity below DBL_EPSILON), as the library's camera state."""
    r = np.asarray(rvec, dtype=np.float64)
    th = math.sqrt(float(r @ r))
    if th < np.finfo(np.float64).eps:
        return np.eye(3)
    k = r / th
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return math.cos(th) * np.eye(3) + (1.0 - math.cos(th)) * np.outer(k, k) + math.sin(th) * K


def log_map(R):
    """(3, 3) rotation -> (3,) rotation vector through the unit quaternion picked by the largest of trace and diagonal
    entries (Shepperd), w >= 0, theta = 2 atan2(|v|, w); small-angle limit 2 v / w."""
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
    q = q / math.sqrt(float(q @ q))
    if q[0] < 0:
        q = -q
    vn = math.sqrt(float(q[1:] @ q[1:]))
    if vn < 1e-10:
        return 2.0 * q[1:] / q[0]
    return q[1:] * (2.0 * math.atan2(vn, q[0]) / vn)


def transform(cams, pts, s, R, t):
    """-> (cams', pts', R_c R^T (Nc, 3, 3)): R_c' = R_c R^T, t_c' = s t_c - R_c' t, rvec' = log(R_c'), X' = s R X + t.
    Columns of cams beyond 6 (f, k1, k2) are kept."""
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    t = np.asarray(t, dtype=np.float64).reshape(3)
    out = np.array(cams, dtype=np.float64)
    Rn = np.empty((out.shape[0], 3, 3))
    for c in range(out.shape[0]):
        Rn[c] = rodrigues(out[c, :3]) @ R.T
        out[c, :3] = log_map(Rn[c])
        out[c, 3:6] = s * np.asarray(cams[c, 3:6], dtype=np.float64) - Rn[c] @ t
    return out, s * (np.asarray(pts, dtype=np.float64) @ R.T) + t, Rn


def centres(cams):
    return np.stack([-rodrigues(c[:3]).T @ c[3:6] for c in np.asarray(cams, dtype=np.float64)])


def rho_prime(loss, z):
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
    raise ValueError(f"unknown loss {loss!r}")


def umeyama(a, b, u, with_scale=True):
    """Weighted closed form over the rows with u > 0 (given in the order they are to be summed).
    -> (status, s, R, t, mu_a, (mu_b, lo))."""
    W = u.sum()
    if not np.isfinite(W) or not W > 0:
        return DEGENERATE, 1.0, np.eye(3), np.zeros(3), np.zeros(3), (np.zeros(3), np.zeros(3))
    mu_a = (u[:, None] * a).sum(axis=0) / W
    mu_b = (u[:, None] * b).sum(axis=0) / W
    # second pass: centred.  A centroid of references at 5e6 is only known to its ulp, 9e-10, from the first pass; the centred
    # sum of the second pass gives what is left of it (lo), and the distances use mu_b + lo without rounding the sum
    lo = (u[:, None] * (b - mu_b)).sum(axis=0) / W
    x, y = a - mu_a, (b - mu_b) - lo
    Sigma = np.einsum("n,ni,nj->ij", u, y, x) / W
    var_a = (u * (x * x).sum(axis=1)).sum() / W
    if not (np.isfinite(Sigma).all() and np.isfinite(mu_a).all() and np.isfinite(mu_b).all() and np.isfinite(lo).all() and np.isfinite(var_a)) or not var_a > 0:
        return DEGENERATE, 1.0, np.eye(3), np.zeros(3), np.zeros(3), (np.zeros(3), np.zeros(3))
    U, D, Vt = np.linalg.svd(Sigma)
    if not D[1] > 1e-12 * D[0]:
        return DEGENERATE, 1.0, np.eye(3), np.zeros(3), np.zeros(3), (np.zeros(3), np.zeros(3))
    d = np.array([1.0, 1.0, np.sign(np.linalg.det(U) * np.linalg.det(Vt))])
    R = U @ np.diag(d) @ Vt
    s = float((D * d).sum() / var_a) if with_scale else 1.0
    return OK, s, R, (mu_b - s * R @ mu_a) + lo, mu_a, (mu_b, lo)


def distances(a, b, s, R, mu_a, mu_b):
    """d_i = |b_i - (s R a_i + t)| with t = mu_b - s R mu_a, evaluated as |(b_i - mu_b) - s R (a_i - mu_a)|: the same number
    without the rounding that a far-away t (5e6: an ulp of 1e-9) would put on every distance.  mu_b = (first pass, its
    second-pass correction)."""
    return np.sqrt(((((b - mu_b[0]) - mu_b[1]) - s * ((a - mu_a) @ R.T)) ** 2).sum(axis=1))


def align(a, b, w=None, loss="linear", f_scale=1.0, iters=10, with_scale=True, order=None):
    """a, b (n, 3); w (n,) or None (ones); rows with w = 0 have no reference (b may be NaN there).
    -> dict(status, s, R, t, rms, max, n_used, err (n,), NaN without a reference or without a similarity)."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    n = a.shape[0]
    w = np.ones(n) if w is None else np.asarray(w, dtype=np.float64)
    if not np.isfinite(w).all() or (w < 0).any():
        raise ValueError("negative or non-finite weight")
    if loss not in LOSSES or not f_scale > 0 or iters < 0:
        raise ValueError("bad options")
    use = np.nonzero(w > 0)[0]
    if order is not None:
        use = np.asarray(order)[np.isin(order, use)]
    out = dict(status=OK, s=1.0, R=np.eye(3), t=np.zeros(3), rms=np.nan, max=np.nan, n_used=int(use.size), err=np.full(n, np.nan))
    if use.size < 3:
        out["status"] = TOO_FEW
        return out
    au, bu, wu = a[use], b[use], w[use]
    status, s, R, t, mu_a, mu_b = umeyama(au, bu, wu, with_scale)
    for _ in range(iters):
        if status != OK:
            break
        d = distances(au, bu, s, R, mu_a, mu_b)
        u = wu * rho_prime(loss, wu * d * d / (f_scale * f_scale))
        keep = u > 0
        status, s, R, t, mu_a, mu_b = umeyama(au[keep], bu[keep], u[keep], with_scale)
    out["status"] = status
    if status != OK:
        return out
    d = distances(au, bu, s, R, mu_a, mu_b)
    out["err"][use] = d
    out.update(s=s, R=R, t=t, rms=float(np.sqrt((d * d).sum() / use.size)), max=float(d.max()))
    return out


def random_rotation(rng, angle=None):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    return rodrigues(axis * (rng.uniform(0.2, 3.0) if angle is None else angle))
