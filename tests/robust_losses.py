"""numpy statement of scipy least_squares' five losses (scipy/optimize/_lsq/least_squares.py), for the tests of the
robust losses the device implements (enum ba_loss).  Per scalar residual f with soft threshold C = f_scale:
z = (f / C)^2, rho-term C^2 rho(z), IRLS weight rho'(z), cost = 0.5 sum C^2 rho(z).  The terms are written without
cancellation (soft_l1 2 z / (sqrt(1 + z) + 1), cauchy log1p(z)), as on the device."""
import numpy as np

from oracle import ba_oracle as o

LOSSES = ("linear", "huber", "soft_l1", "cauchy", "arctan")
NEW_LOSSES = ("soft_l1", "cauchy", "arctan")


def rho(z, loss):
    """(rho(z), rho'(z)) elementwise."""
    z = np.asarray(z, dtype=np.float64)
    if loss == "linear":
        return z.copy(), np.ones_like(z)
    if loss == "huber":
        r0, r1, _ = o.huber_rho(z)
        return r0, r1
    if loss == "soft_l1":
        s = np.sqrt(1.0 + z)
        return 2.0 * z / (s + 1.0), 1.0 / s
    if loss == "cauchy":
        return np.log1p(z), 1.0 / (1.0 + z)
    if loss == "arctan":
        return np.arctan(z), 1.0 / (1.0 + z * z)
    raise ValueError(loss)


def weights(res, loss, f_scale=1.0):
    return rho((np.asarray(res) / f_scale) ** 2, loss)[1]


def cost(res, loss, f_scale=1.0):
    return 0.5 * f_scale ** 2 * float(rho((np.asarray(res) / f_scale) ** 2, loss)[0].sum())


def normal_equations(Jc, Jp, res, w, cam_idx, pt_idx, n_cams, n_pts, fixed_cam=-1):
    """Block normal equations J^T W J, J^T W r with per-scalar-residual weights w (Nobs,2): Hcc (Nc,NB,NB), bc (Nc,NB),
    Hpp (Np,3,3), bp (Np,3).  The fixed camera's blocks are zero."""
    if fixed_cam >= 0:
        Jc = Jc * (cam_idx != fixed_cam)[:, None, None]
    nb = Jc.shape[2]
    Jcw, Jpw = Jc * w[:, :, None], Jp * w[:, :, None]
    Hcc, bc = np.zeros((n_cams, nb, nb)), np.zeros((n_cams, nb))
    Hpp, bp = np.zeros((n_pts, 3, 3)), np.zeros((n_pts, 3))
    np.add.at(Hcc, cam_idx, np.einsum('nki,nkj->nij', Jcw, Jc))
    np.add.at(Hpp, pt_idx, np.einsum('nki,nkj->nij', Jpw, Jp))
    np.add.at(bc, cam_idx, np.einsum('nki,nk->ni', Jcw, res))
    np.add.at(bp, pt_idx, np.einsum('nki,nk->ni', Jpw, res))
    return Hcc, bc, Hpp, bp


def pack_upper(H):
    """(N,n,n) -> (N, n(n+1)/2) row-major upper triangle (the ABI's packed blocks)."""
    iu = np.triu_indices(H.shape[1])
    return H[:, iu[0], iu[1]]


def gradient_inf(Jc, Jp, res, loss, f_scale, cam_idx, pt_idx, n_cams, n_pts, fixed_cam):
    """max |J^T (rho'(z) r)| over the free parameters: the gradient of scipy's cost 0.5 sum C^2 rho(z)."""
    w = weights(res, loss, f_scale)
    _, bc, _, bp = normal_equations(Jc, Jp, res, w, cam_idx, pt_idx, n_cams, n_pts, fixed_cam)
    return max(float(np.abs(bc).max()), float(np.abs(bp).max()))


def inject_outliers(uv, frac, seed, lo=20.0, hi=200.0):
    """A copy of uv with round(frac * Nobs) observations moved by lo .. hi px in a random direction (gross mismatches)."""
    rng = np.random.default_rng(seed)
    uv = np.array(uv, dtype=np.float64, copy=True)
    n = int(round(frac * uv.shape[0]))
    idx = rng.choice(uv.shape[0], size=n, replace=False)
    ang = rng.uniform(0.0, 2.0 * np.pi, n)
    mag = rng.uniform(lo, hi, n)
    uv[idx, 0] += mag * np.cos(ang)
    uv[idx, 1] += mag * np.sin(ang)
    mask = np.zeros(uv.shape[0], dtype=bool)
    mask[idx] = True
    return uv, mask
