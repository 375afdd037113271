"""The problem a BAL solve with shared intrinsics (ba_set_shared_intrinsics) minimises, stated on top of
tests/held_reference.Reduced, tests/prior_reference.PriorProblem and the oracle: with x the per-camera parameters (the free
entries of [cams (Nc, 9) | pts]) and y the shared ones -- a group's f, k1, k2 once -- x = E y.  Provides E from labels, the
dense shared normal equations E^T A E, a dense LM step with the model decrease of the library's lm_decide, the shared
gradient E^T g and the certificate of a minimiser on the y parametrisation.  Test infrastructure only."""
import numpy as np
import scipy.sparse as sp
from scipy.optimize import least_squares

from tests import robust_losses as rl
from tests.held_reference import Reduced
from tests.prior_reference import DIAG_FLOOR, PriorProblem


def normalise(labels):
    """Labels with every group of one member turned into -1 (an ungrouped camera)."""
    lab = np.asarray(labels, dtype=np.int64).copy()
    for g in np.unique(lab[lab >= 0]):
        if np.count_nonzero(lab == g) < 2:
            lab[lab == g] = -1
    return lab


def members(labels):
    """{label: ascending member indices} of the groups with two or more members."""
    lab = normalise(labels)
    return {int(g): np.nonzero(lab == g)[0] for g in np.unique(lab[lab >= 0])}


def expansion(labels, nc, npt, nb=9):
    """E (nb Nc + 3 Np, n_y), 0/1, x_full = E y: column per pose entry, per ungrouped intrinsic, per group intrinsic (at
    the position of the group's leader, its lowest member) and per point coordinate."""
    lab = normalise(labels)
    col = -np.ones(nb * nc + 3 * npt, dtype=np.int64)
    lead = {g: m[0] for g, m in members(lab).items()}
    n = 0
    for c in range(nc):
        for q in range(nb):
            if q >= 6 and lab[c] >= 0 and lead[int(lab[c])] != c:
                col[nb * c + q] = col[nb * lead[int(lab[c])] + q]
            else:
                col[nb * c + q] = n
                n += 1
    col[nb * nc:] = n + np.arange(3 * npt)
    n += 3 * npt
    rows = np.arange(col.size)
    return sp.csr_matrix((np.ones(col.size), (rows, col)), shape=(col.size, n))


class SharedProblem:
    """red: the reduced problem (held masks: the members of a group hold the same intrinsics); labels (Nc,); priors as
    PriorProblem takes them (nb = 9 blocks on members add up to the group's prior)."""

    def __init__(self, red: Reduced, labels, cam_prior=None, pt_prior=None):
        assert red.K4 is None and red.nb == 9, "shared intrinsics are a BAL notion"
        self.red = red
        self.pr = PriorProblem(red, cam_prior, pt_prior)
        self.labels = normalise(labels)
        nc, npt = red.cams.shape[0], red.pts.shape[0]
        E = expansion(self.labels, nc, npt)[np.nonzero(red.free)[0]]          # free x entries only
        keep = np.asarray(E.sum(axis=0)).ravel() > 0
        self.E = E[:, np.nonzero(keep)[0]].tocsr()                             # (n_free_x, n_y)
        # a shared entry counted once: the rows of x that are a column's first (leader) row
        Ec = self.E.tocsc()
        Ec.sort_indices()
        first = Ec.indices[Ec.indptr[:-1]]
        self.once = np.zeros(self.E.shape[0], bool)
        self.once[first] = True

    # ---- y <-> parameters
    def y(self, cams, pts):
        return self.red.x(cams, pts)[self.once]

    def unpack(self, y):
        return self.red.unpack(self.E @ y)

    def fun(self, y):
        return self.red.fun(self.E @ y)

    def jac(self, y):
        return (self.red.jac(self.E @ y) @ self.E).tocsr()

    def cost(self, cams, pts, loss="linear", f_scale=1.0):
        return self.pr.total_cost(cams, pts, loss, f_scale)

    def gradient(self, cams, pts, loss="linear", f_scale=1.0):
        """E^T of the per-camera gradient of the total objective."""
        return self.E.T @ self.pr.gradient(cams, pts, loss, f_scale)

    def grad_inf(self, cams, pts, loss="linear", f_scale=1.0):
        return float(np.abs(self.gradient(cams, pts, loss, f_scale)).max())

    # ---- dense Levenberg-Marquardt step with the library's rules
    def dense_system(self, cams, pts, loss="linear", f_scale=1.0):
        """(A_y, g_y, D_y): E^T (J^T w J + L) E, E^T g and the Marquardt diagonal E^T max(diag, floor) -- floored per camera."""
        red = self.red
        r = red.res(cams, pts)
        w = rl.weights(r, loss, f_scale).ravel()
        J = red.jac(red.x(cams, pts))
        idx = np.nonzero(red.free)[0]
        A = (J.T @ sp.diags(w) @ J + self.pr.L_full[idx][:, idx]).tocsr()
        D = np.maximum(A.diagonal(), DIAG_FLOOR)
        Ay = (self.E.T @ A @ self.E).toarray()
        return Ay, self.gradient(cams, pts, loss, f_scale), self.E.T @ D

    def dense_step(self, cams, pts, lam, loss="linear", f_scale=1.0):
        """d_y = (A_y + lam D_y)^-1 (-g_y).  Returns dict(step (the y step), cams, pts (trial parameters), model (0.5 (lam
        d^T D d - g^T d), lm_decide's with the inner solve exact), gain (ratio on the total objective))."""
        A, g, D = self.dense_system(cams, pts, loss, f_scale)
        d = np.linalg.solve(A + lam * np.diag(D), -g)
        model = 0.5 * (lam * float(d @ (D * d)) - float(g @ d))
        red = self.red
        c1, p1 = red.unpack(red.x(cams, pts) + self.E @ d)
        c1 = c1 + 0.0
        hc, hp = red.held_cam, red.held_pt
        c1[hc] = np.asarray(cams)[hc]
        p1[hp] = np.asarray(pts)[hp]
        gain = (self.cost(cams, pts, loss, f_scale) - self.cost(c1, p1, loss, f_scale)) / model
        return dict(step=d, cams=c1, pts=p1, model=model, gain=gain)

    def step_of(self, cams0, pts0, cams1, pts1):
        """The y step between two parameter sets (members agree: the leader's entries)."""
        return self.y(cams1, pts1) - self.y(cams0, pts0)

    # ---- the certificate of a minimiser, held_reference.Reduced.certify's two thresholds on the y parametrisation
    def certify(self, cams0, pts0, cams, pts, loss="linear", f_scale=1.0, grad_ratio=1e-6, restart_drop=1e-9, report=None):
        g0 = self.grad_inf(cams0, pts0, loss, f_scale)
        g = self.grad_inf(cams, pts, loss, f_scale)
        y = self.y(cams, pts)
        c = rl.cost(self.fun(y), loss, f_scale)
        sol = least_squares(self.fun, y, jac=self.jac, loss=loss, f_scale=f_scale, xtol=1e-5, ftol=1e-5, max_nfev=50)
        drop = (c - sol.cost) / c
        if report is not None:
            report.append((g / g0, drop))
        assert g <= grad_ratio * g0, (loss, g, g0)
        assert drop <= restart_drop, (loss, drop)
