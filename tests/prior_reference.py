"""The objective of a solve with Gaussian priors (ba_set_priors), stated on top of tests/held_reference.Reduced and
tests/robust_losses: total cost and gradient, normal equations with + L, the dense reduced system, a dense LM step with
the model decrease of the library's lm_decide, and the "square-root rows" form [r ; R (x - mu)], R^T R = L, which is what
scipy.optimize.least_squares with loss='linear' solves.  Test infrastructure only."""
import numpy as np
import scipy.sparse as sp
from scipy.optimize import least_squares

from bundle_adjustment_amd.problem import BAProblem
from bundle_adjustment_amd.synthetic import make_problem
from tests import robust_losses as rl
from tests.held_reference import Reduced

DIAG_FLOOR = 1e-12          # the library's floor under a Marquardt diagonal entry


def random_rotation(rng, n):
    q, r = np.linalg.qr(rng.normal(size=(n, n)))
    return q * np.sign(np.diag(r))


def rotated_info(rng, sigmas):
    """A random rotation of diag(1 / sigma^2): a full SPD information block with the given principal standard deviations."""
    sigmas = np.asarray(sigmas, dtype=np.float64)
    q = random_rotation(rng, sigmas.size)
    L = q @ np.diag(1.0 / sigmas ** 2) @ q.T
    return 0.5 * (L + L.T)


def sqrt_rows(L):
    """R with R^T R = L for a symmetric positive semidefinite L (eigh: works for singular blocks); rows of zero
    eigenvalues are zero rows."""
    w, v = np.linalg.eigh(0.5 * (L + L.T))
    return np.sqrt(np.clip(w, 0.0, None))[:, None] * v.T


class PriorProblem:
    """red: the reduced problem (held parameters, fixed camera); cam_prior = (mean (Nc, nbp), info (Nc, nbp, nbp)) with
    nbp <= red.nb (6-coordinate priors on a 9-parameter camera fill the leading block), pt_prior = (mean (Np, 3),
    info (Np, 3, 3)); either may be None."""

    def __init__(self, red: Reduced, cam_prior=None, pt_prior=None):
        self.red = red
        nc, nb = red.cams.shape
        npt = red.pts.shape[0]
        self.cam_mean, self.cam_info = np.zeros((nc, nb)), np.zeros((nc, nb, nb))
        self.pt_mean, self.pt_info = np.zeros((npt, 3)), np.zeros((npt, 3, 3))
        if cam_prior is not None:
            m, L = np.asarray(cam_prior[0], dtype=np.float64), np.asarray(cam_prior[1], dtype=np.float64)
            k = m.shape[1]
            nz = L.reshape(nc, -1).any(axis=1)
            self.cam_mean[nz, :k] = m[nz]
            self.cam_info[:, :k, :k] = L
        if pt_prior is not None:
            m, L = np.asarray(pt_prior[0], dtype=np.float64), np.asarray(pt_prior[1], dtype=np.float64)
            nz = L.reshape(npt, -1).any(axis=1)
            self.pt_mean[nz] = m[nz]
            self.pt_info[:] = L
        # block-diagonal L and R over the FULL parameter vector [cams | pts]
        blocks = [self.cam_info[c] for c in range(nc)] + [self.pt_info[p] for p in range(npt)]
        self.L_full = sp.block_diag(blocks, format="csr")
        self.R_full = sp.block_diag([sqrt_rows(b) for b in blocks], format="csr")
        self.mu_full = np.concatenate([self.cam_mean.ravel(), self.pt_mean.ravel()])

    # ---- cost and gradient
    def prior_cost(self, cams, pts):
        dc = np.asarray(cams) - self.cam_mean
        dp = np.asarray(pts) - self.pt_mean
        return (0.5 * float(np.einsum('ci,cij,cj->', dc, self.cam_info, dc)),
                0.5 * float(np.einsum('pi,pij,pj->', dp, self.pt_info, dp)))

    def total_cost(self, cams, pts, loss="linear", f_scale=1.0):
        return rl.cost(self.red.res(cams, pts), loss, f_scale) + sum(self.prior_cost(cams, pts))

    def gradient(self, cams, pts, loss="linear", f_scale=1.0):
        """Gradient of the total objective over the free entries: J^T (rho' r) + L (x - mu); no loss on the prior terms."""
        red = self.red
        r = red.res(cams, pts)
        w = rl.weights(r, loss, f_scale)
        g = red.jac(red.x(cams, pts)).T @ (w * r).ravel()
        gp = self.L_full @ (red.x_full(cams, pts) - self.mu_full)
        return g + gp[red.free]

    def grad_inf(self, cams, pts, loss="linear", f_scale=1.0):
        return float(np.abs(self.gradient(cams, pts, loss, f_scale)).max())

    # ---- the system the library reports
    def normal_equations(self, cams, pts, loss="linear", f_scale=1.0):
        """Reduced.normal_equations with Hcc += L_c, bc += L_c (x_c - mu_c), Hpp += L_p, bp += L_p (X_p - mu_p), held rows
        and columns zero (a held parameter's prior is a constant of the cost)."""
        red = self.red
        ne = red.normal_equations(cams, pts, loss, f_scale)
        fc = ~red.held_cam
        fp = ~red.held_pt
        Lc = self.cam_info * fc[:, :, None] * fc[:, None, :]
        Lp = self.pt_info * fp[:, None, None]
        ne["Hcc"] = ne["Hcc"] + Lc
        ne["bc"] = ne["bc"] + np.einsum('cij,cj->ci', self.cam_info, np.asarray(cams) - self.cam_mean) * fc
        ne["Hpp"] = ne["Hpp"] + Lp
        ne["bp"] = ne["bp"] + np.einsum('pij,pj->pi', self.pt_info, np.asarray(pts) - self.pt_mean) * fp[:, None]
        return ne

    def schur(self, ne, lam):
        return self.red.schur(ne, lam)

    # ---- square-root rows
    def fun_aug(self, xf):
        cams, pts = self.red.unpack(xf)
        return np.concatenate([self.red.res(cams, pts).ravel(), self.R_full @ (self.red.x_full(cams, pts) - self.mu_full)])

    def jac_aug(self, xf):
        return sp.vstack([self.red.jac(xf), self.R_full[:, np.nonzero(self.red.free)[0]]], format="csr")

    # ---- dense Levenberg-Marquardt with the library's rules
    def dense_system(self, cams, pts, loss="linear", f_scale=1.0):
        """(A, g) over the free entries: A = J^T diag(w) J + L, g the total gradient."""
        red = self.red
        r = red.res(cams, pts)
        w = rl.weights(r, loss, f_scale).ravel()
        J = red.jac(red.x(cams, pts))
        idx = np.nonzero(red.free)[0]
        A = (J.T @ sp.diags(w) @ J + self.L_full[idx][:, idx]).toarray()
        return A, self.gradient(cams, pts, loss, f_scale)

    def dense_step(self, cams, pts, lam, loss="linear", f_scale=1.0):
        """One LM step d = (A + lam D)^-1 (-g), D = diag(max(A_ii, floor)); returns (cams + d, pts + d, d, model decrease
        0.5 (lam d^T D d - g^T d) of lm_decide with the inner solve exact, gain ratio on the total objective)."""
        A, g = self.dense_system(cams, pts, loss, f_scale)
        D = np.maximum(np.diag(A), DIAG_FLOOR)
        d = np.linalg.solve(A + lam * np.diag(D), -g)
        model = 0.5 * (lam * float(d @ (D * d)) - float(g @ d))
        c1, p1 = self.red.unpack(self.red.x(cams, pts) + d)
        c1 = c1 + 0.0
        # (unpack fills held entries from the reduced problem's own start values; the step leaves them alone)
        hc, hp = self.red.held_cam, self.red.held_pt
        c1[hc] = np.asarray(cams)[hc]
        p1[hp] = np.asarray(pts)[hp]
        gain = (self.total_cost(cams, pts, loss, f_scale) - self.total_cost(c1, p1, loss, f_scale)) / model
        return c1, p1, d, model, gain

    def dense_lm(self, cams, pts, loss="linear", f_scale=1.0, lam=1e-4, iters=50, grad_ratio=0.0):
        """LM from (cams, pts) with the library's damping rule (Nielsen's update on an accepted step, lam *= nu, nu *= 2
        on a rejected one).  Stops after `iters` steps or once max |g| <= grad_ratio max |g0|.  Returns (cams, pts, steps)."""
        cams, pts = np.array(cams, dtype=np.float64), np.array(pts, dtype=np.float64)
        g0 = self.grad_inf(cams, pts, loss, f_scale)
        nu, it = 2.0, 0
        while it < iters and self.grad_inf(cams, pts, loss, f_scale) > grad_ratio * g0:
            c1, p1, _, _, gain = self.dense_step(cams, pts, lam, loss, f_scale)
            it += 1
            if gain > 0 and np.isfinite(gain):
                cams, pts = c1, p1
                t = 2.0 * gain - 1.0
                lam = max(lam * max(1.0 / 3.0, 1.0 - t ** 3), 1e-12)
                nu = 2.0
            else:
                lam = min(lam * nu, 1e12)
                nu *= 2.0
        return cams, pts, it

    # ---- the certificate of a minimiser (Reduced.certify's two thresholds, on the total objective)
    def certify(self, cams0, pts0, cams, pts, loss="linear", f_scale=1.0, grad_ratio=1e-6, restart_drop=1e-9, restart=True,
                report=None):
        """The total gradient over the free entries has dropped by grad_ratio; and (linear loss, restart=True) a scipy
        restart on the square-root rows from x* finds no decrease beyond restart_drop.  report: a list that receives
        (gradient ratio, relative restart drop or None)."""
        g0 = self.grad_inf(cams0, pts0, loss, f_scale)
        g = self.grad_inf(cams, pts, loss, f_scale)
        drop = None
        if restart:
            assert loss == "linear", "scipy would apply the loss to the prior rows too"
            x = self.red.x(cams, pts)
            c = 0.5 * float(np.sum(self.fun_aug(x) ** 2))
            sol = least_squares(self.fun_aug, x, jac=self.jac_aug, loss="linear", xtol=1e-5, ftol=1e-5, max_nfev=50)
            drop = (c - sol.cost) / c
        if report is not None:
            report.append((g / g0, drop))
        assert g <= grad_ratio * g0, (loss, g, g0)
        if restart:
            assert drop <= restart_drop, (loss, drop)


def standard_input(seed=4, outlier_frac=0.0):
    """The input the prior tests share: make_problem(12, 800, 5, seed) with a FREE gauge (fixed_cam = -1); camera 0: a
    full 6 x 6 prior, a random rotation of diag(1 / sigma^2), sigma 1e-3 (rvec) and 5e-3 (t), mean = truth + one sigma of
    noise; camera 11: t only, I / 0.01^2; 5 % of the points: random rotations of diag(1 / s^2), s uniform in 0.01 .. 0.05 m,
    means = truth + noise.  Returns (problem, cam_prior (mean (Nc, 6), info (Nc, 6, 6)), pt_prior (mean, info))."""
    p, cams_true, pts_true = make_problem(12, 800, 5, seed=seed, outlier_frac=outlier_frac, return_truth=True)
    p = BAProblem(p.cams, p.pts, p.cam_idx, p.pt_idx, p.uv, p.K4, -1)
    rng = np.random.default_rng(1000 + seed)
    nc, npt = p.n_cams, p.n_pts
    cm, cL = np.zeros((nc, 6)), np.zeros((nc, 6, 6))
    sig0 = np.array([1e-3] * 3 + [5e-3] * 3)
    cL[0] = rotated_info(rng, sig0)
    cm[0] = cams_true[0] + sig0 * rng.normal(size=6)
    cL[nc - 1, 3:, 3:] = np.eye(3) / 0.01 ** 2
    cm[nc - 1, 3:] = cams_true[nc - 1, 3:] + 0.01 * rng.normal(size=3)
    pm, pL = np.zeros((npt, 3)), np.zeros((npt, 3, 3))
    for j in rng.choice(npt, size=npt // 20, replace=False):
        s = rng.uniform(0.01, 0.05, size=3)
        pL[j] = rotated_info(rng, s)
        pm[j] = pts_true[j] + s * rng.normal(size=3)
    return p, (cm, cL), (pm, pL)


def prior_covariance(pr: PriorProblem, cams, pts, loss="linear", f_scale=1.0):
    """tests/covariance_reference.schur_covariance for the system with priors: the same Schur-complement formulas on
    H + L, and a free point seen from one camera only is left out (NaN) only when it carries no prior.  Same keys."""
    from tests.covariance_reference import one_camera_points
    red = pr.red
    ne = pr.normal_equations(cams, pts, loss, f_scale)
    nc, nb = red.cams.shape
    npt = red.pts.shape[0]
    ci, pi = np.asarray(red.ci), np.asarray(red.pi)
    onecam = one_camera_points(ci, pi, npt, red.held_pt) & ~pr.pt_info.reshape(npt, -1).any(axis=1)
    skip = onecam | red.held_pt
    n = nb * nc
    S = np.zeros((n, n))
    for c in range(nc):
        S[nb * c:nb * c + nb, nb * c:nb * c + nb] = ne["Hcc"][c]
    r = red.res(cams, pts)
    w = rl.weights(r, loss, f_scale)
    Jc, _ = red.blocks(cams, pts)
    for q in np.nonzero(onecam[pi])[0]:
        c = ci[q]
        S[nb * c:nb * c + nb, nb * c:nb * c + nb] -= Jc[q].T @ (w[q][:, None] * Jc[q])
    keep = ~skip
    Vinv = np.zeros((npt, 3, 3))
    Vinv[keep] = np.linalg.inv(ne["Hpp"][keep])
    Wd = np.zeros((n, 3 * npt))
    for q in range(len(ci)):
        if not skip[pi[q]]:
            Wd[nb * ci[q]:nb * ci[q] + nb, 3 * pi[q]:3 * pi[q] + 3] += ne["W"][q]
    for p in np.nonzero(keep)[0]:
        wp = Wd[:, 3 * p:3 * p + 3]
        S -= wp @ Vinv[p] @ wp.T
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
    return dict(S=S, full=full, cams=cam_blocks, points=Pc, onecam=onecam, Wobs=ne["W"], Vinv=Vinv, ci=ci, pi=pi)
