"""The reduced problem of a solve with held parameters (ba_set_held), stated with the oracle's residuals and Jacobian
blocks: held columns are dropped, the rest is what scipy's least_squares would see.  Test infrastructure only."""
import numpy as np
import scipy.sparse as sp
from scipy.optimize import least_squares

from oracle import ba_oracle as o
from tests import robust_losses as rl


def cam_bits(mask, nb):
    """(Nc,) uint bit masks -> (Nc, nb) bool."""
    return ((np.asarray(mask, dtype=np.int64)[:, None] >> np.arange(nb)[None]) & 1).astype(bool)


class Reduced:
    """Full parameters [cams (Nc, nb) | pts (Np, 3)]; free = columns neither held by the masks nor by fixed_cam.
    K4 None: the BAL 9-parameter camera."""

    def __init__(self, cams, pts, cam_idx, pt_idx, uv, K4, fixed_cam=-1, cam_mask=None, pt_held=None):
        self.cams, self.pts = np.array(cams, dtype=np.float64), np.array(pts, dtype=np.float64)
        self.ci, self.pi, self.uv, self.K4 = cam_idx, pt_idx, uv, K4
        nc, self.nb = self.cams.shape
        npt = self.pts.shape[0]
        hc = cam_bits(np.zeros(nc) if cam_mask is None else cam_mask, self.nb)
        if fixed_cam >= 0:
            hc[fixed_cam] = True
        hp = np.zeros(npt, bool) if pt_held is None else np.asarray(pt_held, bool)
        self.held_cam, self.held_pt = hc, hp
        self.free = np.concatenate([~hc.ravel(), np.repeat(~hp, 3)])
        self.ncol = nc * self.nb
        n = len(cam_idx)
        cc = self.nb * np.asarray(cam_idx, np.int64)[:, None] + np.arange(self.nb)[None]
        pc = self.ncol + 3 * np.asarray(pt_idx, np.int64)[:, None] + np.arange(3)[None]
        cols = np.concatenate([cc, pc], axis=1)                            # (n, nb + 3)
        self.rows = np.repeat(np.arange(2 * n).reshape(n, 2, 1), self.nb + 3, axis=2)
        self.cols = np.broadcast_to(cols[:, None, :], self.rows.shape)
        newcol = -np.ones(self.free.size, np.int64)
        newcol[self.free] = np.arange(self.free.sum())
        self.newcol = newcol

    def x_full(self, cams, pts):
        return np.concatenate([np.asarray(cams).ravel(), np.asarray(pts).ravel()])

    def x(self, cams, pts):
        return self.x_full(cams, pts)[self.free]

    def unpack(self, xf):
        full = self.x_full(self.cams, self.pts).copy()
        full[self.free] = xf
        return full[:self.ncol].reshape(-1, self.nb), full[self.ncol:].reshape(-1, 3)

    def res(self, cams, pts):
        if self.K4 is None:
            return o.bal_residuals(cams, pts, self.ci, self.pi, self.uv)
        return o.residuals(cams, pts, self.ci, self.pi, self.uv, self.K4)

    def blocks(self, cams, pts):
        """Jacobian blocks with the held columns zeroed."""
        if self.K4 is None:
            Jc, Jp = o.bal_jacobian_blocks(cams, pts, self.ci, self.pi)
        else:
            Jc, Jp = o.jacobian_blocks(cams, pts, self.ci, self.pi, self.K4)
        Jc = Jc * (~self.held_cam[self.ci])[:, None, :]
        Jp = Jp * (~self.held_pt[self.pi])[:, None, None]
        return Jc, Jp

    def fun(self, xf):
        return self.res(*self.unpack(xf)).ravel()

    def jac(self, xf):
        Jc, Jp = self.blocks(*self.unpack(xf))
        vals = np.concatenate([Jc, Jp], axis=2)
        nc = self.newcol[self.cols]
        keep = nc >= 0
        return sp.csr_matrix((vals[keep], (self.rows[keep], nc[keep])), shape=(self.rows.shape[0] * 2, int(self.free.sum())))

    def grad_inf(self, cams, pts, loss, f_scale=1.0):
        """max |gradient| over the free entries (scipy's gtol quantity on the reduced vector)."""
        r = self.res(cams, pts)
        w = rl.weights(r, loss, f_scale)
        g = self.jac(self.x(cams, pts)).T @ (w * r).ravel()
        return float(np.abs(g).max()) if g.size else 0.0

    def normal_equations(self, cams, pts, loss="linear", f_scale=1.0):
        """Hcc (Nc,nb,nb), bc (Nc,nb), Hpp (Np,3,3), bp (Np,3), W (Nobs,nb,3) with held rows / columns zero."""
        r = self.res(cams, pts)
        w = rl.weights(r, loss, f_scale)
        Jc, Jp = self.blocks(cams, pts)
        H, b, Hp, bpp = rl.normal_equations(Jc, Jp, r, w, self.ci, self.pi, self.cams.shape[0], self.pts.shape[0])
        W = np.einsum('nki,nkj->nij', Jc * w[:, :, None], Jp)
        return dict(Hcc=H, bc=b, Hpp=Hp, bp=bpp, W=W)

    def schur(self, ne, lam):
        """Dense S and rhs of the damped reduced system, embedded with identity rows / columns and zero rhs where held."""
        S, rhs, _, _ = o.schur_dense(ne, self.ci, self.pi, lam, -1)
        held = self.held_cam.ravel()
        S[held, :] = 0.0
        S[:, held] = 0.0
        S[held, held] = 1.0
        rhs = rhs.copy()
        rhs[held] = 0.0
        return S, rhs

    def certify(self, cams0, pts0, cams, pts, loss, f_scale=1.0, grad_ratio=1e-6, restart_drop=1e-9):
        """scipy's gradient over the free entries has dropped by grad_ratio, and a scipy restart from x* finds no decrease."""
        g0 = self.grad_inf(cams0, pts0, loss, f_scale)
        g = self.grad_inf(cams, pts, loss, f_scale)
        assert g <= grad_ratio * g0, (loss, g, g0)
        x = self.x(cams, pts)
        c = rl.cost(self.fun(x), loss, f_scale)
        sol = least_squares(self.fun, x, jac=self.jac, loss=loss, f_scale=f_scale, xtol=1e-5, ftol=1e-5, max_nfev=50)
        assert c - sol.cost <= restart_drop * c, (loss, c, sol.cost)
