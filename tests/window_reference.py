"""A dense Levenberg-Marquardt for window-sized problems with held parameters, any of the five losses and f_scale: the
reference tests/test_gpu_window_held.py follows the two single-launch window kernels against (csrc/ba_small.hpp,
csrc/ba_small_mw.hpp).  Test infrastructure only; plain float64 numpy.

Formulated apart from the device on purpose: no Schur complement, no per-point inverse, no identity rows.  Held columns
are simply absent (held_reference.Reduced), and every step solves the FULL damped normal equations over the free
columns, cameras and points together,
    (J^T W J + lam diag(max(diag(J^T W J), 1e-12))) d = -J^T W r        (np.linalg.solve),
with W = rho'((r / f_scale)^2) per scalar residual (robust_losses).  What is shared with the kernels is the driver they
document: model decrease 0.5 (lam d^T D d - g^T d), gain ratio, Nielsen's damping with its floors, a rejected step
keeps the linearisation, and the exits in the kernels' order -- gtol on max |g| over the free entries at every new
linearisation, then per step ftol (dcost <= ftol * cost_new, accepted steps only), xtol (|d| <= xtol (xtol + |x|), |x|
over the free entries plus the fixed camera's block), max_iters.

step_by_elimination is the same step the device's way (block normal equations, Schur complement, back substitution), kept
apart from window_lm's own path: the host test uses the difference between the two as each case's conditioning."""
import numpy as np

from tests import robust_losses as rl
from tests.held_reference import Reduced

DIAG_FLOOR = 1e-12
MUTANTS = ("x_all", "g_all", "pt_coupled", "cam_coupled", "unit_scale")


def _reduced(p, cam_mask, pt_held):
    return Reduced(p.cams, p.pts, p.cam_idx, p.pt_idx, p.uv, p.K4, p.fixed_cam, cam_mask, pt_held)


def linearise(red, cams, pts, loss, f_scale):
    """-> (H = J^T W J dense over red's free columns, g = J^T W r)."""
    r = red.res(cams, pts)
    w = rl.weights(r, loss, f_scale).ravel()
    J = red.jac(red.x(cams, pts))
    JW = J.T.multiply(w[None, :]).tocsr()
    return np.asarray((JW @ J).todense()), np.asarray(JW @ r.ravel()).ravel()


def damped_step(H, g, lam):
    D = np.maximum(np.diag(H), DIAG_FLOOR)
    return np.linalg.solve(H + lam * np.diag(D), -g), D


def window_lm(problem, cam_mask=None, pt_held=None, loss="linear", f_scale=1.0, max_iters=50, ftol=1e-10, xtol=1e-10,
              gtol=1e-10, lam0=1e-4, mutate=None, by_elimination=False):
    """problem: a BAProblem (its fixed_cam is held whole); cam_mask: (Nc,) bit masks of held camera parameters; pt_held:
    (Np,) bool.  Returns what oracle.lm_solve returns -- cams, pts, iterations, accepted, cost0, cost, sse0, sse,
    pcg_iters = 0, status, history, lam, gmax -- with history records it, cost, cost_new, lam, rho, pcg = 0, step, gmax,
    xnorm, so lm_trace.check_follows and from_oracle take it as it is.
    mutate: a fault of a window kernel that still converges (tests of the tests) --
      'x_all'        held entries counted in xtol's |x|
      'g_all'        held entries' gradient counted in gtol's maximum
      'pt_coupled'   a held point is solved for as if free (its columns stay in the system), only its step is dropped
      'cam_coupled'  the same for held camera parameters
      'unit_scale'   IRLS weights rho'(r^2) instead of rho'((r / f_scale)^2)
    by_elimination: every step from step_by_elimination instead of the full system -- the same mathematics in the
    device's order of operations; how far the two runs drift apart is how well the case is conditioned."""
    if mutate is not None and mutate not in MUTANTS:
        raise ValueError(f"unknown mutant {mutate!r}")
    p = problem
    red = _reduced(p, cam_mask, pt_held)                       # the problem that is solved
    # the columns the (possibly faulty) linear system is written over, and those the gradient maximum looks at
    sys_ = _reduced(p, None if mutate == "cam_coupled" else cam_mask, None if mutate == "pt_coupled" else pt_held)
    wide = _reduced(p, None, None)
    w_scale = 1.0 if mutate == "unit_scale" else f_scale
    in_sys = red.free[sys_.free]                               # red's entries among the system's
    fixed_block = np.zeros(red.free.size, bool)
    if p.fixed_cam >= 0:
        fixed_block[6 * p.fixed_cam:6 * p.fixed_cam + 6] = True
    x_mask = np.ones(red.free.size, bool) if mutate == "x_all" else (red.free | fixed_block)

    cams, pts = red.cams.copy(), red.pts.copy()
    res = red.res(cams, pts)
    cost = cost0 = rl.cost(res, loss, f_scale)
    sse0 = float((res * res).sum())
    lam, nu = float(lam0), 2.0
    it = acc = 0
    status, hist, gmax = "max_iters", [], float("nan")
    need_lin = True
    while it < max_iters:
        if need_lin:
            H, g = linearise(sys_, cams, pts, loss, w_scale)
            gmax = float(np.abs(g[in_sys]).max()) if in_sys.any() else 0.0
            if mutate == "g_all":
                gmax = float(np.abs(linearise(wide, cams, pts, loss, w_scale)[1]).max())
            if gtol > 0 and gmax <= gtol:
                status = "gtol"
                break
        d_sys, D_sys = damped_step(H, g, lam)
        if by_elimination:
            if mutate is not None:
                raise ValueError("the mutants are written over the full system")
            d_sys = step_by_elimination(red, cams, pts, loss, f_scale, lam)
        d, D, gf = d_sys[in_sys], D_sys[in_sys], g[in_sys]     # the step that is taken: the free entries alone
        model = 0.5 * (lam * float((D * d * d).sum()) - float((gf * d).sum()))
        x = red.x(cams, pts)
        cams_new, pts_new = red.unpack(x + d)
        cost_new = rl.cost(red.res(cams_new, pts_new), loss, f_scale)
        rho = (cost - cost_new) / model if (model > 0 and np.isfinite(cost_new)) else -1.0
        step = float(np.sqrt((d * d).sum()))
        xnorm = float(np.sqrt((red.x_full(cams, pts)[x_mask] ** 2).sum()))
        it += 1
        hist.append(dict(it=it, cost=cost, cost_new=cost_new, lam=lam, rho=rho, pcg=0, step=step, gmax=gmax, xnorm=xnorm))
        stop = False
        need_lin = bool(rho > 0 and np.isfinite(cost_new))
        if need_lin:
            dcost = cost - cost_new
            cams, pts, cost = cams_new, pts_new, cost_new
            acc += 1
            lam = max(lam * max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3), 1e-12)
            nu = 2.0
            if dcost <= ftol * cost_new:
                status, stop = "ftol", True
        else:
            lam = min(lam * nu, 1e12)
            nu *= 2.0
        if not stop and step <= xtol * (xtol + xnorm):
            status, stop = "xtol", True
        if stop:
            break
    res = red.res(cams, pts)
    return dict(cams=cams, pts=pts, iterations=it, accepted=acc, sse0=sse0, sse=float((res * res).sum()), cost0=cost0,
                cost=cost, pcg_iters=0, status=status, history=hist, lam=lam, gmax=gmax)


def first_step_by_elimination(problem, cam_mask, pt_held, loss, f_scale, lam):
    """step_by_elimination at the problem's start."""
    red = _reduced(problem, cam_mask, pt_held)
    return step_by_elimination(red, red.cams, red.pts, loss, f_scale, lam)


def step_by_elimination(red, cams, pts, loss, f_scale, lam):
    """The damped step a second way, as the device forms it: block normal equations, the dense Schur complement with
    identity rows where held (Reduced.normal_equations, Reduced.schur), back substitution.  -> the step over the free
    entries, in Reduced.x's order."""
    ne = red.normal_equations(cams, pts, loss, f_scale)
    S, rhs = red.schur(ne, lam)
    dc = np.linalg.solve(S, rhs).reshape(-1, 6)
    dc[red.held_cam] = 0.0
    Hpp = ne["Hpp"].copy()
    i3 = np.arange(3)
    Hpp[:, i3, i3] += lam * np.maximum(Hpp[:, i3, i3], DIAG_FLOOR)
    Wt_dc = np.zeros((red.pts.shape[0], 3))
    np.add.at(Wt_dc, red.pi, np.einsum('nij,ni->nj', ne["W"], dc[red.ci]))
    dp = -np.linalg.solve(Hpp, (ne["bp"] + Wt_dc)[:, :, None])[:, :, 0]
    dp[red.held_pt] = 0.0
    return np.concatenate([dc.ravel(), dp.ravel()])[red.free]
