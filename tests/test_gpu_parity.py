"""GPU parity tests (run with -m gpu on an MI355X).  Everything goes through the C ABI
(ctypes -> libba_hip.so) and is compared with the CPU oracle on the same inputs, with the
golden fixtures captured from the imported reference, and -- at BASELINE.json's full
sizes -- through size-independent properties.

Tolerances (fp64 throughout): residuals 1e-9 px absolute; normal-equation blocks, Schur
products 1e-9 relative to the largest entry; converged cost 1e-9 relative; final
reprojection RMSE within 1e-6 px of the scipy path (north star)."""
import numpy as np
import pytest

from bundle_adjustment_amd import hip_backend
from bundle_adjustment_amd.synthetic import make_bal_like, make_config, make_problem
from oracle import ba_oracle as o
from tests.helpers import golden_flat_problem, load_golden
from tests.lm_trace import check_self_consistent

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def solver():
    s = hip_backend.Solver(0)
    yield s
    s.close()


def _rel(a, b):
    return float(np.abs(a - b).max() / max(1e-300, np.abs(b).max()))


# ---------------------------------------------------------------- K1 residuals
@pytest.mark.parametrize("name", ["cost_seed0", "cost_seed1", "cost_seed2", "cost_edge"])
def test_residuals_match_reference_goldens(solver, name):
    """Device residual vector == the imported reference's _cost_function output (rows in
    the reference's order), incl. theta = 0, theta ~ pi, a point behind the camera, a
    duplicated (kf, mp) observation and a point seen only by the fixed keyframe."""
    g = load_golden(name)
    for xk, fk in (("x0", "f0"), ("x1", "f1")):
        p = golden_flat_problem(g, g[xk])
        solver.set_problem(p)
        r, sse, cost = solver.residuals("linear")
        scale = max(1.0, np.abs(g[fk]).max())
        assert np.abs(r.ravel() - g[fk]).max() <= 1e-9 * scale
        assert abs(sse - float((g[fk] ** 2).sum())) <= 1e-9 * sse
        r2, _, cost_h = solver.residuals("huber")
        assert np.array_equal(r, r2)
        assert abs(cost_h - o.robust_cost(g[fk], "huber")) <= 1e-10 * max(1.0, cost_h)


@pytest.mark.parametrize("cfg,seed", [("C1", 0), ("C2", 0), ("C2", 1)])
def test_residuals_match_oracle_synthetic(solver, cfg, seed):
    p = make_config(cfg, seed=seed)
    solver.set_problem(p)
    r, sse, cost = solver.residuals("huber", f_scale=1.0)
    ref = o.residuals(p.cams, p.pts, p.cam_idx, p.pt_idx, p.uv, p.K4)
    assert np.abs(r - ref).max() <= 1e-9
    assert abs(cost - o.robust_cost(ref, "huber")) <= 1e-11 * cost


@pytest.mark.parametrize("small_solver", [0, 1], ids=["single_launch", "multi_kernel"])
def test_empty_and_ragged_inputs(solver, small_solver):
    """A camera without observations, a point seen once, zero observations overall -- through both implementations behind
    ba_solve (a window this small is dispatched to the single-launch solver unless small_solver = 1)."""
    p = make_problem(5, 40, 3, seed=3)
    keep = p.cam_idx != 2                       # camera 2 loses every observation
    keep[np.nonzero(p.pt_idx == 7)[0][1:]] = False   # point 7 keeps a single view
    q = type(p)(p.cams, p.pts, p.cam_idx[keep], p.pt_idx[keep], p.uv[keep], p.K4, 0)
    solver.set_problem(q)
    r, _, _ = solver.residuals()
    ref = o.residuals(q.cams, q.pts, q.cam_idx, q.pt_idx, q.uv, q.K4)
    assert np.abs(r - ref).max() <= 1e-9
    Hcc, bc, Hpp, bp = solver.linearize()
    assert np.all(Hcc[2] == 0) and np.all(bc[2] == 0)
    out = solver.solve(loss="linear", max_iters=10, small_solver=small_solver)
    assert (out["pcg_iterations"] > 0) == bool(small_solver)
    assert np.isfinite(out["final_cost"]) and out["final_cost"] <= out["initial_cost"]
    e = type(p)(p.cams, p.pts, p.cam_idx[:0], p.pt_idx[:0], p.uv[:0], p.K4, 0)
    solver.set_problem(e)
    r, sse, cost = solver.residuals()
    assert r.shape == (0, 2) and sse == 0.0 and cost == 0.0


def test_bad_arguments_are_rejected(solver):
    p = make_problem(4, 20, 2, seed=0)
    bad = type(p)(p.cams, p.pts, p.cam_idx.copy(), p.pt_idx.copy(), p.uv, p.K4, 0)
    bad.cam_idx[3] = 99
    with pytest.raises(ValueError):
        solver.set_problem(bad)
    lib = hip_backend.load_library()
    import ctypes as C
    rc = lib.ba_set_problem(solver._h, 4, 20, 5, bad.cam_idx.ctypes.data_as(C.POINTER(C.c_int32)),
                            bad.pt_idx.ctypes.data_as(C.POINTER(C.c_int32)),
                            bad.uv.ctypes.data_as(C.POINTER(C.c_double)), bad.K4.ctypes.data_as(C.POINTER(C.c_double)), 0)
    assert rc == -1 and b"out of range" in lib.ba_last_error()


# ---------------------------------------------------------------- K2/K3 normal equations
@pytest.mark.parametrize("loss", ["linear", "huber"])
@pytest.mark.parametrize("src", ["cost_edge", "cost_seed0", "C2"])
def test_normal_equations_match_oracle(solver, src, loss):
    p = make_config("C2", seed=0) if src == "C2" else golden_flat_problem(load_golden(src))
    if src == "cost_edge":           # the point behind the camera makes J huge; keep, tolerance is relative
        pass
    solver.set_problem(p)
    Hcc, bc, Hpp, bp = solver.linearize(loss)
    ne = o.normal_equations(p.cams, p.pts, p.cam_idx, p.pt_idx, p.uv, p.K4, 0, loss)
    assert _rel(Hcc, o.sym6_pack(ne["Hcc"])) <= 1e-9
    assert _rel(bc, ne["bc"]) <= 1e-9
    assert _rel(Hpp, o.sym3_pack(ne["Hpp"])) <= 1e-9
    assert _rel(bp, ne["bp"]) <= 1e-9


def test_normal_equations_equal_scipy_jtj(solver):
    """Hcc/Hpp/bc/bp are J^T J, J^T r of the sparse Jacobian scipy would hold (CSR built
    from the analytic blocks, themselves checked against finite differences on CPU)."""
    p = golden_flat_problem(load_golden("cost_seed1"))
    solver.set_problem(p)
    Hcc, bc, Hpp, bp = solver.linearize("linear")
    x0, adj = o.pack_reference_params(p.cams, p.pts, 0)
    J = o.flat_jacobian_fun(p.cams, p.n_pts, p.cam_idx, p.pt_idx, p.K4, 0)(x0)
    r = o.residuals(p.cams, p.pts, p.cam_idx, p.pt_idx, p.uv, p.K4).ravel()
    JtJ = (J.T @ J).toarray()
    Jtr = J.T @ r
    na = len(adj)
    for i, c in enumerate(adj):
        idx = np.r_[3 * i:3 * i + 3, 3 * na + 3 * i:3 * na + 3 * i + 3]
        blk = JtJ[np.ix_(idx, idx)]
        assert _rel(Hcc[c], blk[np.triu_indices(6)]) <= 1e-9
        assert _rel(bc[c], Jtr[idx]) <= 1e-9
    for j in range(0, p.n_pts, 17):
        idx = np.arange(6 * na + 3 * j, 6 * na + 3 * j + 3)
        assert _rel(Hpp[j], JtJ[np.ix_(idx, idx)][np.triu_indices(3)]) <= 1e-9
        assert _rel(bp[j], Jtr[idx]) <= 1e-9


# ---------------------------------------------------------------- K4 Schur products
@pytest.mark.parametrize("loss", ["linear", "huber"])
def test_schur_rhs_and_apply_match_dense(solver, loss):
    p = golden_flat_problem(load_golden("cost_seed2"))
    solver.set_problem(p)
    solver.linearize(loss)
    lam = 1e-3
    ne = o.normal_equations(p.cams, p.pts, p.cam_idx, p.pt_idx, p.uv, p.K4, 0, loss)
    S, rhs, _, _ = o.schur_dense(ne, p.cam_idx, p.pt_idx, lam, 0)
    g = solver.schur_rhs(lam)
    assert _rel(g.ravel(), rhs) <= 1e-9
    rng = np.random.default_rng(0)
    for _ in range(3):
        v = rng.normal(size=(p.n_cams, 6))
        out = solver.schur_apply(lam, v)
        assert _rel(out.ravel(), S @ v.ravel()) <= 1e-9
    # symmetry of the device operator
    a, b = rng.normal(size=(p.n_cams, 6)), rng.normal(size=(p.n_cams, 6))
    a[0] = b[0] = 0
    assert abs((solver.schur_apply(lam, a) * b).sum() - (solver.schur_apply(lam, b) * a).sum()) <= 1e-9 * abs(
        (solver.schur_apply(lam, a) * b).sum())


# ---------------------------------------------------------------- K2-K7 solve
@pytest.mark.parametrize("small_solver", [0, 1], ids=["single_launch", "multi_kernel"])
@pytest.mark.parametrize("name,loss", [("conv_linear", "linear"), ("conv_huber", "huber")])
def test_converged_rmse_matches_scipy_path(solver, name, loss, small_solver):
    """North-star bar: final reprojection RMSE within 1e-6 px of the reference's
    scipy.optimize.least_squares path driven to convergence on the same inputs."""
    g = load_golden(name)
    p = golden_flat_problem(g)
    solver.set_problem(p)
    out = solver.solve(loss=loss, max_iters=300, ftol=1e-15, xtol=1e-15, gtol=0.0, pcg_tol=1e-3, pcg_max_iters=300,
                       small_solver=small_solver)
    assert (out["pcg_iterations"] > 0) == bool(small_solver)
    rmse = np.sqrt(out["final_sse"] / p.n_obs)
    rmse_ref = np.sqrt(float((g["res_fun"] ** 2).sum()) / p.n_obs)
    assert abs(rmse - rmse_ref) <= 1e-6
    assert abs(out["final_cost"] - float(g["res_cost"])) <= 1e-8 * float(g["res_cost"])


@pytest.mark.parametrize("loss,precond", [("linear", "schur_jacobi"), ("huber", "schur_jacobi"), ("linear", "jacobi")])
def test_solve_matches_cpu_mirror(solver, loss, precond):
    p = make_problem(12, 800, 5, seed=4, outlier_frac=0.02 if loss == "huber" else 0.0)
    solver.set_problem(p)
    kw = dict(max_iters=40, ftol=1e-13, xtol=1e-13, gtol=0.0, pcg_tol=1e-4, pcg_max_iters=400)
    out = solver.solve(loss=loss, preconditioner=precond, **kw)
    check_self_consistent(out, solver.trace(), kw)
    ref = o.lm_solve(p.cams, p.pts, p.cam_idx, p.pt_idx, p.uv, p.K4, 0, loss, precond=precond, **kw)
    assert abs(out["final_cost"] - ref["cost"]) <= 1e-9 * ref["cost"]
    cams, pts = solver.get_params()
    assert np.abs(cams - ref["cams"]).max() <= 1e-6
    assert np.abs(pts - ref["pts"]).max() <= 1e-5
    # the device's own final state is self-consistent
    r, sse, cost = solver.residuals(loss)
    assert abs(sse - out["final_sse"]) <= 1e-9 * sse and abs(cost - out["final_cost"]) <= 1e-9 * cost
    np.testing.assert_allclose(solver.get_rotations(), o.rodrigues_batch(cams[:, :3]), atol=1e-14)


@pytest.mark.parametrize("loss", ["linear", "huber"])
def test_kept_preconditioner_blocks_follow_the_oracle_and_reach_the_same_minimiser(loss):
    """ba_options.precond_lag: near convergence (steps that lower the cost by less than 1 %) up to `lag` consecutive damped
    systems keep the Schur-Jacobi blocks built for an earlier one (right-hand side from the 6-sum camera pass, no
    inversions).  The oracle's LM mirror applies the same rule: with a tight PCG tolerance the device follows it step by
    step -- same PCG iteration counts (within one: the kept systems' right-hand side comes out of another kernel, i.e.
    another summation order), same verdicts, same minimiser -- and the counters say how often blocks were built / kept.
    precond_lag = 0 never keeps anything and lands on the same minimiser."""
    p = make_problem(12, 800, 5, seed=4, outlier_frac=0.02 if loss == "huber" else 0.0)
    kw = dict(max_iters=25, ftol=0.0, xtol=0.0, gtol=0.0, pcg_tol=1e-4, pcg_max_iters=400)
    res = {}
    with hip_backend.Solver(0) as s:
        for lag in (3, 0):
            s.set_problem(p)
            st0 = s.stats()
            out = s.solve(loss=loss, precond_lag=lag, **kw)
            st1 = s.stats()
            res[lag] = (out, s.trace(), s.get_params(), {k: st1[k] - st0[k] for k in st1})
            check_self_consistent(out, res[lag][1], kw)
    out, tr, (cams, pts), st = res[3]
    ref = o.lm_solve(p.cams, p.pts, p.cam_idx, p.pt_idx, p.uv, p.K4, 0, loss, precond_lag=3, **kw)
    assert st["precond_reuses"] >= 5 and st["precond_builds"] + st["precond_reuses"] == out["iterations"] == 25
    assert res[0][3]["precond_reuses"] == 0 and res[0][3]["precond_builds"] == 25
    compared = 0
    for t, h in zip(tr, ref["history"]):
        if abs(h["cost"] - h["cost_new"]) <= 1e-11 * h["cost"]:
            break                          # at the minimiser: accept / reject is decided by round-off from here on
        assert abs(t["pcg_iterations"] - h["pcg"]) <= 1, (t, h)
        assert abs(t["cost_trial"] - h["cost_new"]) <= 1e-9 * h["cost_new"], (t, h)
        assert bool(t["accepted"]) == bool(h["rho"] > 0)
        compared += 1
    assert compared >= 6
    assert abs(out["final_cost"] - ref["cost"]) <= 1e-9 * ref["cost"]
    assert abs(out["final_cost"] - res[0][0]["final_cost"]) <= 1e-9 * ref["cost"]


def test_reference_default_settings_never_worse_than_reference(solver):
    """At the reference's literals (huber, xtol = ftol = 1e-5, 50 evaluations) the final SSE
    must not exceed what the reference's own run() reached (golden run_seed0)."""
    from bundle_adjustment_amd.problem import flatten_window, gather_window
    from tests.helpers import rebuild_map
    for name in ("run_seed0", "run_seed1", "run_global"):
        g = load_golden(name)
        gmap = rebuild_map(g)
        w = int(g["window_size"])
        local = sorted(gmap.keyframes)[-(w + 1):-1]
        mp_ids, obs, kp = gather_window(gmap, local)
        p = flatten_window(gmap, local, mp_ids, obs, kp, g["K"])
        ref_sse = float((g["res_fun"] ** 2).sum())
        for small_solver in (0, 1):                      # both implementations behind ba_solve
            solver.set_problem(p)
            out = solver.solve(small_solver=small_solver)
            assert out["final_sse"] <= ref_sse * (1 + 1e-9)


def test_c2_solve_and_properties(solver):
    p = make_config("C2", seed=0)
    solver.set_problem(p)
    out = solver.solve(loss="linear", max_iters=30, ftol=1e-10, xtol=1e-12, gtol=0.0)
    rmse = np.sqrt(out["final_sse"] / p.n_obs)
    # 30 iterations at ftol 1e-10 already sit on the scipy path's converged value (the 1e-6 px pin with tight
    # tolerances is tests/test_gpu_converged.py)
    assert abs(rmse - float(load_golden("conv_c2_linear")["res_rmse"])) <= 1e-5 and out["final_sse"] < out["initial_sse"]
    cams1, pts1 = solver.get_params()
    # determinism: same inputs -> bitwise same outputs
    solver.set_problem(p)
    out2 = solver.solve(loss="linear", max_iters=30, ftol=1e-10, xtol=1e-12, gtol=0.0)
    cams2, pts2 = solver.get_params()
    assert out2["final_cost"] == out["final_cost"] and np.array_equal(cams1, cams2) and np.array_equal(pts1, pts2)
    # invariance to the caller's observation order
    perm = np.random.default_rng(0).permutation(p.n_obs)
    q = type(p)(p.cams, p.pts, p.cam_idx[perm], p.pt_idx[perm], p.uv[perm], p.K4, 0)
    solver.set_problem(q)
    r, _, _ = solver.residuals()
    solver.set_problem(p)
    r0, _, _ = solver.residuals()
    assert np.array_equal(r, r0[perm])


def test_headline_size_properties(solver):
    """C3 (1000 cams / 100k points / 1M observations): residual parity with the
    vectorised oracle at full size, cost decrease, and convergence to the noise floor."""
    p = make_config("C3", seed=0)
    solver.set_problem(p)
    r, sse, cost = solver.residuals("huber")
    ref = o.residuals(p.cams, p.pts, p.cam_idx, p.pt_idx, p.uv, p.K4)
    assert np.abs(r - ref).max() <= 1e-9
    assert abs(sse - float((ref * ref).sum())) <= 1e-10 * sse
    out = solver.solve(loss="huber", max_iters=25, ftol=1e-8, xtol=1e-10, gtol=0.0)
    assert out["final_cost"] < out["initial_cost"]
    rmse = np.sqrt(out["final_sse"] / p.n_obs)
    # Huber minimiser at C3: plain-SSE RMSE a little above the linear-loss minimum the scipy path converges to
    # (golden conv_c3_linear, 0.651152 px); the 1e-6 px pins are in tests/test_gpu_converged.py
    lin = float(load_golden("conv_c3_linear")["res_rmse"])
    assert lin <= rmse <= lin + 1e-3, (rmse, lin)
    r2, sse2, _ = solver.residuals("huber")
    assert abs(sse2 - out["final_sse"]) <= 1e-9 * sse2


def test_bal_like_topology(solver):
    p = make_bal_like(n_cams=300, n_pts=20000, n_obs_target=90000, seed=1)
    solver.set_problem(p)
    r, sse, _ = solver.residuals()
    ref = o.residuals(p.cams, p.pts, p.cam_idx, p.pt_idx, p.uv, p.K4)
    assert np.abs(r - ref).max() <= 1e-9
    out = solver.solve(loss="huber", max_iters=30, ftol=1e-8, xtol=1e-12, gtol=0.0)
    assert out["final_cost"] < 0.05 * out["initial_cost"]


def test_c5_full_size_l2_fallback(solver):
    """BASELINE config 5 topology at full size (1723 cams / 156 502 pts / ~662k obs): more cameras
    than the LDS camera table holds, so the point passes take the L2-gather path."""
    p = make_bal_like(seed=0)
    assert p.n_cams == 1723 and p.n_pts == 156502
    solver.set_problem(p)
    r, sse, _ = solver.residuals()
    ref = o.residuals(p.cams, p.pts, p.cam_idx, p.pt_idx, p.uv, p.K4)
    assert np.abs(r - ref).max() <= 1e-9
    Hcc, bc, Hpp, bp = solver.linearize("huber")
    sel = np.arange(0, p.n_obs, 1)            # oracle blocks on the full list (vectorised)
    ne = o.normal_equations(p.cams, p.pts, p.cam_idx, p.pt_idx, p.uv, p.K4, 0, "huber")
    assert _rel(Hcc, o.sym6_pack(ne["Hcc"])) <= 1e-9 and _rel(bp, ne["bp"]) <= 1e-9
    out = solver.solve(loss="huber", max_iters=30, ftol=1e-9, xtol=1e-12, gtol=0.0)
    assert out["final_cost"] < 0.05 * out["initial_cost"]
    assert np.sqrt(out["final_sse"] / p.n_obs) < 0.75


def test_c5_full_size_fp32_jacobian_mode(solver):
    """BASELINE config 5 AS SPECIFIED on one GPU: the full-size BAL-like problem (1723 cams / 156 502 pts) in its
    precision mode -- fp32 Jacobian blocks in the PCG passes, fp64 accumulation and solve.  The quasi-Newton operator is
    the only thing fp32 touches, so the descent must follow the fp64 run: same accepted steps, costs equal to fp32
    operator accuracy, and the residual vector of the result (fp64 kernel) must agree with the oracle."""
    p = make_bal_like(seed=0)
    kw = dict(loss="huber", max_iters=10, ftol=1e-9, xtol=1e-12, gtol=0.0, pcg_tol=0.1, pcg_max_iters=400)
    solver.set_problem(p)
    ref = solver.solve(**kw)
    solver.set_problem(p)
    out = solver.solve(jacobian_precision=1, **kw)
    cams, pts = solver.get_params()
    assert out["accepted"] == out["iterations"] and ref["accepted"] == ref["iterations"]
    assert out["final_cost"] < 0.05 * out["initial_cost"]
    assert abs(out["final_cost"] - ref["final_cost"]) <= 2e-3 * ref["final_cost"], (out["final_cost"], ref["final_cost"])
    assert np.sqrt(out["final_sse"] / p.n_obs) < 0.75
    r, sse, _ = solver.residuals("huber")
    assert np.abs(r - o.residuals(cams, pts, p.cam_idx, p.pt_idx, p.uv, p.K4)).max() <= 1e-9
    assert abs(sse - out["final_sse"]) <= 1e-9 * sse


def test_fp32_jacobian_mode_reaches_the_fp64_solution(solver):
    """BASELINE config 5's precision mode: Jacobian blocks of the PCG passes in fp32, every sum,
    the gradient, the cost and the update in fp64.  Only the quasi-Newton operator changes, so the
    converged solution is the fp64 one."""
    p = make_problem(15, 1200, 5, seed=9, outlier_frac=0.02)
    kw = dict(loss="huber", max_iters=40, ftol=1e-13, xtol=1e-13, gtol=0.0, pcg_tol=1e-3)
    solver.set_problem(p)
    ref = solver.solve(**kw)
    cams_ref, pts_ref = solver.get_params()
    solver.set_problem(p)
    out = solver.solve(jacobian_precision=1, **kw)
    cams, pts = solver.get_params()
    assert abs(out["final_cost"] - ref["final_cost"]) <= 1e-9 * ref["final_cost"]
    assert np.abs(cams - cams_ref).max() <= 1e-6 and np.abs(pts - pts_ref).max() <= 1e-5
    with pytest.raises(hip_backend.BAHipError):
        solver.solve(jacobian_precision=2, **kw)


def test_multi_round_point_ranges(solver, monkeypatch):
    """Large problems give every point-pass workgroup a range of several rounds (one table fill per
    workgroup, ba_set_problem).  Force that split on a small problem and check every point-pass
    product against the default one-round split: per-point outputs bit-identical, sums over
    workgroups to rounding, the solve to 1e-10."""
    p = make_problem(40, 6000, 6, seed=4, outlier_frac=0.01)
    v = np.random.default_rng(0).normal(size=(p.n_cams, 6))
    kw = dict(loss="huber", max_iters=15, ftol=1e-12, xtol=1e-12, gtol=0.0, pcg_tol=1e-2)

    def products():
        solver.set_problem(p)
        Hcc, bc, Hpp, bp = solver.linearize("huber")
        g = solver.schur_rhs(1e-3)
        Sv = solver.schur_apply(1e-3, v)
        out = solver.solve(**kw)
        return Hcc, bc, Hpp, bp, g, Sv, out, solver.get_params()

    ref = products()
    monkeypatch.setenv("BA_PT_BLOCKS", "3")              # 6000 points / 3 workgroups = 4 rounds of 512 each
    got = products()
    monkeypatch.delenv("BA_PT_BLOCKS")
    for a, b in zip(ref[:4], got[:4]):
        np.testing.assert_array_equal(a, b)
    assert _rel(got[4], ref[4]) <= 1e-12 and _rel(got[5], ref[5]) <= 1e-12
    assert abs(got[6]["final_cost"] - ref[6]["final_cost"]) <= 1e-10 * ref[6]["final_cost"]
    assert np.abs(got[7][0] - ref[7][0]).max() <= 1e-8 and np.abs(got[7][1] - ref[7][1]).max() <= 1e-7


@pytest.mark.parametrize("lanes", [2, 4, 8, 16])
def test_lanes_per_point_variants(solver, monkeypatch, lanes):
    """ba_set_problem picks 2, 4, 8 or 16 lanes per point from the problem size; every choice must give
    the same per-point blocks (to the rounding of the re-grouped sums) and the same solve."""
    p = make_problem(30, 4000, 7, seed=6, outlier_frac=0.01)
    v = np.random.default_rng(1).normal(size=(p.n_cams, 6))
    kw = dict(loss="huber", max_iters=12, ftol=1e-12, xtol=1e-12, gtol=0.0, pcg_tol=1e-2)
    ne = o.normal_equations(p.cams, p.pts, p.cam_idx, p.pt_idx, p.uv, p.K4, 0, "huber")
    monkeypatch.setenv("BA_PT_LANES", str(lanes))
    solver.set_problem(p)
    Hcc, bc, Hpp, bp = solver.linearize("huber")
    assert _rel(Hpp, o.sym3_pack(ne["Hpp"])) <= 1e-9 and _rel(bp, ne["bp"]) <= 1e-9
    op = o.SchurOperator(ne, p.cam_idx, p.pt_idx, 1e-3, 0)
    assert _rel(solver.schur_rhs(1e-3), op.rhs()) <= 1e-9
    vv = v.copy(); vv[0] = 0
    assert _rel(solver.schur_apply(1e-3, vv), op.apply(vv)) <= 1e-9
    out = solver.solve(**kw)
    ref = o.lm_solve(p.cams, p.pts, p.cam_idx, p.pt_idx, p.uv, p.K4, 0, "huber", max_iters=12, ftol=1e-12, xtol=1e-12,
                     gtol=0.0, pcg_tol=1e-2)
    assert abs(out["final_cost"] - ref["cost"]) <= 1e-8 * ref["cost"]


def test_pcg_model_test_follows_the_oracle(solver):
    """ba_options.pcg_model_tol (Nash & Sofer's truncated-Newton test on the quadratic model, opt-in): on a chain problem at
    small damping the PCG loop is ended by the model test well before the residual test or the iteration cap; the device
    and the oracle's mirror stop at the same iteration counts and walk the same LM trajectory."""
    p = make_bal_like(n_cams=120, n_pts=9000, n_obs_target=40000, seed=3)
    kw = dict(max_iters=7, ftol=0.0, xtol=0.0, gtol=0.0, pcg_tol=1e-3, pcg_max_iters=400)
    ref = o.lm_solve(p.cams, p.pts, p.cam_idx, p.pt_idx, p.uv, p.K4, fixed_cam=0, loss="huber", lam0=1e-7, pcg_model_tol=0.5, **kw)
    full = o.lm_solve(p.cams, p.pts, p.cam_idx, p.pt_idx, p.uv, p.K4, fixed_cam=0, loss="huber", lam0=1e-7, pcg_model_tol=0.0, **kw)
    assert ref["pcg_iters"] < 0.6 * full["pcg_iters"]                   # the test does cut the inner solves short
    solver.set_problem(p)
    out = solver.solve(loss="huber", initial_lambda=1e-7, pcg_model_tol=0.5, pcg_min_iters=0, **kw)
    tr = solver.trace()
    check_self_consistent(out, tr, dict(kw, initial_lambda=1e-7))
    assert out["iterations"] == len(ref["history"])
    for t, h in zip(tr, ref["history"]):
        assert abs(t["pcg_iterations"] - h["pcg"]) <= max(1, 0.1 * h["pcg"]), (t, h)
        assert abs(t["cost_trial"] - h["cost_new"]) <= 1e-6 * h["cost_new"], (t, h)
    assert abs(out["final_cost"] - ref["cost"]) <= 1e-6 * ref["cost"]


def test_camera_windows_that_do_not_fit_in_lds_follow_the_oracle(solver):
    """1200 cameras with uniformly random visibility: the camera table (1200 x 144 bytes) exceeds the LDS budget and no
    workgroup's camera window is narrow, so the point passes gather camera rows from L2 (ALL_LDS = false instantiations)
    and the camera update runs as a launch of its own instead of riding along the back substitution.  Same LM trajectory
    as the oracle, residuals <= 1e-9 px."""
    p = make_problem(1200, 6000, 6, seed=31, outlier_frac=0.01)
    solver.set_problem(p)
    r, sse, _ = solver.residuals("huber")
    assert np.abs(r - o.residuals(p.cams, p.pts, p.cam_idx, p.pt_idx, p.uv, p.K4)).max() <= 1e-9
    kw = dict(max_iters=5, ftol=0.0, xtol=0.0, gtol=0.0, pcg_tol=1e-2, pcg_max_iters=300)
    ref = o.lm_solve(p.cams, p.pts, p.cam_idx, p.pt_idx, p.uv, p.K4, fixed_cam=0, loss="huber", **kw)
    out = solver.solve(loss="huber", pcg_min_iters=0, **kw)
    tr = solver.trace()
    check_self_consistent(out, tr, kw)
    assert out["iterations"] == len(ref["history"]) == 5
    for t, h in zip(tr, ref["history"]):
        assert abs(t["pcg_iterations"] - h["pcg"]) <= max(1, 0.1 * h["pcg"]), (t, h)
        assert abs(t["cost_trial"] - h["cost_new"]) <= 1e-7 * h["cost_new"], (t, h)
        assert bool(t["accepted"]) == bool(h["rho"] > 0)
    assert abs(out["final_cost"] - ref["cost"]) <= 1e-7 * ref["cost"]


@pytest.mark.parametrize("long_slots", [None, "3"])
def test_chain_with_long_tracks_and_camera_windows_follows_the_oracle(monkeypatch, long_slots):
    """A 1300-camera chain with BAL-like track lengths (median 3, up to ~80): the camera table exceeds LDS, every workgroup
    stages its own window of cameras, tracks longer than 8 observations run as 16-lane rows behind the 2-lane ranges in the
    same launch.  long_slots = 3: the long-track workgroups walk three rounds of 64 points each (BA_LONG_SLOTS; what
    ba_set_problem chooses by itself when one-round workgroups would not all be resident, config 5).  Same LM trajectory
    as the oracle either way, and the two grids agree to rounding."""
    from bundle_adjustment_amd import hip_backend
    from bundle_adjustment_amd.synthetic import make_bal_like
    if long_slots is not None:
        monkeypatch.setenv("BA_LONG_SLOTS", long_slots)
    p = make_bal_like(1300, 9000, 40000, seed=5)
    # (three LM iterations: from the fourth on the chain's inner solves take ~100 PCG iterations, over which two
    # implementations' rounding separates the iterates by more than a trajectory comparison tolerates)
    kw = dict(max_iters=3, ftol=0.0, xtol=0.0, gtol=0.0, pcg_tol=1e-2, pcg_max_iters=300)
    ref = o.lm_solve(p.cams, p.pts, p.cam_idx, p.pt_idx, p.uv, p.K4, fixed_cam=0, loss="huber", **kw)
    with hip_backend.Solver(0) as s:
        s.set_problem(p)
        r, sse, _ = s.residuals("huber")
        assert np.abs(r - o.residuals(p.cams, p.pts, p.cam_idx, p.pt_idx, p.uv, p.K4)).max() <= 1e-9
        out = s.solve(loss="huber", pcg_min_iters=0, **kw)
        tr = s.trace()
    check_self_consistent(out, tr, kw)
    assert out["iterations"] == len(ref["history"]) == 3
    for t, h in zip(tr, ref["history"]):
        assert abs(t["pcg_iterations"] - h["pcg"]) <= max(1, 0.1 * h["pcg"]), (t, h)
        assert abs(t["cost_trial"] - h["cost_new"]) <= 1e-6 * h["cost_new"], (t, h)
        assert bool(t["accepted"]) == bool(h["rho"] > 0)
    assert abs(out["final_cost"] - ref["cost"]) <= 1e-6 * ref["cost"]

