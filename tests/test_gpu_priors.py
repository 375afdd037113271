"""GPU: Gaussian priors (ba_set_priors) through every layer -- the linearisation and reduced-system hooks against
tests/prior_reference.py, the no-op rule, one LM step against the dense step, solves certified on the TOTAL objective
(both values of small_solver, Huber, BAL intrinsics), the scaling with sigma, covariances on a gauge the priors fix, two
ranks, and the error rules."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from bundle_adjustment_amd import bal, hip_backend
from bundle_adjustment_amd.problem import BAProblem
from bundle_adjustment_amd.synthetic import make_bal_problem, make_problem
from tests import robust_losses as rl
from tests.held_reference import Reduced
from tests.prior_reference import PriorProblem, prior_covariance, rotated_info, standard_input
from tests.test_gpu_covariance import check_covariance

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIGHT = dict(ftol=0.0, xtol=0.0, gtol=0.0)


def _rel(a, b):
    return float(np.abs(a - b).max() / max(1e-300, np.abs(b).max()))


@pytest.fixture(scope="module")
def solver():
    s = hip_backend.Solver(0)
    yield s
    s.close()


def _reference(p, cp, pp, cam_mask=None, pt_held=None, K4="pinhole"):
    red = Reduced(p.cams, p.pts, p.cam_idx, p.pt_idx, p.uv, p.K4 if K4 == "pinhole" else None, p.fixed_cam if K4 == "pinhole" else -1,
                  cam_mask, pt_held)
    return PriorProblem(red, cp, pp)


# ---------------------------------------------------------------- 1. linearisation and the reduced system
@pytest.mark.parametrize("loss", ["linear", "huber"])
def test_linearize_adds_the_priors_ahead_of_the_held_zeroing(solver, loss):
    p, cp, pp = standard_input(outlier_frac=0.02)
    rng = np.random.default_rng(1)
    cm = (rng.integers(0, 64, size=p.n_cams) * (rng.random(p.n_cams) < 0.3)).astype(np.uint16)
    cm[p.n_cams - 1] |= 1 << 4                         # a held coordinate under camera 11's prior on t
    cm[0] |= 1 << 1                                    # ... and one under camera 0's full block
    pm = rng.random(p.n_pts) < 0.1
    pm[np.nonzero(pp[1].reshape(p.n_pts, -1).any(axis=1))[0][:3]] = True     # held points that carry a prior
    solver.set_problem(p)
    solver.set_priors(cp, pp)
    solver.set_held(cm, pm)
    Hcc, bc, Hpp, bp = solver.linearize(loss, f_scale=2.0)
    pr = _reference(p, cp, pp, cm, pm)
    ne = pr.normal_equations(p.cams, p.pts, loss, 2.0)
    plain = pr.red.normal_equations(p.cams, p.pts, loss, 2.0)
    assert _rel(ne["Hcc"], plain["Hcc"]) > 1e-6 and _rel(ne["bp"], plain["bp"]) > 1e-6      # (the priors are not negligible)
    assert _rel(Hcc, rl.pack_upper(ne["Hcc"])) <= 1e-12 and _rel(bc, ne["bc"]) <= 1e-12
    assert _rel(Hpp, rl.pack_upper(ne["Hpp"])) <= 1e-12 and _rel(bp, ne["bp"]) <= 1e-12
    assert np.all(Hpp[pm] == 0) and np.all(bp[pm] == 0)
    held = pr.red.held_cam
    full = hip_backend.unpack_sym(Hcc, 6)
    assert np.all(bc[held] == 0) and np.all(full[held] == 0) and np.all(np.swapaxes(full, 1, 2)[held] == 0)
    lam = 1e-3
    S, rhs = pr.schur(ne, lam)
    g = solver.schur_rhs(lam).ravel()
    assert _rel(g, rhs) <= 1e-9 and np.all(g[held.ravel()] == 0)
    v = np.random.default_rng(0).normal(size=(p.n_cams, 6))
    assert _rel(solver.schur_apply(lam, v).ravel(), S @ v.ravel()) <= 1e-9
    assert solver.stats()["prior_blocks"] == 2 + p.n_pts // 20
    solver.set_held()
    solver.set_priors()


def test_bal_linearize_with_priors_on_the_intrinsics(solver):
    p = make_bal_problem(n_cams=16, n_pts=800, n_obs_target=3500, seed=2)
    rng = np.random.default_rng(5)
    nc = p.n_cams
    mean, info = np.zeros((nc, 9)), np.zeros((nc, 9, 9))
    for c in range(nc):                                     # f, k1, k2 of every camera; a full 9 x 9 block on two of them
        info[c, 6:, 6:] = rotated_info(rng, [18.0, 0.01, 0.003])
        mean[c, 6:] = p.cams[c, 6:] + rng.normal(size=3) * [18.0, 0.01, 0.003]
    for c in (3, 9):
        info[c] = rotated_info(rng, [1e-3] * 3 + [5e-3] * 3 + [18.0, 0.01, 0.003])
        mean[c] = p.cams[c] + rng.normal(size=9) * 1e-3
    cm = np.zeros(nc, np.uint16)
    cm[:4] |= 0x1C0
    intr = solver.set_problem_bal(p, fixed_cam=0)
    solver.set_priors(cams=(mean, info))
    solver.set_held(cm)
    out = dict(Hcc=np.empty((nc, 45)), bc=np.empty((nc, 9)), Hpp=np.empty((p.n_pts, 6)), bp=np.empty((p.n_pts, 3)))
    dp = hip_backend._dp
    hip_backend._check(solver._lib.ba_linearize_bal(solver._h, dp(intr), hip_backend.loss_code("huber"), 2.0, dp(out["Hcc"]),
                                                    dp(out["bc"]), dp(out["Hpp"]), dp(out["bp"])))
    red = Reduced(p.cams, p.pts, p.cam_idx, p.pt_idx, p.uv, None, 0, cm, None)
    pr = PriorProblem(red, (mean, info), None)
    ne = pr.normal_equations(p.cams, p.pts, "huber", 2.0)
    assert _rel(ne["Hcc"], red.normal_equations(p.cams, p.pts, "huber", 2.0)["Hcc"]) > 1e-9
    assert _rel(out["Hcc"], rl.pack_upper(ne["Hcc"])) <= 1e-12 and _rel(out["bc"], ne["bc"]) <= 1e-12
    assert _rel(out["Hpp"], rl.pack_upper(ne["Hpp"])) <= 1e-12 and _rel(out["bp"], ne["bp"]) <= 1e-12
    assert np.all(out["bc"][0] == 0) and np.all(out["Hcc"][0] == 0)                     # the fixed camera's block stays zero
    cc, pc = solver.prior_cost(intr)
    ref_c, ref_p = pr.prior_cost(p.cams, p.pts)
    assert abs(cc - ref_c) <= 1e-12 * ref_c and pc == 0.0 == ref_p


# ---------------------------------------------------------------- 2. no priors, no change
def test_cleared_and_all_zero_priors_leave_a_solve_bit_identical():
    p, cp, pp = standard_input()
    kw = dict(loss="huber", max_iters=12, small_solver=1)

    def run(prepare):
        with hip_backend.Solver(0) as s:
            s.set_problem(p)
            prepare(s)
            assert s.stats()["prior_blocks"] == 0
            out = s.solve(**kw)
            tr = [{k: v for k, v in r.items() if k != "seconds"} for r in s.trace()]
            return {k: v for k, v in out.items() if not k.startswith("seconds")}, tr, s.get_params()

    ref = run(lambda s: None)

    def set_then_clear(s):
        s.set_priors(cp, pp)
        assert s.stats()["prior_blocks"] == 2 + p.n_pts // 20
        s.set_priors()

    def all_zero(s):
        s.set_priors((np.full((p.n_cams, 6), np.nan), np.zeros((p.n_cams, 6, 6))), (np.zeros((p.n_pts, 3)), np.zeros((p.n_pts, 3, 3))))

    for prepare in (set_then_clear, all_zero):
        got = run(prepare)
        assert got[0] == ref[0] and got[1] == ref[1]
        assert np.array_equal(got[2][0], ref[2][0]) and np.array_equal(got[2][1], ref[2][1])


# ---------------------------------------------------------------- 3. one LM iteration against the dense step
def _one_step(p, pr, priors_on, lam):
    with hip_backend.Solver(0) as s:
        s.set_problem(p)
        if priors_on is not None:
            s.set_priors(*priors_on)
        out = s.solve(loss="linear", max_iters=1, initial_lambda=lam, pcg_tol=1e-12, pcg_max_iters=5000, small_solver=1, **TIGHT)
        assert out["iterations"] == 1 and out["accepted"] == 1 and 0 < out["pcg_iterations"] < 5000
        cams, pts = s.get_params()
        gain = s.trace()[0]["gain_ratio"]
    c1, p1, d, _, gain_ref = pr.dense_step(p.cams, p.pts, lam)
    step = np.concatenate([(cams - p.cams).ravel(), (pts - p.pts).ravel()])
    return _rel(step, d), abs(gain - gain_ref) / abs(gain_ref)


def test_one_lm_step_matches_the_dense_step():
    """Tolerance: the same comparison WITHOUT priors (behaviour the parent commit has) sets the scale; the prior case may be
    ten times worse -- the priors make this input's reduced system worse conditioned, not the arithmetic less exact.
    Measured on an MI355X: see DESIGN.md 4f."""
    p, cp, pp = standard_input()
    lam = 1e-3
    e0, g0 = _one_step(p, _reference(p, None, None), None, lam)
    e1, g1 = _one_step(p, _reference(p, cp, pp), (cp, pp), lam)
    print(f"one LM step, relative error of the step: no priors {e0:.3e}, priors {e1:.3e}; of the gain ratio: {g0:.3e}, {g1:.3e}")
    assert e1 <= 10.0 * e0
    # the gain ratio is one fp64 number, and both sides reach it through a rounded difference of costs, a rounded model sum
    # and a rounded quotient: below a few units of roundoff (16 u) the comparison says nothing, whatever the no-prior error is
    assert g1 <= max(10.0 * g0, 16.0 * 2.0 ** -53)


# ---------------------------------------------------------------- 4. solves to convergence, linear loss
@pytest.mark.parametrize("small", [1, 0])
def test_solve_is_a_minimiser_of_the_total_objective(solver, small):
    p, cp, pp = standard_input()
    pr = _reference(p, cp, pp)
    solver.set_problem(p)
    solver.set_priors(cp, pp)
    out = solver.solve(loss="linear", max_iters=100, pcg_tol=1e-6, small_solver=small, **TIGHT)
    assert out["status"] >= 0 and out["final_cost"] < out["initial_cost"] and out["pcg_iterations"] > 0
    cams, pts = solver.get_params()
    report = []
    pr.certify(p.cams, p.pts, cams, pts, "linear", report=report)
    print(f"small_solver {small}: gradient ratio {report[0][0]:.3e}, scipy restart drop {report[0][1]:.3e}")
    _, sse, cost = solver.residuals("linear", want_vector=False)
    cc, pc = solver.prior_cost()
    ref_c, ref_p = pr.prior_cost(cams, pts)
    assert abs(cc - ref_c) <= 1e-12 * ref_c and abs(pc - ref_p) <= 1e-12 * ref_p
    assert abs(out["final_cost"] - (cost + cc + pc)) <= 1e-12 * out["final_cost"]
    assert abs(out["final_sse"] - sse) <= 1e-12 * sse
    assert abs(out["initial_cost"] - pr.total_cost(p.cams, p.pts)) <= 1e-12 * out["initial_cost"]
    tr = solver.trace()
    assert tr[0]["cost"] == out["initial_cost"] and abs(2.0 * tr[-1]["cost_trial"] - tr[-1]["sse_trial"]) > 1e-6    # total against sse
    solver.set_priors()


def test_window_sized_problem_with_priors_takes_the_multi_kernel_path():
    """The routing: five cameras would go to the window solver; with priors set the multi-kernel path serves them."""
    p, cams_true, pts_true = make_problem(5, 600, 4, seed=13, return_truth=True)
    p = BAProblem(p.cams, p.pts, p.cam_idx, p.pt_idx, p.uv, p.K4, -1)
    rng = np.random.default_rng(2)
    cp = {0: (cams_true[0], rotated_info(rng, [1e-3] * 3 + [5e-3] * 3)), 4: (cams_true[4], np.diag([0, 0, 0, 1e4, 1e4, 1e4]))}
    pp = {int(j): (pts_true[j], rotated_info(rng, [0.02] * 3)) for j in range(0, p.n_pts, 25)}
    kw = dict(loss="linear", max_iters=60, pcg_tol=1e-6, small_solver=0, **TIGHT)
    with hip_backend.Solver(0) as s:
        s.set_problem(p)
        s.set_priors(cp, pp)
        before = s.stats()
        out = s.solve(**kw)
        after = s.stats()
        cams, pts = s.get_params()
        assert out["pcg_iterations"] > 0
        assert all(after[k] == before[k] for k in ("window_mw_launches", "window_lm_launches"))
        s.set_priors()                                          # cleared: the window solver serves the same handle again
        s.set_params(p.cams, p.pts)
        s.set_held(cams=np.arange(p.n_cams) == 0)
        plain = s.solve(**kw)
        assert plain["pcg_iterations"] == 0 and s.stats()["window_mw_launches"] + s.stats()["window_lm_launches"] == \
            after["window_mw_launches"] + after["window_lm_launches"] + 1
    from bundle_adjustment_amd.priors import pack_priors
    cm, cL = pack_priors(cp, p.n_cams, 6, "camera")
    pm, pL = pack_priors(pp, p.n_pts, 3, "point")
    pr = _reference(p, (cm, hip_backend.unpack_sym(cL, 6)), (pm, hip_backend.unpack_sym(pL, 3)))
    pr.certify(p.cams, p.pts, cams, pts, "linear")


# ---------------------------------------------------------------- 5. Huber
def test_huber_solve_meets_the_gradient_certificate(solver):
    p, cp, pp = standard_input(outlier_frac=0.02)
    pr = _reference(p, cp, pp)
    solver.set_problem(p)
    solver.set_priors(cp, pp)
    out = solver.solve(loss="huber", max_iters=400, pcg_tol=1e-6, small_solver=1, **TIGHT)
    cams, pts = solver.get_params()
    report = []
    pr.certify(p.cams, p.pts, cams, pts, "huber", restart=False, report=report)      # IRLS weights on the pixel rows only
    print(f"huber: gradient ratio {report[0][0]:.3e}")
    _, sse, cost = solver.residuals("huber", want_vector=False)
    cc, pc = solver.prior_cost()
    assert abs(out["final_cost"] - (cost + cc + pc)) <= 1e-12 * out["final_cost"]
    solver.set_priors()


# ---------------------------------------------------------------- 6. the priors act, and scale with sigma
def test_displacement_from_the_mean_shrinks_with_sigma(solver):
    p, cp, pp = standard_input()
    c = p.n_cams - 1
    mu = cp[0][c, 3:].copy()
    kw = dict(loss="linear", max_iters=100, pcg_tol=1e-8, small_solver=1, **TIGHT)
    dist, sols = [], []
    for sigma in (1e-2, 1e-4, 1e-6):
        cL = cp[1].copy()
        cL[c] = 0.0
        cL[c, 3:, 3:] = np.eye(3) / sigma ** 2
        solver.set_problem(p)
        solver.set_priors((cp[0], cL), pp)
        solver.solve(**kw)
        cams, pts = solver.get_params()
        dist.append(float(np.linalg.norm(cams[c, 3:] - mu)))
        sols.append(cams)
    print("|t - mu| of camera 11 at sigma 1e-2, 1e-4, 1e-6:", " ".join(f"{d:.3e}" for d in dist))
    assert dist[0] > dist[1] > dist[2]
    # ... and the solve without priors, gauge fixed by camera 0 instead, ends somewhere else
    solver.set_problem(BAProblem(p.cams, p.pts, p.cam_idx, p.pt_idx, p.uv, p.K4, 0))
    solver.solve(**kw)
    plain, _ = solver.get_params()
    assert np.abs(plain - sols[0]).max() > 1e-4


# ---------------------------------------------------------------- 7. covariances on a gauge the priors fix
def test_covariance_with_priors_matches_the_dense_inverse(solver):
    p, cp, pp = standard_input()
    # one more point, seen once: without a prior its depth is unobservable (NaN); with one it is an ordinary point
    o0 = int(np.nonzero(p.cam_idx == 3)[0][0])
    extra = p.pts[p.pt_idx[o0]] + 0.03
    q = BAProblem(p.cams, np.concatenate([p.pts, extra[None]]), np.append(p.cam_idx, np.int32(3)),
                  np.append(p.pt_idx, np.int32(p.n_pts)), np.concatenate([p.uv, p.uv[o0][None] + 0.7]), p.K4, -1)
    pm = np.concatenate([pp[0], extra[None]])
    pL = np.concatenate([pp[1], np.zeros((1, 3, 3))])
    pL1 = pL.copy()
    pL1[-1] = rotated_info(np.random.default_rng(3), [0.02, 0.03, 0.05])
    kw = dict(loss="linear", max_iters=60, pcg_tol=1e-6, small_solver=1, **TIGHT)
    # the parent's behaviour on the same problem without priors: the free gauge is refused by name
    solver.set_problem(q)
    solver.solve(**kw)
    with pytest.raises(hip_backend.BAHipError, match="error -4: .*gauge"):
        solver.covariance(full=True)
    for info, finite in ((pL, False), (pL1, True)):
        solver.set_problem(q)
        solver.set_priors(cp, (pm, info))
        solver.solve(**kw)
        cams, pts = solver.get_params()
        out = solver.covariance(full=True)
        pr = _reference(q, cp, (pm, info))
        ref = prior_covariance(pr, cams, pts)
        check_covariance(ref, out, 6)
        assert bool(np.isfinite(out["points"][-1]).all()) == finite and bool(np.isnan(out["points"][-1]).all()) != finite
        if finite:
            assert not ref["onecam"][-1] and _rel(out["points"][-1], ref["points"][-1]) <= 1e-9
            # the Schur-complement reference IS the dense inverse of H + L
            A, _ = pr.dense_system(cams, pts)
            Sigma = np.linalg.inv(A)
            n = 6 * q.n_cams
            np.testing.assert_allclose(ref["full"], Sigma[:n, :n], rtol=0, atol=1e-7 * np.abs(Sigma[:n, :n]).max())
            np.testing.assert_allclose(out["points"][-1], Sigma[-3:, -3:], rtol=0, atol=1e-7 * np.abs(Sigma[-3:, -3:]).max())
    solver.set_priors()


# ---------------------------------------------------------------- 8. BAL
def test_bal_intrinsics_regulariser_and_the_nb9_refusal(solver):
    p = make_bal_problem(16, 800, 3500, seed=2)
    sig = (18.0, 0.01, 0.003)
    q, out = bal.solve(p, intrinsics_sigma=sig, loss="linear", max_iters=300, pcg_tol=1e-6, **TIGHT)
    assert out["final_cost"] < out["initial_cost"]
    mean = np.zeros((p.n_cams, 9))
    info = np.zeros((p.n_cams, 9, 9))
    mean[:, 6:] = p.cams[:, 6:]
    info[:, 6:, 6:] = np.diag(1.0 / np.square(sig))
    pr = PriorProblem(Reduced(p.cams, p.pts, p.cam_idx, p.pt_idx, p.uv, None, -1), (mean, info), None)
    report = []
    pr.certify(p.cams, p.pts, q.cams, q.pts, "linear", restart=False, report=report)
    print(f"BAL with the calibration regulariser: gradient ratio {report[0][0]:.3e}")
    free, _ = bal.solve(p, loss="linear", max_iters=300, pcg_tol=1e-6, **TIGHT)
    assert np.abs(free.cams[:, 6:] - q.cams[:, 6:]).max() > 1e-6          # (the regulariser is not ignored)
    # nb = 9 priors followed by a pinhole solve / linearisation / cost
    pin = make_problem(12, 800, 5, seed=4)
    solver.set_problem(pin)
    solver.set_priors(cams={2: (np.zeros(9), np.eye(9))})
    for call in (lambda: solver.solve(loss="huber", max_iters=3, small_solver=1), lambda: solver.linearize("huber"),
                 lambda: solver.schur_system(1e-3), lambda: solver.covariance(), lambda: solver.prior_cost()):
        with pytest.raises(hip_backend.BAHipError, match="error -1: .*nb = 9 .*BAL camera model"):
            call()
    solver.set_priors()
    assert solver.solve(loss="huber", max_iters=3, small_solver=1)["status"] >= 0


# ---------------------------------------------------------------- 9. two ranks
WORKER = r"""
import json, os, sys
import numpy as np
sys.path.insert(0, %(root)r)
import torch.distributed as dist
from bundle_adjustment_amd import hip_backend
from bundle_adjustment_amd.problem import BAProblem, extract_shard, shard_by_landmark
from tests.prior_reference import standard_input
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group(backend="gloo")
p, cp, pp = standard_input(outlier_frac=0.02)
p = BAProblem(p.cams, p.pts, p.cam_idx, p.pt_idx, p.uv, p.K4, p.fixed_cam, cam_prior=cp, pt_prior=pp)
b, e = shard_by_landmark(p, world)[rank]
sub, _ = extract_shard(p, b, e)
s = hip_backend.Solver(0)
uid = [hip_backend.comm_unique_id() if rank == 0 else None]
dist.broadcast_object_list(uid, src=0)
s.comm_init(rank, world, uid[0])
s.set_problem(sub)
out = s.solve(loss="huber", max_iters=25, ftol=1e-13, xtol=1e-13, gtol=1e-12, pcg_tol=1e-3)
cams, pts = s.get_params()
out["prior_cost"] = s.prior_cost()
out["prior_blocks"] = s.stats()["prior_blocks"]
np.save(os.path.join(%(out)r, f"cams_{rank}.npy"), cams)
np.save(os.path.join(%(out)r, f"pts_{rank}.npy"), pts)
json.dump(out, open(os.path.join(%(out)r, f"out_{rank}.json"), "w"))
s.close()
dist.barrier()
dist.destroy_process_group()
"""


def _free_port():
    import socket
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    return str(port)


def test_two_ranks_with_priors_match_one_rank(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(WORKER % dict(root=ROOT, out=str(tmp_path)))
    env = dict(os.environ, BA_COMM="shm")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", _free_port(), str(script)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    p, cp, pp = standard_input(outlier_frac=0.02)
    with hip_backend.Solver(0) as s:
        s.set_problem(BAProblem(p.cams, p.pts, p.cam_idx, p.pt_idx, p.uv, p.K4, p.fixed_cam, cam_prior=cp, pt_prior=pp))
        ref = s.solve(loss="huber", max_iters=25, ftol=1e-13, xtol=1e-13, gtol=1e-12, pcg_tol=1e-3, small_solver=1)
        cams_ref, pts_ref = s.get_params()
        cc_ref, pc_ref = s.prior_cost()
    outs = [json.load(open(tmp_path / f"out_{k}.json")) for k in range(2)]
    for key in ("iterations", "accepted", "final_sse", "final_cost", "initial_cost"):
        assert outs[0][key] == outs[1][key], key
    # the camera prior cost is counted once: the total of two ranks is the total of one
    assert cc_ref > 1e-6 * ref["final_cost"]
    assert abs(outs[0]["initial_cost"] - ref["initial_cost"]) <= 1e-10 * ref["initial_cost"]
    assert abs(outs[0]["final_cost"] - ref["final_cost"]) <= 1e-9 * ref["final_cost"]
    cams0 = np.load(tmp_path / "cams_0.npy")
    assert np.array_equal(cams0, np.load(tmp_path / "cams_1.npy"))
    assert np.abs(cams0 - cams_ref).max() <= 1e-6
    pts = np.concatenate([np.load(tmp_path / f"pts_{k}.npy") for k in range(2)])
    assert np.abs(pts - pts_ref).max() <= 1e-5
    # ba_prior_cost: the camera sum as on one rank, the point sums of the shards add up
    assert outs[0]["prior_cost"][0] == outs[1]["prior_cost"][0]
    assert abs(outs[0]["prior_cost"][0] - cc_ref) <= 1e-6 * cc_ref
    assert abs(outs[0]["prior_cost"][1] + outs[1]["prior_cost"][1] - pc_ref) <= 1e-6 * pc_ref
    assert outs[0]["prior_blocks"] + outs[1]["prior_blocks"] == 2 * 2 + p.n_pts // 20


# ---------------------------------------------------------------- 10. the error rules
def test_error_rules_and_the_handle_afterwards(solver):
    p = make_problem(12, 800, 5, seed=15)
    solver.set_problem(p)
    lib, h, dp = solver._lib, solver._h, hip_backend._dp
    nc, npt = p.n_cams, p.n_pts

    def raw(nb, cm, ci, pm, pi):
        rc = lib.ba_set_priors(h, nb, dp(cm), dp(ci), dp(pm), dp(pi))
        return rc, lib.ba_last_error().decode()

    cm, ci = np.zeros((nc, 6)), np.zeros((nc, 21))
    pm, pi = np.zeros((npt, 3)), np.zeros((npt, 6))
    ci[4, 0] = 1.0
    rc, msg = raw(7, cm, ci, None, None)
    assert rc == -1 and "nb must be 6" in msg
    bad = ci.copy()
    bad[5, [0, 6, 11]] = [1.0, 1.0, -1.0]                  # diag(1, 1, -1, 0, 0, 0): indefinite
    rc, msg = raw(6, cm, bad, None, None)
    assert rc == -1 and "camera 5" in msg and "positive semidefinite" in msg
    bad = ci.copy()
    bad[7, 3] = np.nan
    rc, msg = raw(6, cm, bad, None, None)
    assert rc == -1 and "camera 7" in msg and "non-finite entry" in msg
    badm = cm.copy()
    badm[4, 2] = np.inf                                    # camera 4's block is non-zero
    rc, msg = raw(6, badm, ci, None, None)
    assert rc == -1 and "camera 4" in msg and "non-finite mean" in msg
    badm = cm.copy()
    badm[3, 2] = np.nan                                    # camera 3's block is zero: its mean is not read
    assert raw(6, badm, ci, None, None)[0] == 0
    bpi = pi.copy()
    bpi[17] = [1.0, 2.0, 0.0, 1.0, 0.0, 1.0]               # [[1, 2, 0], [2, 1, 0], [0, 0, 1]]: eigenvalue -1
    rc, msg = raw(6, None, None, pm, bpi)
    assert rc == -1 and "point 17" in msg and "positive semidefinite" in msg
    rc, msg = raw(6, cm, None, None, None)
    assert rc == -1 and "both or neither" in msg
    with pytest.raises(ValueError, match="camera 2: .*not positive semidefinite"):      # the same rule, one layer up
        solver.set_priors(cams={2: (np.zeros(6), -np.eye(6))})
    # a refused call leaves the priors that were set (camera 4, from the zero-mean call above); clear, then solve as a fresh handle
    assert solver.stats()["prior_blocks"] == 1
    solver.set_priors()
    assert solver.stats()["prior_blocks"] == 0
    kw = dict(loss="huber", max_iters=8, small_solver=1)
    with hip_backend.Solver(0) as plain:
        plain.set_problem(p)
        ref = plain.solve(**kw)
        cref, pref = plain.get_params()
    solver.set_params(p.cams, p.pts)
    a = solver.solve(**kw)
    ca, pa = solver.get_params()
    assert a["final_cost"] == ref["final_cost"] and a["iterations"] == ref["iterations"]
    assert np.array_equal(ca, cref) and np.array_equal(pa, pref)
    solver.set_priors(cams={1: (p.cams[1], np.eye(6))})
    solver.set_problem(p)                                  # cleared by set_problem
    assert solver.stats()["prior_blocks"] == 0
    solver.solve(**kw)
    cb, pb = solver.get_params()
    assert np.array_equal(cb, cref) and np.array_equal(pb, pref)
