"""GPU: the single-launch direct solver for sliding-window-sized problems (csrc/ba_small.hpp; the reference's default
BundleAdjuster(window_size=5), src/pipeline.py:39,99).  Same options / summary / trace as the multi-kernel path; the
reduced camera system is solved exactly (dense Cholesky) instead of by PCG, so the two paths walk different LM
trajectories to the SAME minimiser."""
import time

import numpy as np
import pytest

from bundle_adjustment_amd import hip_backend
from bundle_adjustment_amd.synthetic import make_problem
from oracle import ba_oracle as o
from tests.helpers import golden_flat_problem, load_golden
from tests.lm_trace import check_self_consistent

pytestmark = pytest.mark.gpu
TIGHT = dict(max_iters=60, ftol=1e-14, xtol=1e-14, gtol=0.0)


@pytest.mark.parametrize("loss", ["linear", "huber"])
def test_small_solver_reaches_the_minimiser_of_the_multi_kernel_path(loss):
    p = make_problem(5, 500, 4, seed=3, outlier_frac=0.03)
    with hip_backend.Solver(0) as s:
        s.set_problem(p)
        small = s.solve(loss=loss, **TIGHT)
        tr = s.trace()
        cams_s, pts_s = s.get_params()
        r, sse, cost = s.residuals(loss)
        s.set_problem(p)
        multi = s.solve(loss=loss, small_solver=1, pcg_tol=1e-3, **TIGHT)
        cams_m, pts_m = s.get_params()
    assert small["pcg_iterations"] == 0 and multi["pcg_iterations"] > 0          # the two paths really are different
    # (Huber by IRLS converges linearly: after 60 iterations the exact-step path sits slightly lower than the inexact one)
    tol = 1e-9 if loss == "linear" else 1e-5
    assert abs(small["final_cost"] - multi["final_cost"]) <= tol * multi["final_cost"]
    assert small["final_cost"] <= multi["final_cost"] * (1 + 1e-9)
    assert abs(np.sqrt(small["final_sse"] / p.n_obs) - np.sqrt(multi["final_sse"] / p.n_obs)) <= (1e-6 if loss == "linear" else 1e-3)
    # the summary describes the parameters the handle now holds
    assert abs(sse - small["final_sse"]) <= 1e-10 * sse and abs(cost - small["final_cost"]) <= 1e-10 * cost
    ref = o.residuals(cams_s, pts_s, p.cam_idx, p.pt_idx, p.uv, p.K4)
    assert np.abs(r - ref).max() <= 1e-9
    assert np.array_equal(cams_s[0], p.cams[0])                                    # the fixed camera did not move
    assert len(tr) == small["iterations"] and sum(t["accepted"] for t in tr) == small["accepted"]
    assert abs(tr[0]["cost"] - small["initial_cost"]) <= 1e-12 * small["initial_cost"]
    # only camera 0 is fixed, so the monocular SCALE is free: the minimiser is a one-parameter family and the two paths
    # stop at different members of it.  Rotations agree; translations and points agree after removing the scale.
    gt = 1e-4 if loss == "linear" else 5e-3            # (the Huber runs are still creeping after 60 iterations)
    assert np.abs(cams_s[:, :3] - cams_m[:, :3]).max() <= 1e-2 * gt
    sc = np.linalg.norm(cams_m[1, 3:]) / np.linalg.norm(cams_s[1, 3:])
    assert np.abs(sc * cams_s[:, 3:] - cams_m[:, 3:]).max() <= gt * np.abs(cams_m[:, 3:]).max()
    assert np.abs(sc * pts_s - pts_m).max() <= gt * np.abs(pts_m).max()


@pytest.mark.parametrize("name", ["conv_linear", "conv_huber"])
def test_small_solver_converged_rmse_matches_scipy_goldens(name):
    """The 4-keyframe scenes scipy drove to convergence on the imported reference's residual (make_golden.py section D)
    fall to the direct solver: final RMSE within 1e-6 px, converged cost within 1e-8 relative."""
    g = load_golden(name)
    p = golden_flat_problem(g)
    loss = str(g["loss"])
    with hip_backend.Solver(0) as s:
        s.set_problem(p)
        out = s.solve(loss=loss, **TIGHT)
    assert out["pcg_iterations"] == 0
    n_obs = p.n_obs
    assert abs(np.sqrt(out["final_sse"] / n_obs) - np.sqrt(float((g["res_fun"] ** 2).sum()) / n_obs)) <= 1e-6
    assert abs(out["final_cost"] - float(g["res_cost"])) <= 1e-8 * float(g["res_cost"])


def _with_duplicates(p, n_dup, seed):
    """n_dup extra observations that repeat an existing (camera, point) pair with a slightly different pixel."""
    rng = np.random.default_rng(seed)
    pick = rng.choice(p.n_obs, n_dup, replace=False)
    return type(p)(p.cams, p.pts, np.concatenate([p.cam_idx, p.cam_idx[pick]]), np.concatenate([p.pt_idx, p.pt_idx[pick]]),
                   np.concatenate([p.uv, p.uv[pick] + rng.normal(0, 0.5, (n_dup, 2))]), p.K4, p.fixed_cam)


@pytest.mark.parametrize("n_cams,n_pts,k,loss,dups", [
    (2, 37, 2, "huber", 0),         # 12 + 1 rows: 1 tile row
    (3, 130, 3, "linear", 5),       # 18 + 1 rows: 2 tile rows; repeated (camera, point) pairs add up inside V
    (5, 333, 4, "huber", 0),        # 30 + 1 rows; a point count that is no multiple of 16
    (6, 700, 4, "linear", 9),       # 36 + 1 rows: 3 tile rows; more points than threads
    (7, 256, 5, "huber", 0),        # 42 + 1 rows
    (8, 513, 6, "linear", 0),       # 48 + 1 rows: the z row alone in tile row 3
    # no repeated pairs, up to 2048 landmarks: the multi-workgroup kernel (ba_small_mw.hpp; the 7- and 8-camera rows above too)
    (5, 129, 4, "huber", 0),        # 3 workgroups, the last one with a single landmark
    (4, 512, 3, "linear", 0),       # 8 full workgroups
    (5, 1000, 5, "huber", 0),       # 16 workgroups, every landmark seen by every camera
    (3, 700, 2, "linear", 0),       # 11 workgroups, 18 + 1 rows
    (2, 300, 2, "huber", 0),        # 12 + 1 rows, one adjustable camera
    (5, 1531, 4, "huber", 0),       # 24 workgroups, 6124 observations: just under the dispatch limit of the window solver
])
def test_small_solver_follows_the_oracles_dense_lm_step_by_step(n_cams, n_pts, k, loss, dups):
    """Every LM iteration of k_small_lm against the oracle's LM with the explicit reduced system solved exactly
    (oracle lm_solve(linear_solver='dense')): trial cost, gain ratio, damping and acceptance per iteration, then the
    final parameters.  fp64 throughout; the device forms S with fp64 MFMA tiles and a Cholesky factorisation, numpy with
    LAPACK's LU -- agreement to 1e-9 relative per iteration is what the two orders of summation leave."""
    p = make_problem(n_cams, n_pts, min(k, n_cams), seed=17 + n_cams, outlier_frac=0.03 if loss == "huber" else 0.0)
    if dups:
        p = _with_duplicates(p, dups, seed=n_cams)
    iters = 6
    ref = o.lm_solve(p.cams, p.pts, p.cam_idx, p.pt_idx, p.uv, p.K4, fixed_cam=p.fixed_cam, loss=loss, max_iters=iters,
                     ftol=0.0, xtol=0.0, gtol=0.0, linear_solver="dense")
    with hip_backend.Solver(0) as s:
        s.set_problem(p)
        out = s.solve(loss=loss, max_iters=iters, ftol=0.0, xtol=0.0, gtol=0.0)
        tr = s.trace()
        cams, pts = s.get_params()
    check_self_consistent(out, tr, {})
    assert out["pcg_iterations"] == 0 and out["iterations"] == iters == len(ref["history"])
    for t, h in zip(tr, ref["history"]):
        assert abs(t["cost"] - h["cost"]) <= 1e-9 * h["cost"]
        assert abs(t["cost_trial"] - h["cost_new"]) <= 1e-9 * h["cost_new"], (t, h)
        assert abs(t["damping"] - h["lam"]) <= 1e-6 * h["lam"]
        assert bool(t["accepted"]) == bool(h["rho"] > 0)
        assert abs(t["step_norm"] - h["step"]) <= 1e-7 * max(h["step"], 1e-12)
    assert abs(out["final_cost"] - ref["cost"]) <= 1e-9 * ref["cost"]
    assert np.abs(cams - ref["cams"]).max() <= 1e-7 * max(1.0, np.abs(ref["cams"]).max())
    assert np.abs(pts - ref["pts"]).max() <= 1e-7 * max(1.0, np.abs(ref["pts"]).max())


def test_small_solver_rejected_steps_follow_the_oracle():
    """A start far from the minimiser (0.2 rad, 1 m, 3 m of noise): the first four steps are rejected -- same linearisation,
    larger damping, no re-linearisation in the kernel -- then the descent starts; acceptance, damping and trial costs
    against the oracle's dense LM, iteration by iteration."""
    p = make_problem(5, 200, 4, seed=5, point_sigma=3.0, rot_sigma=0.2, trans_sigma=1.0)
    iters = 10
    ref = o.lm_solve(p.cams, p.pts, p.cam_idx, p.pt_idx, p.uv, p.K4, fixed_cam=0, loss="huber", max_iters=iters, ftol=0.0, xtol=0.0,
                     gtol=0.0, lam0=1e-6, linear_solver="dense")
    assert [h["rho"] > 0 for h in ref["history"]][:5] == [False, False, False, False, True]
    with hip_backend.Solver(0) as s:
        s.set_problem(p)
        out = s.solve(loss="huber", max_iters=iters, ftol=0.0, xtol=0.0, gtol=0.0, initial_lambda=1e-6)
        tr = s.trace()
    assert out["pcg_iterations"] == 0 and out["iterations"] == iters
    for t, h in zip(tr, ref["history"]):
        assert bool(t["accepted"]) == bool(h["rho"] > 0)
        assert abs(t["damping"] - h["lam"]) <= 1e-6 * h["lam"]
        assert abs(t["cost_trial"] - h["cost_new"]) <= 1e-6 * h["cost_new"], (t, h)
    assert abs(out["final_cost"] - ref["cost"]) <= 1e-6 * ref["cost"]


def test_small_solver_with_only_the_fixed_camera():
    """One keyframe, fixed: nothing but points move, each onto the ray of its single observation (cost -> 0)."""
    p = make_problem(1, 40, 1, seed=18)
    with hip_backend.Solver(0) as s:
        s.set_problem(p)
        out = s.solve(max_iters=8, ftol=0.0, xtol=0.0, gtol=0.0)
        cams, _ = s.get_params()
    assert out["pcg_iterations"] == 0 and out["final_cost"] <= 1e-12 * out["initial_cost"]
    assert np.array_equal(cams, p.cams)


def test_small_solver_is_bit_reproducible_and_honours_the_options():
    p = make_problem(8, 1200, 5, seed=9, outlier_frac=0.02)
    with hip_backend.Solver(0) as s:
        outs = []
        for _ in range(2):
            s.set_problem(p)
            outs.append((s.solve(loss="huber", max_iters=25, ftol=1e-10, xtol=1e-12, gtol=1e-12), s.get_params()))
        assert outs[0][0]["final_cost"] == outs[1][0]["final_cost"] and outs[0][0]["iterations"] == outs[1][0]["iterations"]
        assert np.array_equal(outs[0][1][0], outs[1][1][0]) and np.array_equal(outs[0][1][1], outs[1][1][1])
        s.set_problem(p)
        three = s.solve(loss="huber", max_iters=3, ftol=0.0, xtol=0.0, gtol=0.0)
        assert three["iterations"] == 3 and three["status_name"] == "max_iters"
        s.set_problem(p)
        loose = s.solve(loss="huber")                      # the reference's tolerances: stops on ftol
        assert loose["status_name"] in ("ftol", "xtol") and loose["final_cost"] < 0.2 * loose["initial_cost"]      # (2 % gross outliers stay in the Huber cost)
        # nine cameras: not the single-launch solver's case any more.  More than 6144 observations (the ONE-workgroup
        # kernel's measured crossover): still its case while the window fits the multi-workgroup
        # kernel (2048 landmarks), the multi-kernel path beyond that
        q = make_problem(9, 600, 4, seed=1)
        s.set_problem(q)
        assert s.solve(max_iters=5)["pcg_iterations"] > 0
        q = make_problem(8, 1300, 5, seed=1)
        assert q.n_obs > 6144
        s.set_problem(q)
        assert s.solve(max_iters=5)["pcg_iterations"] == 0
        q = make_problem(8, 2100, 3, seed=1)
        assert q.n_obs > 6144 and q.n_pts > 2048
        s.set_problem(q)
        assert s.solve(max_iters=5)["pcg_iterations"] > 0
        # NaN pixel: the same failure code as the multi-kernel path
        uv = p.uv.copy(); uv[7, 1] = np.nan
        s.set_problem(type(p)(p.cams, p.pts, p.cam_idx, p.pt_idx, uv, p.K4, 0))
        with pytest.raises(hip_backend.BAHipError, match="non-finite cost at the initial parameters"):
            s.solve()
        s.set_problem(p)
        assert s.solve()["final_cost"] > 0


def test_small_solver_on_a_reused_handle_with_fewer_landmarks():
    """One Solver kept across windows (BundleAdjuster.run's default use, src/pipeline.py:39,99): a window of 100 landmarks,
    then one of 97 with the same number of cameras -- the same 16-column padding of V.  The second solve must not see
    the columns the first one left for points 97..99: results bit-equal to a fresh handle, and on the oracle's dense LM."""
    big = make_problem(5, 100, 4, seed=21, outlier_frac=0.03)
    keep = big.pt_idx < 97
    small = type(big)(big.cams, big.pts[:97], big.cam_idx[keep], big.pt_idx[keep], big.uv[keep], big.K4, big.fixed_cam)
    kw = dict(loss="huber", max_iters=6, ftol=0.0, xtol=0.0, gtol=0.0)
    with hip_backend.Solver(0) as fresh:
        fresh.set_problem(small)
        want = fresh.solve(**kw)
        want_tr = fresh.trace()
        want_cams, want_pts = fresh.get_params()
    with hip_backend.Solver(0) as s:
        s.set_problem(big)
        first = s.solve(**kw)
        assert first["pcg_iterations"] == 0 and first["final_cost"] < first["initial_cost"]
        s.set_problem(small)
        got = s.solve(**kw)
        got_tr = s.trace()
        cams, pts = s.get_params()
    assert got["pcg_iterations"] == 0
    assert got["final_cost"] == want["final_cost"] and got["final_sse"] == want["final_sse"]
    assert [t["cost_trial"] for t in got_tr] == [t["cost_trial"] for t in want_tr]
    assert np.array_equal(cams, want_cams) and np.array_equal(pts, want_pts)
    ref = o.lm_solve(small.cams, small.pts, small.cam_idx, small.pt_idx, small.uv, small.K4, fixed_cam=small.fixed_cam,
                     loss="huber", max_iters=6, ftol=0.0, xtol=0.0, gtol=0.0, linear_solver="dense")
    for t, h in zip(got_tr, ref["history"]):
        assert abs(t["cost_trial"] - h["cost_new"]) <= 1e-9 * h["cost_new"], (t, h)
        assert bool(t["accepted"]) == bool(h["rho"] > 0)
    assert abs(got["final_cost"] - ref["cost"]) <= 1e-9 * ref["cost"]


@pytest.mark.parametrize("n_cams,n_pts,k,fixed", [(5, 500, 4, 0), (5, 777, 3, 2), (4, 130, 4, 3), (6, 400, 4, 0), (7, 300, 5, 6), (8, 900, 6, 0)])
def test_multi_workgroup_window_solver_agrees_with_the_single_workgroup_one(monkeypatch, n_cams, n_pts, k, fixed):
    """k_small_mw (several workgroups, two exchanges per LM iteration) against k_small_lm (BA_SMALL_MW=0) on the same
    handle and problem: same iteration count, verdicts and damping, costs to 1e-10 relative (the partial sums are
    grouped by workgroup instead of by wave), parameters to 1e-9; the multi-workgroup result repeats bit for bit.
    fixed = 2 / 3: the held camera in the middle / at the end."""
    p = make_problem(n_cams, n_pts, k, seed=40 + n_pts, outlier_frac=0.02)
    p = type(p)(p.cams, p.pts, p.cam_idx, p.pt_idx, p.uv, p.K4, fixed)
    kw = dict(loss="huber", max_iters=8, ftol=0.0, xtol=0.0, gtol=0.0)
    res = {}
    with hip_backend.Solver(0) as s:
        for mode in ("1", "0", "1"):
            monkeypatch.setenv("BA_SMALL_MW", mode)
            s.set_problem(p)
            out = s.solve(**kw)
            res.setdefault(mode, []).append((out, s.trace(), s.get_params()))
    (o1, t1, (c1, x1)), (o1b, _, (c1b, x1b)) = res["1"]
    (o0, t0, (c0, x0)), = res["0"]
    assert o1["pcg_iterations"] == 0 and o1["iterations"] == o0["iterations"] == 8
    assert o1["final_cost"] == o1b["final_cost"] and np.array_equal(c1, c1b) and np.array_equal(x1, x1b)
    for a, b in zip(t1, t0):
        assert a["accepted"] == b["accepted"]
        assert abs(a["cost_trial"] - b["cost_trial"]) <= 1e-10 * b["cost_trial"]
        assert abs(a["damping"] - b["damping"]) <= 1e-7 * b["damping"]
    assert abs(o1["final_cost"] - o0["final_cost"]) <= 1e-10 * o0["final_cost"]
    assert np.abs(c1 - c0).max() <= 1e-9 * max(1.0, np.abs(c0).max()) and np.abs(x1 - x0).max() <= 1e-9 * max(1.0, np.abs(x0).max())


def test_multi_workgroup_window_solver_on_random_window_shapes(monkeypatch):
    """Forty windows of random shape -- 2 .. 8 cameras, landmark counts around the workgroup boundaries (63, 64, 65, 127,
    ... 1500), 2 .. Nc observations per landmark, the held camera anywhere, both losses -- through k_small_mw and through
    k_small_lm on the same handle: same verdict for every step that changes the cost by more than 1e-7, final cost to 1e-7
    relative."""
    rng = np.random.default_rng(123)
    kw = dict(max_iters=6, ftol=0.0, xtol=0.0, gtol=0.0)
    with hip_backend.Solver(0) as s:
        for case in range(40):
            nc = int(rng.integers(2, 9))
            npt = int(rng.choice([7, 63, 64, 65, 127, 128, 129, 200, 333, 511, 512, 513, 777, 1000, 1500]))
            k = int(rng.integers(2, nc + 1))
            npt = min(npt, 6000 // k)                                  # both kernels take it (6144-observation limit of k_small_lm)
            fixed = int(rng.integers(0, nc))
            loss = "huber" if rng.random() < 0.6 else "linear"
            p = make_problem(nc, npt, k, seed=int(rng.integers(0, 10000)), outlier_frac=0.03 if loss == "huber" else 0.0)
            p = type(p)(p.cams, p.pts, p.cam_idx, p.pt_idx, p.uv, p.K4, fixed)
            res = {}
            for mode in ("1", "0"):
                monkeypatch.setenv("BA_SMALL_MW", mode)
                s.set_problem(p)
                res[mode] = (s.solve(loss=loss, **kw), s.trace())
            (o1, t1), (o0, t0) = res["1"], res["0"]
            what = (case, nc, npt, k, fixed, loss)
            assert o1["pcg_iterations"] == 0 and o0["pcg_iterations"] == 0 and o1["iterations"] == o0["iterations"] == 6, what
            for a, b in zip(t1, t0):                                 # (at the noise floor a step's verdict is decided by rounding)
                if abs(b["cost"] - b["cost_trial"]) > 1e-7 * b["cost"]:
                    assert a["accepted"] == b["accepted"], what
            # (two-view landmarks and a handful of them per camera pair make some of these windows ill-conditioned: the
            # Gauss-Jordan sweeps and the Cholesky factorisation then differ by more than on the well-posed windows above)
            assert abs(o1["final_cost"] - o0["final_cost"]) <= 1e-7 * o0["final_cost"], what



def test_window_solver_falls_back_when_a_barrier_is_not_served(monkeypatch):
    """The workgroups of k_small_mw meet at a counter barrier and the launch is an ordinary one: nothing promises that they
    are resident together.  BA_DEBUG_MW_EXTRA_WG makes every barrier wait for one workgroup more than the launch has, i.e.
    the bounded spin (50 ms of the device clock) runs out at the first barrier in every workgroup.  ba_solve must then
    return BA_OK with the result of the one-workgroup kernel on the SAME start point, in the same process, and count the
    fall-back; the next solve on the handle (hook off) goes through k_small_mw again."""
    p = make_problem(5, 500, 4, seed=77, outlier_frac=0.02)
    kw = dict(loss="huber", max_iters=8, ftol=0.0, xtol=0.0, gtol=0.0)
    with hip_backend.Solver(0) as s:
        monkeypatch.setenv("BA_SMALL_MW", "0")
        s.set_problem(p)
        ref, ref_par = s.solve(**kw), s.get_params()
        monkeypatch.delenv("BA_SMALL_MW")
        st0 = s.stats()
        monkeypatch.setenv("BA_DEBUG_MW_EXTRA_WG", "1")
        s.set_problem(p)
        out, par = s.solve(**kw), s.get_params()
        st1 = s.stats()
        assert st1["window_fallbacks"] == st0["window_fallbacks"] + 1
        assert st1["window_mw_launches"] == st0["window_mw_launches"] + 1 and st1["window_lm_launches"] == st0["window_lm_launches"] + 1
        # the very kernel, the very start point: identical bits
        assert out["iterations"] == ref["iterations"] == 8 and out["final_cost"] == ref["final_cost"] and out["final_sse"] == ref["final_sse"]
        assert np.array_equal(par[0], ref_par[0]) and np.array_equal(par[1], ref_par[1])
        assert out["seconds_total"] < 2.0                      # a handful of 50 ms time-outs, not the host's 20 s limit
        monkeypatch.delenv("BA_DEBUG_MW_EXTRA_WG")
        s.set_problem(p)
        again = s.solve(**kw)
        st2 = s.stats()
        assert st2["window_fallbacks"] == st1["window_fallbacks"] and st2["window_mw_launches"] == st1["window_mw_launches"] + 1
        assert abs(again["final_cost"] - ref["final_cost"]) <= 1e-10 * ref["final_cost"]


def test_window_solver_survives_a_chip_somebody_else_occupies():
    """every compute unit but four holds a resident workgroup of ANOTHER stream with 100 KB of LDS
    (ba_debug_occupy: idle workgroups that leave after 600 ms of the device clock), so at most four of the eight workgroups
    of a 5-camera / 500-landmark window's k_small_mw launch (87 KB of LDS each) can be resident together.  The solve must
    come back BA_OK with the oracle's cost; whether it needed the fall-back depends on where the runtime put the
    occupying workgroups, so the counter is only reported -- the forced variant above asserts it."""
    p = make_problem(5, 500, 4, seed=78, outlier_frac=0.02)
    kw = dict(loss="huber", max_iters=30, ftol=1e-12, xtol=1e-12, gtol=0.0)
    ref = o.lm_solve(p.cams, p.pts, p.cam_idx, p.pt_idx, p.uv, p.K4, 0, linear_solver="dense", **kw)
    with hip_backend.Solver(0) as s, hip_backend.Solver(0) as hog:
        s.set_problem(p)
        n_cu = 256
        hog.debug_occupy(n_cu - 4, 100 * 1024, 600.0)
        time.sleep(0.02)                                         # the occupying workgroups are resident by now
        t0 = time.perf_counter()
        out = s.solve(**kw)
        dt = time.perf_counter() - t0
        st = s.stats()
        hog.synchronize()
    print(f"occupied chip: solve {dt * 1e3:.1f} ms, fall-backs {st['window_fallbacks']}, status {out['status_name']}")
    assert abs(out["final_cost"] - ref["cost"]) <= 1e-8 * ref["cost"]
    assert dt < 5.0
