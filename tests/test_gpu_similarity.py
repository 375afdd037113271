"""GPU: ba_transform / ba_align / ba_get_centres against the numpy yardstick of tests/similarity_reference.py -- the change
of frame on both camera models (parameters, residuals, rotation edge cases, what it leaves on the handle, refusals) and
the weighted, robust alignment (parity over losses / scale / rounds / reference sets, sizes around the wave and workgroup
boundaries, exact data, robustness, statuses, reproducibility, and the loop solve -> align).

Tolerances.  Transform: 1e-13 max(1, max |value|), about 50 roundings of a 3 x 3 product and an add.  Residuals: the
project's parity tolerance 1e-9 px; in the far frame (|t| = 5e5, s = 250) fp64 itself moves them, so the bound there is 4 x the
yardstick's own change + 1e-9; sse and cost 1e-10 relative in every frame.  Alignment: 1e-10 on s (relative), R (absolute),
t / max(1, |t0|) and every error d_i relative to itself (to the references' noise level, 0.05, where it is smaller), rms
and max relative to themselves."""
import functools
import math

import numpy as np
import pytest

from bundle_adjustment_amd import bal, hip_backend, similarity
from bundle_adjustment_amd.bal import BALProblem, from_pinhole
from bundle_adjustment_amd.problem import BAProblem
from bundle_adjustment_amd.synthetic import _project, bal_project, make_bal_like, make_problem, make_shared_bal_problem
from tests import similarity_cases as sc
from tests import similarity_reference as sr

pytestmark = pytest.mark.gpu
K4 = np.array([900.0, 900.0, 640.0, 360.0])
FAR = np.array([4.1e5, 5.2e6, 310.0])
NOISE = 0.05          # standard deviation of the noise on every set of references below


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------------- problems
@functools.lru_cache(maxsize=None)
def problem(model):
    """70 cameras / 257 points in either camera model, and the 5-camera / 120-point window."""
    if model == "window":
        return make_problem(5, 120, 4, seed=3)
    prob, cams_true, pts_true = make_problem(70, 257, 4, seed=7, K4=K4, return_truth=True)
    if model == "pinhole":
        return prob
    rng = np.random.default_rng(12)
    truth = from_pinhole(BAProblem(cams_true, pts_true, prob.cam_idx, prob.pt_idx, prob.uv, K4, 0))
    intr = np.stack([900.0 * (1.0 + 0.02 * rng.normal(size=70)), -0.03 + 0.01 * rng.normal(size=70),
                     0.003 * rng.choice([-1.0, 1.0], size=70)], axis=1)
    truth.cams[:, 6:9] = intr
    uv = bal_project(truth.cams, pts_true, truth.cam_idx, truth.pt_idx) + rng.normal(0.0, 0.5, size=(truth.n_obs, 2))
    start = from_pinhole(prob)
    start.cams[:, 6:9] = intr
    return BALProblem(start.cams, start.pts, truth.cam_idx, truth.pt_idx, uv).validate()


@functools.lru_cache(maxsize=None)
def sims():
    rng = np.random.default_rng(21)
    d = rng.normal(size=(2, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (("identity", 1.0, np.eye(3), np.zeros(3)), ("mid", 37.5, sr.random_rotation(rng), 100.0 * d[0]),
            ("far", 250.0, sr.random_rotation(rng), 5e5 * d[1]))


def upload(s, prob, fixed_cam=None):
    """-> the BAL intrinsics (None for the pinhole)."""
    if isinstance(prob, BALProblem):
        return s.set_problem_bal(prob, -1 if fixed_cam is None else fixed_cam)
    s.set_problem(prob)
    return None


def device_residuals(s, intr, loss="huber"):
    return s.residuals(loss) if intr is None else s._residuals_bal_resident(intr, loss)


def project(prob, cams, pts):
    if isinstance(prob, BALProblem):
        return bal_project(cams, pts, prob.cam_idx, prob.pt_idx)
    return _project(cams, pts, prob.cam_idx, prob.pt_idx, prob.K4)[0]


# ------------------------------------------------------------------------------------- 1, 2 transform and residuals
@pytest.mark.parametrize("k", range(3), ids=["identity", "mid", "far"])
@pytest.mark.parametrize("model", ["pinhole", "bal"])
def test_transform_matches_the_yardstick_and_keeps_the_residuals(model, k):
    prob = problem(model)
    _, sc, R, t = sims()[k]
    cams_y, pts_y, Rn_y = sr.transform(prob.cams, prob.pts, sc, R, t)
    y_change = float(np.abs(project(prob, cams_y, pts_y) - project(prob, prob.cams, prob.pts)).max())
    with hip_backend.Solver(0) as s:
        intr = upload(s, prob)
        r0, sse0, cost0 = device_residuals(s, intr)
        ctr0 = s.centres()
        s.transform(sc, R, t)
        cams, pts = s.get_params()
        r1, sse1, cost1 = device_residuals(s, intr)
        ctr1 = s.centres()
    d_pts = np.abs(pts - pts_y).max() / max(1.0, np.abs(pts_y).max())
    d_t = np.abs(cams[:, 3:6] - cams_y[:, 3:6]).max() / max(1.0, np.abs(cams_y[:, 3:6]).max())
    d_R = max(np.abs(sr.rodrigues(cams[c, :3]) - Rn_y[c]).max() for c in range(prob.n_cams))
    d_res = float(np.abs(r1 - r0).max())
    print(f"{model} {sims()[k][0]}: points {d_pts:.2e} t {d_t:.2e} (of the largest value) R {d_R:.2e}; residuals moved {d_res:.3e} px "
          f"(yardstick {y_change:.3e}); sse rel {abs(sse1 - sse0) / sse0:.2e} cost rel {abs(cost1 - cost0) / cost0:.2e}")
    assert d_pts <= 1e-13 and d_t <= 1e-13 and d_R <= 1e-13
    assert np.abs(sr.centres(prob.cams) - ctr0).max() <= 1e-13 * 20
    assert np.abs(ctr1 - (sc * ctr0 @ R.T + t)).max() <= 1e-13 * max(1.0, np.abs(ctr1).max()) * 10
    assert d_res <= (1e-9 if k < 2 else 4.0 * y_change + 1e-9)
    assert abs(sse1 - sse0) <= 1e-10 * sse0 and abs(cost1 - cost0) <= 1e-10 * cost0


# --------------------------------------------------------------------------------------------- 3 rotation edge cases
def test_rotation_edge_cases():
    """Cameras and R built so that R_c R^T has every angle from 0 to pi that a log map gets wrong."""
    prob = problem("pinhole")
    rng = np.random.default_rng(5)
    angles = (0.0, 1e-12, 1e-9, 1e-6, 1e-3, 1.0, math.pi - 1e-3, math.pi - 1e-5, math.pi - 1e-7, math.pi - 1e-9, math.pi)
    rnd = rng.normal(size=3)
    axes = [np.array([1.0, 0, 0]), np.array([0, -1.0, 0]), np.array([0, 0, 1.0]), np.array([1.0, 1.0, 0]) / math.sqrt(2.0),
            np.array([1.0, -1.0, 1.0]) / math.sqrt(3.0), rnd / np.linalg.norm(rnd)]
    R = sr.random_rotation(rng)
    cams = prob.cams.copy()
    for i, (th, ax) in enumerate((th, ax) for th in angles for ax in axes):
        cams[i, :3] = sr.log_map(sr.rodrigues(ax * th) @ R)
    with hip_backend.Solver(0) as s:
        s.set_problem(prob, with_params=False)
        s.set_params(cams, prob.pts)
        s.transform(1.0, R, np.array([0.3, -0.2, 0.1]))
        out = s.get_params()[0]
    worst = max(np.abs(sr.rodrigues(out[c, :3]) - sr.rodrigues(cams[c, :3]) @ R.T).max() for c in range(prob.n_cams))
    print(f"rotation edge cases: largest |R(rvec') - R_c R^T| {worst:.3e}, largest |rvec'| - pi {np.linalg.norm(out[:, :3], axis=1).max() - math.pi:.3e}")
    assert worst <= 1e-13
    assert np.linalg.norm(out[:, :3], axis=1).max() <= math.pi + 1e-12


# ------------------------------------------------------------------------------------------------- 4 handle state
def strip(d):
    return {k: v for k, v in d.items() if not k.startswith("seconds")}


def check_same_run(a, b):
    (sum_a, tr_a, par_a), (sum_b, tr_b, par_b) = a, b
    assert strip(sum_a) == strip(sum_b)
    assert [strip(r) for r in tr_a] == [strip(r) for r in tr_b] and len(tr_a) > 0
    for x, y in zip(par_a, par_b):
        assert same_bits(x, y)


@pytest.mark.parametrize("case", ["multi-kernel-held", "window"])
def test_transform_leaves_what_set_params_would(case):
    """Handle A: transform, solve.  Handle B: set_problem + set_params(A's parameters after the transform), solve.  Bit-equal."""
    import dataclasses
    _, sc, R, t = sims()[1]
    if case == "window":
        prob, kw = problem("window"), dict(max_iters=8)
    else:
        held_c = np.zeros((70, 6), dtype=bool)
        held_c[3, 3:6] = True
        held_p = np.zeros(257, dtype=bool)
        held_p[np.arange(20) * 12 + 5] = True
        prob, kw = dataclasses.replace(problem("pinhole"), cam_held=held_c, pt_held=held_p), dict(max_iters=8, small_solver=1)
    with hip_backend.Solver(0) as a:
        a.set_problem(prob)
        a.transform(sc, R, t)
        moved = a.get_params()
        run_a = (a.solve(**kw), a.trace(), a.get_params())
        stats = a.stats()
    with hip_backend.Solver(0) as b:
        b.set_problem(prob, with_params=False)
        if case != "window":
            b.set_held(prob.cam_held, prob.pt_held)
        b.set_params(*moved)
        run_b = (b.solve(**kw), b.trace(), b.get_params())
    check_same_run(run_a, run_b)
    assert run_a[0]["accepted"] > 0
    if case == "window":
        assert stats["window_mw_launches"] + stats["window_lm_launches"] > 0
    else:
        cams, pts = run_a[2]
        assert same_bits(cams[0], moved[0][0]) and same_bits(cams[3, 3:6], moved[0][3, 3:6]) and not same_bits(cams[3, :3], moved[0][3, :3])
        assert same_bits(pts[prob.pt_held], moved[1][prob.pt_held]) and not same_bits(pts[~prob.pt_held], moved[1][~prob.pt_held])


def test_transform_leaves_what_set_params_would_bal_shared():
    labels = np.arange(16) % 2
    prob, lab = make_shared_bal_problem(labels, 16, 800, 3500, seed=0)
    _, sc, R, t = sims()[1]
    kw = dict(max_iters=6)
    with hip_backend.Solver(0) as a:
        intr_a = a.set_problem_bal(prob)
        a.set_shared_intrinsics(lab)
        a.transform(sc, R, t)
        moved = a.get_params()
        run_a = (a.solve_bal_resident(intr_a, **kw), a.trace(), a.get_params() + (intr_a,))
    with hip_backend.Solver(0) as b:
        intr_b = b.set_problem_bal(prob)
        b.set_shared_intrinsics(lab)
        b.set_params(*moved)
        run_b = (b.solve_bal_resident(intr_b, **kw), b.trace(), b.get_params() + (intr_b,))
    check_same_run(run_a, run_b)
    assert run_a[0]["accepted"] > 0 and not same_bits(intr_a, prob.cams[:, 6:9])


@pytest.mark.parametrize("model", ["pinhole", "window", "bal"])
def test_transform_and_align_on_a_solved_handle(model):
    """The resident use: solve, then transform / align(apply) on the same handle (the current parameter set may be set 1),
    then solve again -- against a fresh handle given the parameters read in between.  A degenerate align with apply = 1 in
    between changes nothing, the linearisation included: the run stays bit-equal to one without it."""
    prob = problem(model)
    _, sc, R, t = sims()[1]
    kw = dict(max_iters=3) if model != "pinhole" else dict(max_iters=3, small_solver=1)
    n_pt = prob.n_pts

    def solve(s, intr):
        return s.solve(**kw) if intr is None else s.solve_bal_resident(intr, **kw)

    def session(degenerate, use_align):
        with hip_backend.Solver(0) as s:
            intr = upload(s, prob, 0)
            first = solve(s, intr)
            intr_first = None if intr is None else intr.copy()
            solved = s.get_params()
            r_solved = device_residuals(s, intr)[0]
            if degenerate:
                out = s.align(pt_ref=np.tile((1.0, 2.0, 3.0), (n_pt, 1)), pt_w=(np.arange(n_pt) < 2).astype(float), apply=True)
                assert out["status"] == 1
                out = s.align(pt_ref=np.outer(np.arange(float(n_pt)), (1.0, 2.0, 3.0)), apply=True)      # collinear references
                assert out["status"] == 2
                kept = s.get_params()
                assert same_bits(kept[0], solved[0]) and same_bits(kept[1], solved[1])
            if use_align:
                ref = sc * solved[1] @ R.T + t
                out = s.align(pt_ref=ref, apply=True)
                assert out["status"] == 0 and out["max"] <= 1e-9 * sc * 20
            else:
                s.transform(sc, R, t)
            moved = s.get_params()
            r_moved = device_residuals(s, intr)[0]
            again = (solve(s, intr), s.trace(), s.get_params() + (() if intr is None else (intr.copy(),)))
        return first, solved, moved, float(np.abs(r_moved - r_solved).max()), again, intr_first
    first, solved, moved, d_res, run_a, intr_after_first = session(False, False)
    cams_y, pts_y, _ = sr.transform(solved[0], solved[1], sc, R, t)
    assert first["accepted"] > 0 and d_res <= 1e-9
    assert np.abs(moved[1] - pts_y).max() <= 1e-13 * np.abs(pts_y).max() and np.abs(moved[0][:, 3:6] - cams_y[:, 3:6]).max() <= 1e-13 * np.abs(cams_y[:, 3:6]).max()
    # a fresh handle with the moved parameters (and, for the BAL camera, the intrinsics the first solve left)
    with hip_backend.Solver(0) as b:
        intr_b = upload(b, prob, 0)
        if intr_b is not None:
            intr_b[:] = intr_after_first
        b.set_params(*moved)
        run_b = (solve(b, intr_b), b.trace(), b.get_params() + (() if intr_b is None else (intr_b.copy(),)))
    check_same_run(run_a, run_b)
    _, _, moved_d, _, run_d, _ = session(True, False)
    assert same_bits(moved_d[0], moved[0]) and same_bits(moved_d[1], moved[1])
    check_same_run(run_a, run_d)
    _, _, moved_al, d_res_al, _, _ = session(False, True)
    assert d_res_al <= 1e-9 and np.abs(moved_al[1] - pts_y).max() <= 1e-9 * np.abs(pts_y).max()


# ----------------------------------------------------------------------------------------------------- 5 refusals
def test_refusals_leave_the_handle_as_found():
    prob = problem("pinhole")
    rot = sr.random_rotation(np.random.default_rng(1))
    with hip_backend.Solver(0) as s:
        with pytest.raises(hip_backend.BAHipError, match=r"-3.*ba_set_problem"):
            s.n_cams, s.n_pts = 70, 257
            s.transform(2.0)
        s.set_problem(prob, with_params=False)
        for call in (lambda: s.transform(2.0), lambda: s.align(cam_ref=np.zeros((70, 3))), lambda: s.centres()):
            with pytest.raises(hip_backend.BAHipError, match=r"-3.*ba_set_params"):
                call()
        s.set_params(prob.cams, prob.pts)
        before = s.get_params()

        def refused(code, words, call):
            with pytest.raises(hip_backend.BAHipError, match=rf"error {code}:.*{words}"):
                call()
            after = s.get_params()
            assert same_bits(after[0], before[0]) and same_bits(after[1], before[1])
        refused(-1, "scale", lambda: s.transform(0.0))
        refused(-1, "scale", lambda: s.transform(-1.0))
        refused(-1, "scale", lambda: s.transform(float("nan")))
        refused(-1, "scale", lambda: s.transform(float("inf")))
        refused(-1, "not orthogonal", lambda: s.transform(1.0, rot * (1.0 + 1e-8)))
        refused(-1, "reflection", lambda: s.transform(1.0, rot @ np.diag([1.0, 1.0, -1.0])))
        refused(-1, "t is not finite", lambda: s.transform(1.0, rot, np.array([0.0, np.nan, 0.0])))
        refused(-1, "R is not finite", lambda: s.transform(1.0, np.full((3, 3), np.inf)))
        ref = np.zeros((70, 3))
        refused(-1, "unknown loss", lambda: s.align(cam_ref=ref, loss=7))
        refused(-1, "f_scale", lambda: s.align(cam_ref=ref, f_scale=0.0))
        refused(-1, "iters", lambda: s.align(cam_ref=ref, iters=-1))
        refused(-1, "both NULL", lambda: s.align())
        refused(-1, "camera weight 4", lambda: s.align(cam_ref=ref, cam_w=np.where(np.arange(70) == 4, -1.0, 1.0)))
        refused(-1, "point weight 9", lambda: s.align(pt_ref=np.zeros((257, 3)), pt_w=np.where(np.arange(257) == 9, np.nan, 1.0)))
        with pytest.raises(ValueError, match="unknown loss"):
            s.align(cam_ref=ref, loss="tukey")
        s.set_priors(points={3: (prob.pts[3], np.eye(3))})
        refused(-3, "priors", lambda: s.transform(2.0, rot))
        refused(-3, "priors", lambda: s.align(cam_ref=sr.centres(prob.cams) * 2.0, apply=True))
        assert s.align(cam_ref=sr.centres(prob.cams) * 2.0)["status"] == 0          # estimating alone does not touch the priors
        s.set_priors()
        s.transform(2.0, rot)
        after = s.get_params()
        assert not same_bits(after[1], before[1])
        assert np.abs(after[1] - 2.0 * before[1] @ rot.T).max() <= 1e-13 * 40


# ------------------------------------------------------------------------------------------------- 6 align parity
@functools.lru_cache(maxsize=None)
def gps_scene(far):
    """The truth of make_problem(40, 300, 4, seed=5) on the handle; references for the 40 centres and the first 60 points:
    s0 = 12.5, a random rotation, |t0| ~ 3 or the UTM-like offset, 0.05 noise, 15 gross outliers of 30."""
    prob, cams_true, pts_true = make_problem(40, 300, 4, seed=5, return_truth=True)
    truth = BAProblem(cams_true, pts_true, prob.cam_idx, prob.pt_idx, prob.uv, prob.K4, 0)
    rng = np.random.default_rng(17)
    a = np.concatenate([sr.centres(cams_true), pts_true[:60]])
    R0, s0 = sr.random_rotation(rng), 12.5
    t0 = FAR if far else np.array([1.0, -2.0, 2.0])
    clean = s0 * a @ R0.T + t0
    b = clean + rng.normal(0.0, 0.05, size=a.shape)
    d = rng.normal(size=(15, 3))
    b[rng.choice(100, 15, replace=False)] += 30.0 * d / np.linalg.norm(d, axis=1, keepdims=True)
    w = np.where(rng.random(100) < 0.25, 0.0, rng.uniform(0.5, 2.0, size=100))
    return truth, a, b, clean, (s0, R0, t0), w


def reference_sets(mode, a, b, w):
    """-> (kwargs of Solver.align, the yardstick's a, b, w over [40 cameras | 300 points] or a part of it)."""
    pt_ref = np.full((300, 3), np.nan)
    pt_ref[:60] = b[40:]
    pt_w = np.zeros(300)
    pt_w[:60] = 1.0
    a_pts = np.concatenate([a[40:], np.zeros((240, 3))])
    if mode == "cameras":
        return dict(cam_ref=b[:40]), a[:40], b[:40], None
    if mode == "points":
        return dict(pt_ref=pt_ref, pt_w=pt_w), a_pts, pt_ref, pt_w
    if mode == "both":
        return dict(cam_ref=b[:40], pt_ref=pt_ref, pt_w=pt_w), np.concatenate([a[:40], a_pts]), np.concatenate([b[:40], pt_ref]), \
            np.concatenate([np.ones(40), pt_w])
    cam_ref = b[:40].copy()
    cam_ref[w[:40] == 0] = np.nan
    pt_w[:60] = w[40:]
    pt_ref[:60][w[40:] == 0] = np.nan
    return dict(cam_ref=cam_ref, cam_w=w[:40], pt_ref=pt_ref, pt_w=pt_w), np.concatenate([a[:40], a_pts]), \
        np.concatenate([cam_ref, pt_ref]), np.concatenate([w[:40], pt_w])


def compare_alignment(got, want, t_scale):
    """-> the four normalised differences (s, R, t / t_scale, errors each relative to itself or to the noise level where
    it is smaller, rms and max to themselves) after checking status, count and NaN pattern."""
    assert got["status"] == want["status"] == 0 and got["n_used"] == want["n_used"]
    err = np.concatenate([e for e in (got["cam_err"], got["pt_err"]) if e is not None])
    assert np.array_equal(np.isnan(err), np.isnan(want["err"]))
    m = ~np.isnan(err)
    d_err = max((np.abs(err[m] - want["err"][m]) / np.maximum(want["err"][m], NOISE)).max(), abs(got["rms"] - want["rms"]) / want["rms"],
                abs(got["max"] - want["max"]) / want["max"])
    return np.array([abs(got["s"] - want["s"]) / want["s"], np.abs(got["R"] - want["R"]).max(),
                     np.abs(got["t"] - want["t"]).max() / t_scale, d_err])


@pytest.mark.parametrize("mode", ["cameras", "points", "both", "weights"])
@pytest.mark.parametrize("far", [False, True], ids=["near", "utm"])
def test_align_matches_the_yardstick(far, mode):
    truth, a, b, _, (s0, R0, t0), w = gps_scene(far)
    kw, ya, yb, yw = reference_sets(mode, a, b, w)
    t_scale = max(1.0, float(np.linalg.norm(t0)))
    worst, where = np.zeros(4), [None] * 4
    with hip_backend.Solver(0) as s:
        s.set_problem(truth)
        before = s.get_params()
        for loss in sr.LOSSES:
            for with_scale in (True, False):
                for iters in (0, 10):
                    got = s.align(loss=loss, f_scale=0.15, iters=iters, with_scale=with_scale, **kw)
                    want = sr.align(ya, yb, yw, loss=loss, f_scale=0.15, iters=iters, with_scale=with_scale)
                    d = compare_alignment(got, want, t_scale)
                    for q in range(4):
                        if d[q] > worst[q]:
                            worst[q], where[q] = d[q], (loss, with_scale, iters)
        after = s.get_params()
    print(f"align parity {'utm' if far else 'near'} / {mode}: s {worst[0]:.2e} {where[0]}, R {worst[1]:.2e} {where[1]}, "
          f"t {worst[2]:.2e} {where[2]}, errors {worst[3]:.2e} {where[3]}")
    assert same_bits(after[0], before[0]) and same_bits(after[1], before[1])          # apply = 0 leaves the handle alone
    assert (worst <= 1e-10).all(), (worst, where)


# --------------------------------------------------------------------------------------------------------- 7 sizes
@pytest.mark.parametrize("n", [3, 63, 64, 65, 257, 2570])
def test_align_sizes(n):
    """Correspondence counts around a wave, a workgroup and several workgroups with a ragged tail (70 + 2500)."""
    rng = np.random.default_rng(n)
    if n == 2570:
        prob = make_problem(70, 2500, 3, seed=2)
        a = np.concatenate([sr.centres(prob.cams), prob.pts])
    else:
        prob = make_problem(3, n, 2, seed=n)
        a = prob.pts
    s0, R0, t0 = 0.8, sr.random_rotation(rng), np.array([-3.0, 1.0, 2.0])
    b = s0 * a @ R0.T + t0 + rng.normal(0.0, 0.05, size=a.shape)
    with hip_backend.Solver(0) as s:
        s.set_problem(prob)
        got = s.align(cam_ref=b[:70], pt_ref=b[70:]) if n == 2570 else s.align(pt_ref=b)
    d = compare_alignment(got, sr.align(a, b), max(1.0, float(np.linalg.norm(t0))))
    print(f"align size {n}: s {d[0]:.2e} R {d[1]:.2e} t {d[2]:.2e} errors {d[3]:.2e}")
    assert (d <= 1e-10).all()


@pytest.mark.parametrize("nn", sc.BORDER_COUNTS)
def test_align_grid_borders(nn):
    """64 and 65 partial rows; ALIGN_MAX_BLOCKS workgroups with one correspondence per thread, and one correspondence more,
    which starts the second trip of the grid-stride loops (tests/similarity_cases.py).  The last 40 correspondences weigh
    1000: test_similarity_host.py shows that without them s or t moves by more than 100 x the tolerance."""
    blocks, per_thread = sc.partial_rows(nn)
    assert (blocks, per_thread) == {sc.BORDER_COUNTS[0]: (64, 1), sc.BORDER_COUNTS[1]: (65, 1),
                                    sc.BORDER_COUNTS[2]: (hip_backend.ALIGN_MAX_BLOCKS, 1),
                                    sc.BORDER_COUNTS[3]: (hip_backend.ALIGN_MAX_BLOCKS, 2)}[nn]
    prob, a, b, w, (s0, R0, t0) = sc.border_scene(nn)
    t_scale = max(1.0, float(np.linalg.norm(t0)))
    with hip_backend.Solver(0) as s:
        s.set_problem(prob)
        for loss, iters in (("linear", 0), ("cauchy", 5)):
            kw = dict(cam_ref=b[:3], cam_w=w[:3], pt_ref=b[3:], pt_w=w[3:], loss=loss, f_scale=0.15, iters=iters)
            got, again = s.align(**kw), s.align(**kw)
            want = sr.align(a, b, w, loss=loss, f_scale=0.15, iters=iters)
            d = compare_alignment(got, want, t_scale)
            last = abs(got["pt_err"][-1] - want["err"][-1]) / max(want["err"][-1], NOISE)
            print(f"align {nn} correspondences ({blocks} partial rows, {per_thread} per thread), {loss}: s {d[0]:.2e} R {d[1]:.2e} "
                  f"t {d[2]:.2e} errors {d[3]:.2e}, the last point's {last:.2e}")
            assert got["n_used"] == nn
            assert (d <= sc.TOL).all() and last <= sc.TOL
            for key in ("R", "t", "cam_err", "pt_err"):
                assert same_bits(got[key], again[key]), key
            assert same_bits([got[k] for k in ("s", "rms", "max")], [again[k] for k in ("s", "rms", "max")])


# ---------------------------------------------------------------------------------------------------- 8 exact data
def test_exact_references_and_apply():
    truth, a, _, clean, (s0, R0, t0), _ = gps_scene(False)
    pt_ref = np.full((300, 3), np.nan)
    pt_ref[:60] = clean[40:]
    pt_w = (np.arange(300) < 60).astype(float)
    kw = dict(cam_ref=clean[:40], pt_ref=pt_ref, pt_w=pt_w, loss="huber", f_scale=0.15, iters=3)
    with hip_backend.Solver(0) as s1, hip_backend.Solver(0) as s2:
        s1.set_problem(truth)
        s2.set_problem(truth)
        r1 = s1.align(apply=True, **kw)
        ctr = s1.centres()
        p1 = s1.get_params()
        r2 = s2.align(apply=False, **kw)
        s2.transform(r2["s"], r2["R"], r2["t"])
        p2 = s2.get_params()
    err = (abs(r1["s"] - s0) / s0, np.abs(r1["R"] - R0).max(), np.abs(r1["t"] - t0).max() / max(1.0, np.linalg.norm(t0)))
    size = float(np.abs(clean - clean.mean(axis=0)).max())
    print(f"exact data: s {err[0]:.2e} R {err[1]:.2e} t {err[2]:.2e}; centres off the references by {np.abs(ctr - clean[:40]).max():.2e} "
          f"(scene size {size:.3g}); rms {r1['rms']:.2e}")
    assert max(err) <= 1e-12
    assert np.abs(ctr - clean[:40]).max() <= 1e-9 * size and r1["max"] <= 1e-9 * size
    assert r1["status"] == 0 and same_bits(r1["R"], r2["R"]) and r1["s"] == r2["s"] and same_bits(r1["t"], r2["t"])
    assert same_bits(p1[0], p2[0]) and same_bits(p1[1], p2[1])


# ---------------------------------------------------------------------------------------------------- 9 robustness
def test_huber_resists_the_outliers():
    truth, a, b, _, (s0, R0, t0), _ = gps_scene(False)
    kw, *_ = reference_sets("both", a, b, None)
    with hip_backend.Solver(0) as s:
        s.set_problem(truth)
        fits = {loss: s.align(loss=loss, f_scale=0.15, iters=10, **kw) for loss in ("linear", "huber")}
    e = {k: (abs(f["s"] - s0) / s0, np.abs(f["R"] - R0).max(), np.abs(f["t"] - t0).max()) for k, f in fits.items()}
    print("errors in s, R, t: linear " + ", ".join(f"{v:.2e}" for v in e["linear"]) + "; huber " + ", ".join(f"{v:.2e}" for v in e["huber"]))
    for q in range(3):
        assert e["huber"][q] <= 0.1 * e["linear"][q]


# ------------------------------------------------------------------------------------------------------ 10 statuses
def test_statuses():
    prob = problem("pinhole")
    rng = np.random.default_rng(8)
    turn = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    line = np.outer(np.arange(257.0), (1.0, 2.0, 3.0))
    same = np.tile((1.0, 2.0, 3.0), (257, 1))
    flat = rng.uniform(-5.0, 5.0, size=(257, 3)) * (1.0, 1.0, 0.0)
    generic = rng.uniform(-5.0, 5.0, size=(257, 3))
    R0 = sr.random_rotation(rng)
    with hip_backend.Solver(0) as s:
        s.set_problem(prob)

        def run(pts, ref, **kw):
            s.set_params(prob.cams, pts)
            before = s.get_params()
            out = s.align(pt_ref=ref, **kw)
            return out, before, s.get_params()
        two = (np.arange(257) < 2).astype(float)
        for name, (out, before, after), status in (
                ("two", run(generic, generic * 2.0, pt_w=two, apply=True), 1),
                ("collinear", run(line, 2.0 * line @ turn.T + (5.0, 6.0, 7.0), apply=True), 2),
                ("coincident", run(same, generic, apply=True), 2),
                ("nan-reference", run(generic, np.where(np.arange(257)[:, None] == 5, np.nan, generic), apply=True), 2)):
            assert out["status"] == status, name
            assert out["s"] == 1.0 and np.array_equal(out["R"], np.eye(3)) and np.array_equal(out["t"], np.zeros(3)), name
            assert np.isnan(out["pt_err"]).all() and np.isnan(out["rms"]) and np.isnan(out["max"]), name
            assert same_bits(after[0], before[0]) and same_bits(after[1], before[1]), name
        assert run(generic, generic, pt_w=two)[0]["n_used"] == 2
        out = run(flat, 2.0 * flat @ R0.T + 1.0)[0]
        assert out["status"] == 0 and abs(np.linalg.det(out["R"]) - 1.0) <= 1e-12
        assert np.abs(out["R"] - R0).max() <= 1e-10 and abs(out["s"] - 2.0) <= 2e-10
        out = run(generic, generic * (1.0, 1.0, -1.0))[0]
        want = sr.align(generic, generic * (1.0, 1.0, -1.0))
        assert out["status"] == 0 and abs(np.linalg.det(out["R"]) - 1.0) <= 1e-12 and np.abs(out["R"] - want["R"]).max() <= 1e-10
        assert abs(out["s"] - want["s"]) <= 1e-10 * want["s"]


# ----------------------------------------------------------------------------------------------- 11 reproducibility
def test_two_identical_calls_give_the_same_bits():
    prob = make_problem(70, 2500, 3, seed=2)
    rng = np.random.default_rng(3)
    a = np.concatenate([sr.centres(prob.cams), prob.pts])
    b = 3.0 * a @ sr.random_rotation(rng).T + FAR + rng.normal(0.0, 0.05, size=a.shape)
    b[::17] += 20.0
    with hip_backend.Solver(0) as s:
        s.set_problem(prob)
        r = [s.align(cam_ref=b[:70], pt_ref=b[70:], loss="cauchy", f_scale=0.15, iters=10) for _ in range(2)]
    assert r[0]["status"] == 0
    for key in ("R", "t", "cam_err", "pt_err"):
        assert same_bits(r[0][key], r[1][key]), key
    assert same_bits([r[0][k] for k in ("s", "rms", "max")], [r[1][k] for k in ("s", "rms", "max")])


# ------------------------------------------------------------------------------------------------------ 12 the loop
def test_solve_then_align_to_the_true_centres():
    """A gauge-free bal.solve drifts by a similarity; bal.align to the true centres takes it out and leaves the residuals."""
    args = (20, 2000, 9000)
    prob, _ = make_shared_bal_problem(None, *args, seed=3)
    _, cams_true, _ = make_bal_like(*args, seed=3, K4=K4, pixel_sigma=0.0, return_truth=True)
    true_centres = sr.centres(cams_true)            # (the BAL camera frame is the pinhole's turned over: same centres)
    solved, summary = bal.solve(prob, fixed_cam=-1, max_iters=30)
    drift = sr.centres(solved.cams) - true_centres
    rms_before = float(np.sqrt((drift * drift).sum(axis=1).mean()))
    want = sr.align(sr.centres(solved.cams), true_centres)
    res, aligned = bal.align(solved, cam_ref=true_centres)
    left = sr.centres(aligned.cams) - true_centres
    rms_after = float(np.sqrt((left * left).sum(axis=1).mean()))
    with hip_backend.Solver(0) as s:
        r0 = s.residuals_bal(solved)[0]
        r1 = s.residuals_bal(aligned)[0]
    print(f"loop: centre rms {rms_before:.3e} -> {rms_after:.3e} (yardstick {want['rms']:.3e}, device reports {res['rms']:.3e}); "
          f"residuals moved {np.abs(r1 - r0).max():.2e} px")
    assert res["status"] == 0 and want["status"] == 0
    assert rms_after <= want["rms"] * (1.0 + 1e-9) + 1e-12 and rms_after < rms_before
    assert abs(res["rms"] - want["rms"]) <= 1e-10 * max(1.0, want["rms"])
    assert np.array_equal(aligned.cams[:, 6:9], solved.cams[:, 6:9])
    assert np.abs(r1 - r0).max() <= 1e-9
    assert similarity.compose(similarity.inverse((res["s"], res["R"], res["t"])), (res["s"], res["R"], res["t"]))[0] == pytest.approx(1.0, abs=1e-15)
