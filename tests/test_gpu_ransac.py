"""GPU: ba_resect_ransac -- P3P hypotheses scored on the device, consensus, ba_resect's refinement on the consensus set --
against the numpy yardstick of tests/ransac_reference.py: the minimal solver alone, the outcome under uniform outliers
(which ba_resect does not survive), the edges of the hypothesis and observation mappings, planar and collinear scenes, the
masks and the caller's observation order, reproducibility, what the call leaves on the handle, the refusals, and the loop
register -> drop mismatches -> adjust."""
import ctypes as C
import functools

import numpy as np
import pytest

from bundle_adjustment_amd import bal, hip_backend
from bundle_adjustment_amd.bal import BALProblem
from bundle_adjustment_amd.problem import BAProblem
from bundle_adjustment_amd.synthetic import make_problem, make_shared_bal_problem
from bundle_adjustment_amd.triangulation import filter_observations, resect_cameras_ransac
from tests import ransac_reference as R
from tests import resect_reference as rr
from tests.resect_reference import pose_diff

pytestmark = pytest.mark.gpu
K4 = R.K4
MODELS = ["pinhole", "bal"]
THR = 4.0
FULL = -1
# observations per camera: below and at the four P3P needs, around min_inliers, the edges of a wave (64), of the lane stride
# and of the LDS tile (256), and several tiles.  Thirteen counts on twelve cameras: two assignments.
COUNTS = {"a": [FULL, 0, 3, 4, 5, 6, 7, 63, 64, 65, 255, 256], "b": [257, FULL, 256, 255, 65, 64, 63, 7, 6, 5, 4, 3]}


def upload(s, prob):
    return s._set_bal(prob) if isinstance(prob, BALProblem) else s.set_problem(prob)


def run_device(prob, **opts):
    with hip_backend.Solver(0) as s:
        return s.resect_ransac(intr=upload(s, prob), **opts)


def errors(prob, poses):
    """|r| of every observation at the given poses (n_obs,), the depths (n_obs,)."""
    e, d = np.empty(prob.n_obs), np.empty(prob.n_obs)
    for c in range(prob.n_cams):
        sel = prob.cam_idx == c
        r, _, depth = rr.obs_of(prob, c).project(poses[c])
        e[sel], d[sel] = np.sqrt((r * r).sum(axis=1)), depth
    return e, d


# ------------------------------------------------------------------------------------------------ 1 the minimal solver
@pytest.mark.parametrize("model", MODELS)
def test_p3p_alone_reproduces_every_observation(model):
    """n_hyp = 1, no local optimisation, noise-free unrounded pixels, 1e-3 px: one triple's best solution must explain every
    observation of its camera.  Up to 1 % of the (camera, seed) pairs may be void or short."""
    base, cams_true, pts_true = make_problem(8, 400, 4, K4=K4, return_truth=True)
    prob, truth = R.in_model(model, cams_true, pts_true, base.cam_idx, base.pt_idx, base.cams, pts_true,
                             np.random.default_rng(11), sigma=0.0, rounded=False)
    n = np.bincount(prob.cam_idx, minlength=8)
    good, worst = 0, 0.0
    with hip_backend.Solver(0) as s:
        intr = upload(s, prob)
        for seed in range(16):
            out = s.resect_ransac(intr=intr, n_hyp=1, lo_rounds=0, refine_iters=0, max_reproj_px=1e-3, min_inliers=0, seed=seed)
            ok = (out["status"] == R.OK) & (out["n_inliers"] == n)
            good += int(ok.sum())
            worst = max(worst, float(pose_diff(out["poses"][ok], truth[ok]).max()))
            assert np.array_equal(out["obs_inlier"].sum(), out["n_inliers"].sum())
    print(f"{model}: {good} of 128 (camera, seed) pairs reproduce every observation within 1e-3 px; worst pose against the truth {worst:.3e}")
    assert good >= 127


# ------------------------------------------------------------------------------------------------ 2 outcome under outliers
@functools.lru_cache(maxsize=None)
def outlier_case(model, share):
    """The 8-camera problem with a share of uniform outliers, its yardstick, and the reference's own RANSAC + LO against it."""
    prob, truth, planted, yard = R.outlier_problem(model, share)
    e, depth = errors(prob, yard)
    assert (np.abs(e - THR) > 1e-6).all() and (depth > 0.0).all()       # no observation sits on the threshold
    ref = R.resect_ransac(prob, n_hyp=256)
    assert (ref["status"] == R.OK).all()
    return dict(prob=prob, truth=truth, planted=planted, yard=yard, inl=e <= THR, d_ref=float(pose_diff(ref["poses"], yard).max()))


def check_outcome(out, case, label):
    prob = case["prob"]
    assert (out["status"] == R.OK).all()
    assert np.array_equal(out["obs_inlier"], case["inl"])
    assert np.array_equal(out["n_inliers"], np.bincount(prob.cam_idx[out["obs_inlier"]], minlength=prob.n_cams))
    d = pose_diff(out["poses"], case["yard"])
    print(f"{label}: d_ref {case['d_ref']:.3e}, device against the yardstick {d.max():.3e}")
    assert d.max() <= 10.0 * case["d_ref"] + 1e-12


@pytest.mark.parametrize("share", [0.3, 0.5])
@pytest.mark.parametrize("model", MODELS)
def test_outcome_under_uniform_outliers(model, share):
    case = outlier_case(model, share)
    prob = case["prob"]
    with hip_backend.Solver(0) as s:
        intr = upload(s, prob)
        out = s.resect_ransac(intr=intr, n_hyp=256)
        plain = s.resect(intr=intr, loss="huber", f_scale=2.0, max_reproj_px=THR) if share == 0.3 else None
    check_outcome(out, case, f"{model} {share}")
    assert np.array_equal(case["inl"], ~case["planted"])                     # (the consensus is the planted inliers)
    if plain is not None:                                                    # what the feature adds: ba_resect fails on every camera
        off = pose_diff(plain["poses"], case["yard"])
        print(f"{model} {share}: ba_resect (Huber) status {plain['status']}, pose off by {np.array2string(off, precision=2)}")
        assert ((plain["status"] != R.OK) | (off > 1e-2)).all()


# ------------------------------------------------------------------------------------------------ 3 edges of the mapping
@functools.lru_cache(maxsize=None)
def shapes_case(model, variant):
    """make_problem(12, 1200, 12) with observations deleted so that camera c holds COUNTS[variant][c] of them, the true points,
    no outliers; the all-observation refinement from the true pose, and the reference's own RANSAC + LO against it."""
    base, cams_true, pts_true = make_problem(12, 1200, 12, K4=K4, return_truth=True)
    rng = np.random.default_rng(17)
    keep = np.zeros(base.n_obs, dtype=bool)
    counts = []
    for c, k in enumerate(COUNTS[variant]):
        mine = np.nonzero(base.cam_idx == c)[0]
        if k == FULL:
            assert len(mine) >= 1025
            k = len(mine)
        keep[rng.choice(mine, size=k, replace=False)] = True
        counts.append(k)
    counts = np.array(counts)
    prob, truth = R.in_model(model, cams_true, pts_true, base.cam_idx[keep], base.pt_idx[keep], base.cams, pts_true, rng)
    big = np.nonzero(counts >= 6)[0]
    yard = prob.cams[:, :6].copy()
    yard[big] = R.yardstick_poses(prob, truth, np.zeros(prob.n_obs, dtype=bool), cams=big)
    ref = R.resect_ransac(prob, cams=big, n_hyp=16)
    assert (ref["status"] == R.OK).all()
    return dict(prob=prob, counts=counts, yard=yard, d_ref=float(pose_diff(ref["poses"], yard[big]).max()))


@pytest.mark.parametrize("n_hyp", [1, 63, 64, 65, 256, 257, 1000])
@pytest.mark.parametrize("variant", ["a", "b"])
@pytest.mark.parametrize("model", MODELS)
def test_status_inliers_and_poses_at_the_edges_of_the_mapping(model, variant, n_hyp):
    """n_hyp > 1: every OK camera against the yardstick.  One hypothesis is the one case whose outcome depends on the triple
    drawn: from a weak triple of a 7-observation camera the second round still refines a consensus of 6 and ends 1.4e-2
    (pinhole) and 6.5e-3 (BAL) in pose_diff from the all-observation optimum, in the reference as on the device.  There
    every OK camera is held against the reference run on the device's own camera-ordered list -- the same generator then
    draws the same triple -- in consensus and in pose, and the yardstick takes the cameras whose reference run meets it."""
    case = shapes_case(model, variant)
    prob, counts = case["prob"], case["counts"]
    with hip_backend.Solver(0) as s:
        intr = upload(s, prob)
        out = s.resect_ransac(intr=intr, n_hyp=n_hyp)
        c_orig = s.debug_layout("c_orig")
    few = counts < 4
    assert (out["status"][few] == R.FEW_POINTS).all() and np.array_equal(out["poses"][few], prob.cams[few, :6])
    assert (out["n_inliers"][few] == 0).all() and np.isnan(out["rms_px"][few]).all() and np.isnan(out["max_px"][few]).all()
    for c in np.nonzero(~few)[0]:                 # status and measures: the reference's, given the device's final pose
        m = rr.resect(rr.obs_of(prob, c), out["poses"][c], init="current", refine_iters=0, max_reproj_px=THR)
        assert out["status"][c] == m["status"] and out["n_inliers"][c] == m["n_inliers"], (c, counts[c])
        assert abs(out["rms_px"][c] - m["rms_px"]) <= 1e-9 * m["rms_px"] and abs(out["max_px"][c] - m["max_px"]) <= 1e-9 * m["max_px"]
    assert (out["status"][(counts >= 4) & (counts < 6)] == R.FEW_INLIERS).all()
    assert np.array_equal(out["n_inliers"], np.bincount(prob.cam_idx[out["obs_inlier"]], minlength=12))
    ok = out["status"] == R.OK
    assert np.array_equal(ok, counts >= 6)
    if n_hyp == 1:
        for c in np.nonzero(ok)[0]:
            rows = c_orig[prob.cam_idx[c_orig] == c]
            o = rr.Obs(prob.pts[prob.pt_idx[rows]], prob.uv[rows], K4=None if model == "bal" else K4, intr=prob.cams[c, 6:9] if model == "bal" else None)
            ref = R.ransac(o, prob.cams[c, :6], cam=c, n_hyp=1)
            dr = float(pose_diff(out["poses"][c], ref["pose"])[0])
            assert np.array_equal(out["obs_inlier"][rows], ref["inlier"]) and dr <= 10.0 * case["d_ref"] + 1e-12, (c, counts[c], dr)
            ok[c] = float(pose_diff(ref["pose"], case["yard"][c])[0]) <= 10.0 * case["d_ref"] + 1e-12
        print(f"{model} {variant} n_hyp 1: the reference run from the same triple meets the yardstick on {ok.sum()} of {(counts >= 6).sum()} cameras")
        assert ok.sum() >= 6
    d = pose_diff(out["poses"][ok], case["yard"][ok])
    print(f"{model} {variant} n_hyp {n_hyp}: d_ref {case['d_ref']:.3e}, device against the yardstick {d.max():.3e}")
    assert d.max() <= 10.0 * case["d_ref"] + 1e-12


# ------------------------------------------------------------------------------------------------ 4, 5 planar and collinear scenes
@pytest.mark.parametrize("model", MODELS)
def test_a_tilted_plane_is_no_obstacle(model):
    prob, truth, planted, yard = R.outlier_problem(model, 0.3, base=(4, 80, 4), plane=True)
    ref = R.resect_ransac(prob, n_hyp=256)
    d_ref = float(pose_diff(ref["poses"], yard).max())
    e, _ = errors(prob, yard)
    assert (np.abs(e - THR) > 1e-6).all()
    with hip_backend.Solver(0) as s:
        intr = upload(s, prob)
        out = s.resect_ransac(intr=intr, n_hyp=256)
        plain = s.resect(intr=intr, init="dlt")
    d = pose_diff(out["poses"], yard)
    print(f"{model} plane: d_ref {d_ref:.3e}, device against the yardstick {d.max():.3e}")
    assert (out["status"] == R.OK).all() and np.array_equal(out["obs_inlier"], e <= THR)
    assert d.max() <= 10.0 * d_ref + 1e-12
    assert (plain["status"] == R.DEGENERATE).all()


@pytest.mark.parametrize("model", MODELS)
def test_collinear_points_are_degenerate(model):
    base, cams_true, pts_true = make_problem(4, 80, 4, K4=K4, return_truth=True)
    line = np.arange(0, 80, 8)
    pts = pts_true.copy()
    pts[line] = np.array([0.5, -0.2, 11.0]) + np.linspace(-1.0, 1.0, len(line))[:, None] * np.array([1.0, 0.4, 0.7])
    keep = (base.cam_idx != 2) | np.isin(base.pt_idx, line)                  # camera 2 sees the line only
    prob, truth = R.in_model(model, cams_true, pts, base.cam_idx[keep], base.pt_idx[keep], base.cams, pts, np.random.default_rng(5))
    out = run_device(prob)
    assert out["status"][2] == R.DEGENERATE and np.array_equal(out["poses"][2], prob.cams[2, :6])
    assert out["n_inliers"][2] == 0 and np.isnan(out["rms_px"][2]) and np.isnan(out["max_px"][2])
    assert not out["obs_inlier"][prob.cam_idx == 2].any() and (prob.cam_idx == 2).sum() == len(line)
    assert (np.delete(out["status"], 2) == R.OK).all() and out["obs_inlier"][prob.cam_idx != 2].all()


# ------------------------------------------------------------------------------------------------ 6 masks and order
def same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)


@pytest.mark.parametrize("model", MODELS)
def test_pt_known_masks_the_moved_points_bit_for_bit(model):
    clean = outlier_case(model, 0.3)["prob"]
    known = np.arange(clean.n_pts) % 10 != 4
    moved = clean.pts.copy()
    moved[~known] += np.array([5.0, 0.0, 0.0])
    dirty = BALProblem(clean.cams, moved, clean.cam_idx, clean.pt_idx, clean.uv) if model == "bal" else \
        BAProblem(clean.cams, moved, clean.cam_idx, clean.pt_idx, clean.uv, clean.K4, 0)
    a = run_device(clean, known_points=known)
    b = run_device(dirty, known_points=known)
    c = run_device(dirty)
    idx = run_device(dirty, known_points=np.nonzero(known)[0])
    assert same(a, b) and same(a, idx)
    assert (a["status"] == R.OK).all() and not np.array_equal(a["poses"], c["poses"])
    assert not a["obs_inlier"][~known[clean.pt_idx]].any()
    assert np.array_equal(a["n_inliers"], np.bincount(clean.cam_idx[a["obs_inlier"]], minlength=clean.n_cams))
    ref_pose = R.yardstick_poses(clean, outlier_case(model, 0.3)["truth"], outlier_case(model, 0.3)["planted"] | ~known[clean.pt_idx])
    assert pose_diff(a["poses"], ref_pose).max() <= 1e-9


@pytest.mark.parametrize("model", MODELS)
def test_cam_sel_leaves_the_other_cameras_alone(model):
    prob = outlier_case(model, 0.3)["prob"]
    sel = np.array([0, 1, 0, 0, 1, 1, 0, 1], dtype=bool)
    full = run_device(prob)
    part = run_device(prob, cams=sel)
    byidx = run_device(prob, cams=[1, 4, 5, 7])
    for k in ("poses", "status", "n_inliers", "rms_px", "max_px"):
        assert np.array_equal(part[k][sel], full[k][sel]), k
    assert same(part, byidx)
    mine = sel[prob.cam_idx]
    assert np.array_equal(part["obs_inlier"][mine], full["obs_inlier"][mine]) and not part["obs_inlier"][~mine].any()
    assert np.array_equal(part["poses"][~sel], prob.cams[~sel, :6]) and (part["status"][~sel] == R.OK).all()
    assert (part["n_inliers"][~sel] == 0).all() and np.isnan(part["rms_px"][~sel]).all() and np.isnan(part["max_px"][~sel]).all()


@pytest.mark.parametrize("model", MODELS)
def test_obs_inlier_is_in_the_callers_observation_order(model):
    case = outlier_case(model, 0.3)
    prob = case["prob"]
    perm = np.random.default_rng(9).permutation(prob.n_obs)
    kw = dict(cam_idx=prob.cam_idx[perm].copy(), pt_idx=prob.pt_idx[perm].copy(), uv=prob.uv[perm].copy())
    shuffled = BALProblem(prob.cams, prob.pts, **kw) if model == "bal" else BAProblem(prob.cams, prob.pts, K4=prob.K4, fixed_cam=0, **kw)
    out = run_device(shuffled)
    assert (out["status"] == R.OK).all() and np.array_equal(out["obs_inlier"], case["inl"][perm])
    assert not np.array_equal(case["inl"][perm], case["inl"])


# ------------------------------------------------------------------------------------------------ 7 reproducibility
@pytest.mark.parametrize("model", MODELS)
def test_two_calls_give_identical_bits_and_another_seed_the_same_outcome(model):
    case = outlier_case(model, 0.3)
    prob = case["prob"]
    with hip_backend.Solver(0) as s:
        intr = upload(s, prob)
        a = s.resect_ransac(intr=intr)
        b = s.resect_ransac(intr=intr)
        lo0 = s.resect_ransac(intr=intr, lo_rounds=0)
        lo0_other = s.resect_ransac(intr=intr, lo_rounds=0, seed=12345)
        other = s.resect_ransac(intr=intr, seed=12345)
    c = run_device(prob)
    assert same(a, b) and same(a, c)
    assert not np.array_equal(lo0["poses"], lo0_other["poses"])              # (another seed draws other samples)
    check_outcome(other, case, f"{model} seed 12345")
    assert np.array_equal(other["obs_inlier"], a["obs_inlier"])


def test_resect_and_resect_ransac_interleaved_keep_their_own_state():
    """ba_resect and ba_resect_ransac go through one upload path and one staging buffer for pt_known: a ba_resect_ransac with
    another mask, another selection and other intrinsics between two identical ba_resect calls leaves the second as the
    first, bit for bit, and is itself what a fresh handle gives."""
    base, cams_true, pts_true = make_problem(6, 60, 4, K4=K4, return_truth=True)
    prob, _ = R.in_model("bal", cams_true, pts_true, base.cam_idx, base.pt_idx, base.cams, pts_true, np.random.default_rng(3))
    known_a, known_b = np.arange(60) % 3 != 0, np.arange(60) % 4 != 1
    sel_a, sel_b = np.array([1, 1, 0, 1, 1, 0], dtype=bool), np.array([0, 1, 1, 1, 0, 1], dtype=bool)
    with hip_backend.Solver(0) as s:
        intr_a = upload(s, prob)
        intr_b = intr_a * np.array([1.002, 0.9, 1.1])
        first = s.resect(intr=intr_a, cams=sel_a, known_points=known_a)
        second = s.resect_ransac(intr=intr_b, cams=sel_b, known_points=known_b, n_hyp=64)
        third = s.resect(intr=intr_a, cams=sel_a, known_points=known_a)
    with hip_backend.Solver(0) as s:
        upload(s, prob)
        fresh = s.resect_ransac(intr=intr_b, cams=sel_b, known_points=known_b, n_hyp=64)
    print(f"resect status {first['status']}, resect_ransac status {second['status']}, inliers {second['n_inliers']}")
    assert (first["status"][sel_a] == R.OK).all()        # (every selected camera sees 22 or more of the known points)
    assert same(first, third)
    assert same(second, fresh)


# ------------------------------------------------------------------------------------------------ 8 handle hygiene
SOLVE = dict(loss="huber", max_iters=6, small_solver=1)
SAME = ("final_cost", "final_sse", "iterations", "pcg_iterations", "final_lambda")


def test_write_cams_0_leaves_the_handle_as_found():
    prob = make_problem(12, 300, 4, seed=5)
    with hip_backend.Solver(0) as s:
        s.set_problem(prob)
        a = s.solve(**SOLVE)
        pa = s.get_params()
    with hip_backend.Solver(0) as s:
        s.set_problem(prob)
        before = s.get_params()
        out = s.resect_ransac(max_reproj_px=16.0)              # (the points are 0.05 off: some 4 px on top of the pixel noise)
        after = s.get_params()
        assert (out["status"] == R.OK).all() and not np.array_equal(out["poses"], before[0])
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        b = s.solve(**SOLVE)
        pb = s.get_params()
    assert np.array_equal(pa[0], pb[0]) and np.array_equal(pa[1], pb[1])
    assert all(a[k] == b[k] for k in SAME)


def test_write_cams_1_is_set_params_with_the_merged_cameras():
    prob = make_problem(12, 300, 4, seed=5)                      # (fixed_cam = 0)
    held = np.zeros((12, 6), dtype=bool)
    held[3] = True                                               # a whole camera
    held[6, 4] = True                                            # one translation component
    sel = np.arange(12) != 9
    with hip_backend.Solver(0) as s:
        s.set_problem(prob)
        s.set_held(cams=held)
        s.solve(**SOLVE)                                   # (the current parameter set is then whichever the solve ended on)
        old, pts = s.get_params()
        out = s.resect_ransac(cams=sel, write_cams=1, max_reproj_px=16.0)
        c1, p1 = s.get_params()
        take = sel & (out["status"] == R.OK) & ~held.any(axis=1) & (np.arange(12) != 0)
        assert take.sum() == 8 and (out["status"] == R.OK).all()
        assert np.array_equal(p1, pts)
        assert np.array_equal(c1[take], out["poses"][take]) and np.array_equal(c1[~take], old[~take])
        assert not np.array_equal(out["poses"][[0, 3, 6]], old[[0, 3, 6]])       # (resected, reported, not stored)
        a = s.solve(**SOLVE)
        pa = s.get_params()
    with hip_backend.Solver(0) as s:
        s.set_problem(prob)
        s.set_held(cams=held)
        s.solve(**SOLVE)
        s.set_params(c1, pts)
        b = s.solve(**SOLVE)
        pb = s.get_params()
    assert np.array_equal(pa[0], pb[0]) and np.array_equal(pa[1], pb[1])
    assert all(a[k] == b[k] for k in SAME)


# ------------------------------------------------------------------------------------------------ 9 refusals
def _raw(s, o):
    lib = hip_backend.load_library()
    rc = lib.ba_resect_ransac(s._h, None, C.byref(o), None, None, None, None, None, None, None, None)
    return rc, lib.ba_last_error().decode()


def test_refusals():
    prob = make_problem(5, 50, 3)
    with hip_backend.Solver(0) as s:
        o = s.ransac_options()
        assert (o.n_hyp, o.lo_rounds, o.seed, o.max_reproj_px, o.loss, o.refine_iters, o.f_scale, o.min_inliers, o.write_cams,
                o.max_rms_px, o.min_depth) == (256, 2, 0, 4.0, 0, 20, 1.0, 6, 0, 0.0, 0.0)
        rc, msg = _raw(s, o)
        assert rc == -3 and msg                          # BA_ERR_STATE: no problem
        s.set_problem(prob, with_params=False)
        rc, msg = _raw(s, o)
        assert rc == -3 and msg                          # ... no parameters
        s.set_params(prob.cams, prob.pts)
        before = s.get_params()
        assert _raw(s, o)[0] == 0
        for field, value in (("n_hyp", 0), ("n_hyp", 4097), ("n_hyp", -1), ("lo_rounds", -1), ("max_reproj_px", 0.0),
                             ("max_reproj_px", -1.0), ("max_reproj_px", float("nan")), ("loss", 5), ("loss", -1), ("f_scale", 0.0),
                             ("f_scale", -1.0), ("refine_iters", -1), ("min_inliers", -1)):
            o = s.ransac_options()
            setattr(o, field, value)
            rc, msg = _raw(s, o)
            assert rc == -1 and field in msg, (field, msg)   # BA_ERR_INVALID, naming the field
        o = s.ransac_options(n_hyp=4096)
        assert _raw(s, o)[0] == 0
        lib = hip_backend.load_library()
        assert lib.ba_resect_ransac(s._h, None, None, None, None, None, None, None, None, None, None) == -1
        with pytest.raises(TypeError):
            s.resect_ransac(no_such_option=1)
        with pytest.raises(ValueError):
            s.resect_ransac(loss="nope")
        # the kernel-timing slot repeats the last call
        assert s.time_kernel(hip_backend.K_RESECT_RANSAC, 2) > 0.0
        # priors: their means were set for the old poses
        s.set_priors(cams={2: (prob.cams[2], np.eye(6))})
        o = s.ransac_options(write_cams=1)
        rc, msg = _raw(s, o)
        assert rc == -3 and "priors" in msg
        assert (s.resect_ransac(max_reproj_px=16.0)["status"] == R.OK).all()     # (write_cams = 0 is no write: allowed)
        after = s.get_params()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        s.set_priors()
        assert _raw(s, o)[0] == 0


# ------------------------------------------------------------------------------------------------ 10 the loop
def test_register_drop_mismatches_adjust():
    """20 cameras / 2 000 points, BAL camera with every intrinsic free.  The reconstruction is adjusted without cameras 5-14's
    mismatches; then those cameras are registered anew against its points: 20 % of their observations are uniform pixels and
    they start 0.3 rad / 1 m off.  resect_ransac (write) -> filter_observations(obs_inlier) -> least squares, against the solve
    of the problem with the planted outliers removed from the stock start.  Measured: DESIGN.md 4k."""
    prob, _ = make_shared_bal_problem(None, 20, 2000, 9000, seed=3)
    kw = dict(fixed_cam=0, loss="linear", max_iters=100, ftol=1e-14, xtol=1e-14, gtol=0.0)
    rng = np.random.default_rng(5)
    sel = (prob.cam_idx >= 5) & (prob.cam_idx < 15)
    mine = np.nonzero(sel)[0]
    idx = rng.choice(mine, size=len(mine) // 5, replace=False)
    planted = np.zeros(prob.n_obs, dtype=bool)
    planted[idx] = True
    clean, _ = filter_observations(prob, ~planted)
    model, s0 = bal.solve(clean, **kw)
    again = BALProblem(clean.cams.copy(), clean.pts, clean.cam_idx, clean.pt_idx, clean.uv)
    again.cams[1:, 3:6] += 1e-4 * rng.normal(size=(19, 3))           # a second start next to the stock one: the minimiser's spread
    _, s0b = bal.solve(again, **kw)
    uv = prob.uv.copy()
    uv[idx] = np.stack([rng.uniform(-640.0, 640.0, len(idx)), rng.uniform(-360.0, 360.0, len(idx))], axis=1)
    dirty = BALProblem(model.cams.copy(), model.pts, prob.cam_idx, prob.pt_idx, uv)
    for c in range(5, 15):
        axis = rng.normal(size=3)
        dirty.cams[c, :3] += 0.3 * axis / np.linalg.norm(axis)
        step = rng.normal(size=3)
        dirty.cams[c, 3:6] += 1.0 * step / np.linalg.norm(step)
    out, merged = bal.resect_ransac(dirty, cams=np.arange(5, 15))
    assert (out["status"] == R.OK).all()
    assert np.array_equal(merged.cams[:5], dirty.cams[:5]) and np.array_equal(merged.cams[15:], dirty.cams[15:])
    assert np.array_equal(merged.cams[5:15, :6], out["poses"][5:15]) and np.array_equal(merged.cams[:, 6:], dirty.cams[:, 6:])
    print(f"registered poses against the adjusted ones: {pose_diff(out['poses'][5:15], model.cams[5:15, :6]).max():.3e}")
    assert np.array_equal(out["obs_inlier"][sel], ~planted[sel]) and not out["obs_inlier"][~sel].any()
    kept, old = filter_observations(merged, out["obs_inlier"] | ~sel)
    assert np.array_equal(old, np.nonzero(~planted)[0])
    _, s1 = bal.solve(kept, **kw)
    _, s2 = bal.solve(dirty, **kw)                                   # (no registration, no filter: what the loop is for)
    rmse = [float(np.sqrt(s["final_sse"] / n)) for s, n in ((s0, clean.n_obs), (s0b, clean.n_obs), (s1, kept.n_obs), (s2, dirty.n_obs))]
    print(f"rmse: stock start {rmse[0]:.9f} px ({s0['status_name']}, {s0['iterations']}), a second start {rmse[1]:.9f} px, "
          f"registered and filtered {rmse[2]:.9f} px ({s1['status_name']}, {s1['iterations']}), neither {rmse[3]:.3f} px")
    assert abs(rmse[1] - rmse[0]) <= 1e-6
    assert abs(rmse[2] - rmse[0]) <= 1e-6
    assert not abs(rmse[3] - rmse[0]) <= 1e-2


def test_pinhole_wrapper_returns_the_merged_problem():
    prob = make_problem(6, 120, 4, seed=9)
    out, merged = resect_cameras_ransac(prob, cams=[1, 2, 5], max_reproj_px=16.0)
    assert (out["status"] == R.OK).all() and out["obs_inlier"].shape == (prob.n_obs,)
    assert np.array_equal(merged.cams[[1, 2, 5]], out["poses"][[1, 2, 5]]) and np.array_equal(merged.cams[[0, 3, 4]], prob.cams[[0, 3, 4]])
    out2, same_prob = resect_cameras_ransac(prob, write=False, max_reproj_px=16.0)
    assert np.array_equal(same_prob.cams, prob.cams) and np.array_equal(out2["poses"][[1, 2, 5]], out["poses"][[1, 2, 5]])
