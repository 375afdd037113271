"""The planted cases of tests/hypothesis_cases.py carry what they claim, on the numpy references alone (no GPU): h* wins with
exactly the planted inliers for every n_hyp of h* + 1 .. limit, with n_hyp = h* the winner has fewer inliers, every other
hypothesis costs at least 1 % more than h*, and the reference's own minimal solver reproduces the true model from sample h* to
1e-10.  The 1 % is a condition on the inputs: h* leaves n - |I| saturated matches, a contaminated sample n - 6 or so (P3P: 390
against 397 of 400).  tests/test_gpu_hypothesis_stage.py holds the device against these cases without running the references
again."""
import numpy as np
import pytest

from tests import homography_reference as HG
from tests import hypothesis_cases as HC
from tests import ransac_reference as RS
from tests import relpose_reference as RP
from tests import resect_reference as rr


def check_plan(sample, index, n, h_star, limit, inlier):
    """The planner's promise, restated: of h = 0 .. limit (one past the end) only h* draws its whole sample inside I."""
    I = set(np.nonzero(inlier)[0].tolist())
    inside = [h for h in range(limit + 1) if set(sample(HC.SEED, index, h, n)) <= I]
    assert inside == [h_star], inside


def check_costs(cost, h_star, limit, n_inside, inliers_of, plan):
    """cost (limit,) of the reference's hypotheses; inliers_of(h) -> the reference's inlier mask at hypothesis h's model."""
    assert len(cost) == limit
    for n_hyp in [N for N in HC.call_sizes(plan) if h_star < N <= limit]:
        assert RS.winner(cost, n_hyp) == h_star, n_hyp
    others = np.delete(cost, h_star)
    ratio = float(others.min() / cost[h_star]) if len(others) else np.inf
    assert ratio >= 1.01, ratio
    if h_star > 0:
        w = RS.winner(cost, h_star)
        assert w != h_star and (0 if w < 0 else int(inliers_of(w).sum())) < n_inside
    return ratio


@pytest.mark.parametrize("index", range(len(HC.RELPOSE_PLAN)))
def test_relpose_pair_plants_exactly_one_clean_hypothesis(index):
    h_star, limit = list(HC.RELPOSE_PLAN.items())[index]
    c = HC.relpose_pair(index, h_star, limit)
    n, I = len(c["p1"]), c["inlier"]
    assert n == HC.RELPOSE_N and I.sum() == HC.RELPOSE_I and c["solver_error"] <= HC.SOLVER_TOL
    check_plan(RP.sample5, index, n, h_star, limit, I)
    fbar = 0.5 * (HC.K[0, 0] + HC.K[1, 1])
    r = RP.sampson(RP.essential(c["R"], c["t"]), RP.normalise(HC.K, c["p1"]), RP.normalise(HC.K, c["p2"])) * fbar
    assert (np.abs(r[I]) <= 1e-9).all() and (np.abs(r[~I]) > HC.FAR_PX).all()
    cost, _, Es = RP.hypothesis_costs(HC.K, c["p1"], c["p2"], pair=index, n_hyp=limit, seed=HC.SEED)
    assert RP.E_distance(Es[h_star], RP.essential(c["R"], c["t"])) <= HC.SOLVER_TOL
    assert np.array_equal(HC.relpose_outcome(c["p1"], c["p2"], Es[h_star]), I)
    ratio = check_costs(cost, h_star, limit, HC.RELPOSE_I, lambda h: HC.relpose_outcome(c["p1"], c["p2"], Es[h]), HC.RELPOSE_PLAN)
    print(f"relpose pair {index}: h* {h_star}, limit {limit}, the next hypothesis costs {ratio:.3f} x the planted one, solver error {c['solver_error']:.1e}")


@pytest.mark.parametrize("index", range(len(HC.PLANE_PLAN)))
def test_plane_pair_plants_exactly_one_clean_hypothesis(index):
    h_star, limit = list(HC.PLANE_PLAN.items())[index]
    c = HC.plane_pair(index, h_star, limit)
    n, I = len(c["p1"]), c["inlier"]
    assert n == (HC.PLANE_N_LONG if limit > 1024 else HC.PLANE_N) and I.sum() == HC.PLANE_I and c["solver_error"] <= HC.SOLVER_TOL
    check_plan(HG.sample4, index, n, h_star, limit, I)
    y = HG.hom(c["p1"]) @ (HC.K @ c["Ht"] @ np.linalg.inv(HC.K)).T
    e = np.linalg.norm(y[:, :2] / y[:, 2:] - c["p2"], axis=1)
    assert (e[I] <= 1e-9).all() and (e[~I] > HC.FAR_PX).all()
    cost, _, Hs = HG.hypothesis_costs(HC.K, c["p1"], c["p2"], pair=index, n_hyp=limit, seed=HC.SEED)
    assert HG.H_distance(Hs[h_star], c["Ht"]) <= HC.SOLVER_TOL
    assert np.array_equal(HC.plane_outcome(c["p1"], c["p2"], Hs[h_star]), I)
    ratio = check_costs(cost, h_star, limit, HC.PLANE_I, lambda h: HC.plane_outcome(c["p1"], c["p2"], Hs[h]), HC.PLANE_PLAN)
    print(f"plane pair {index}: h* {h_star}, limit {limit}, the next hypothesis costs {ratio:.3f} x the planted one, solver error {c['solver_error']:.1e}")


@pytest.mark.parametrize("cam", range(len(HC.P3P_PLAN)))
@pytest.mark.parametrize("model", HC.MODELS)
def test_p3p_camera_plants_exactly_one_clean_hypothesis(model, cam):
    case = HC.p3p_problem(model)
    prob = case["prob"]
    assert prob.cams.shape[1] == (9 if model == "bal" else 6)
    h_star, limit = case["plan"][cam]
    sel = prob.cam_idx == cam
    I = case["inlier"][sel]
    assert sel.sum() == HC.P3P_N and I.sum() == HC.P3P_I and case["solver_error"][cam] <= HC.SOLVER_TOL
    assert np.array_equal(prob.cam_idx, np.sort(prob.cam_idx)) and (np.diff(prob.pt_idx[sel]) > 0).all()     # the handle's order
    check_plan(RS.sample3, cam, HC.P3P_N, h_star, limit, I)
    o = rr.obs_of(prob, cam)
    r, _, depth = o.project(case["truth"][cam])
    e = np.linalg.norm(r, axis=1)
    assert (depth > 0.0).all() and (e[I] <= 1e-9).all() and (e[~I] > HC.FAR_PX).all() and o.bearings()[1].all()
    cost, _, poses = RS.hypothesis_costs(o, cam=cam, n_hyp=limit, seed=HC.SEED)
    assert rr.pose_diff(HC.pose_of(*poses[h_star]), case["truth"][cam])[0] <= HC.SOLVER_TOL
    assert np.array_equal(HC.p3p_outcome(o, HC.pose_of(*poses[h_star])), I)
    ratio = check_costs(cost, h_star, limit, HC.P3P_I, lambda h: HC.p3p_outcome(o, HC.pose_of(*poses[h])), HC.P3P_PLAN)
    print(f"P3P {model} camera {cam}: h* {h_star}, limit {limit}, the next hypothesis costs {ratio:.4f} x the planted one, solver error {case['solver_error'][cam]:.1e}")


def test_the_winner_of_a_prefix_is_what_the_calls_return():
    """One statement of step (4): relative_pose / homography / ransac take their winner from hypothesis_costs."""
    c = HC.relpose_pair(1, 6, 257)
    cost, _, Es = RP.hypothesis_costs(HC.K, c["p1"], c["p2"], pair=1, n_hyp=40, seed=HC.SEED)
    for n_hyp in (6, 7, 40):
        ref = RP.relative_pose(HC.K, c["p1"], c["p2"], pair=1, n_hyp=n_hyp, seed=HC.SEED, lo_rounds=0)
        assert ref["best_hyp"] == RP.winner(cost, n_hyp) and np.array_equal(ref["E_raw"], Es[ref["best_hyp"]])
    assert RP.relative_pose(HC.K, c["p1"], c["p2"], pair=1, n_hyp=7, seed=HC.SEED, lo_rounds=0)["best_hyp"] == 6
    c = HC.plane_pair(1, 63, 258)
    cost, _, Hs = HG.hypothesis_costs(HC.K, c["p1"], c["p2"], pair=1, n_hyp=70, seed=HC.SEED)
    for n_hyp in (63, 64, 70):
        ref = HG.homography(HC.K, c["p1"], c["p2"], pair=1, n_hyp=n_hyp, seed=HC.SEED, lo_rounds=0)
        assert ref["best_hyp"] == HG.winner(cost, n_hyp) and np.array_equal(ref["H_raw"], Hs[ref["best_hyp"]])
    case = HC.p3p_problem()
    o = rr.obs_of(case["prob"], 1)
    cost, _, poses = RS.hypothesis_costs(o, cam=1, n_hyp=70, seed=HC.SEED)
    for n_hyp in (63, 64, 70):
        ref = RS.ransac(o, case["prob"].cams[1, :6], cam=1, n_hyp=n_hyp, seed=HC.SEED, lo_rounds=0)
        assert ref["best_hyp"] == RS.winner(cost, n_hyp) and np.array_equal(ref["pose"], HC.pose_of(*poses[ref["best_hyp"]]))
    assert RS.ransac(o.keep(np.arange(HC.P3P_N) < 3), case["prob"].cams[1, :6])["best_hyp"] == -1            # FEW_POINTS


def test_tie_cases_draw_every_sample_again():
    """The premise of the tie test.  Homography: each of the 120 ordered samples of 4 out of 5 is drawn some 34 times, so every
    one that occurs recurs.  Relative pose: 4096 draws over the 720 ordered samples of 5 out of 6 leave 4096 exp(-4096 / 720) =
    14 of them drawn once on average; at most 4 % of the samples that occur may be such, in every pair."""
    for index in range(HC.TIE_PAIRS):
        count = HC.recurrence(HG.sample4, HC.TIE_SEED, index, 5)
        assert len(count) == 120 and min(count.values()) >= 2
        count = HC.recurrence(RP.sample5, HC.TIE_SEED, index, 6)
        once = sum(1 for v in count.values() if v == 1)
        assert len(count) >= 700 and once <= 0.04 * len(count), (index, len(count), once)
