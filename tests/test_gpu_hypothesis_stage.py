"""GPU: WHICH hypothesis wins in ba_relative_pose, ba_homography and ba_resect_ransac -- the samples for h > 0, the scores of every
hypothesis and the one lexicographic arg-min -- against the numpy references (include/ba_hip.h: the sample is a pure function of
(seed, pair or camera, h, n); the lowest cost wins, ties go to the lower h; n_hyp is 1 .. 4096).

(a) Planted winners (tests/hypothesis_cases.py, proven on the references by tests/test_hypothesis_cases_host.py): exactly one
hypothesis h* of 0 .. limit draws an uncontaminated sample.  With lo_rounds = 0 the raw winner comes back: best_hyp == h*, the
inliers are exactly the planted set, and the raw model meets the bound its own file sets for the minimal solver (relative pose
1e-6 on the unit-norm E, homography 100 x the reference's own worst error + 1e-12 on H~, P3P 1e-3 px on every planted inlier).  With
n_hyp = h* the planted hypothesis is not drawn and the winner has fewer inliers.  ba_resect_ransac (both camera models: its
kernels are instantiated per model) has no best_hyp output: the winner shows in those measures and in the flip between n_hyp =
h* and h* + 1; its samples index the handle's camera-ordered list, which the cases' observation order equals (asserted).  h* sits at every edge of the mappings: the waves
and workgroups of the solve kernels, the hypothesis that straddles two score blocks, the 256th and the last of 4096.
(b) The running best on ordinary data (the files' outlier cases): for every hypothesis r that lowers the reference's running
minimum, n_hyp = r returns the record before it and n_hyp = r + 1 returns r.  No mismatch is tolerated; the precondition is
that the two lowest reference costs of every tested prefix differ by 1e-4 in relative terms (the solvers agree to 1e-6 and better).
(c) The tie rule: with 6 (5) noise-free matches and 4096 hypotheses the 720 (120) ordered samples recur -- every one of the 120,
and all but some 14 of the 720, which 4096 uniform draws leave drawn once -- equal samples give equal bits, and the winner must
be the first hypothesis that draws its sample; in at least 12 (16) of the 16 pairs the winner's sample is one that recurs.
(d) n_hyp = 4096 twice gives the same bits and leaves a resident problem alone."""
import numpy as np
import pytest

from bundle_adjustment_amd.hip_backend import HOMOGRAPHY_STATUS
from tests import homography_reference as HG
from tests import hypothesis_cases as HC
from tests import ransac_reference as RS
from tests import relpose_reference as RP
from tests import resect_reference as rr

pytestmark = pytest.mark.gpu

K = HC.K
RP_OK = 0
RAW = dict(lo_rounds=0, seed=HC.SEED)


@pytest.fixture(scope="module")
def solver():
    import __graft_entry__ as g
    g.build()
    from bundle_adjustment_amd import hip_backend
    with hip_backend.Solver(0) as s:
        yield s


# ---------------------------------------------------------------------------------------------------- (a) planted winners
@pytest.mark.parametrize("n_hyp", HC.call_sizes(HC.RELPOSE_PLAN))
def test_relpose_planted_winner(solver, n_hyp):
    pairs = HC.relpose_pairs()
    p1, p2, off = HC.concatenated(pairs)
    r = solver.relative_pose(K, p1, p2, off, n_hyp=n_hyp, **RAW)
    seen, worst, worst_ref = 0, 0.0, 0.0
    for i, c in enumerate(pairs):
        got = r["match_inlier"][off[i]:off[i + 1]]
        assert r["n_inliers"][i] == got.sum() and r["best_hyp"][i] < n_hyp
        what = HC.expectation(c["h_star"], c["limit"], n_hyp)
        if what == "planted":
            assert r["best_hyp"][i] == c["h_star"], (i, r["best_hyp"][i])
            assert r["status"][i] == RP_OK and np.array_equal(got, c["inlier"]) and r["n_inliers"][i] == HC.RELPOSE_I
            d = RP.E_distance(RP.essential(r["R"][i], r["t"][i]), RP.essential(c["R"], c["t"]))
            assert d <= 1e-6, (i, d)
            worst, worst_ref = max(worst, d), max(worst_ref, c["solver_error"])
        elif what == "outside":
            assert r["best_hyp"][i] != c["h_star"] and r["n_inliers"][i] < HC.RELPOSE_I and not np.array_equal(got, c["inlier"])
        seen += what is not None
    print(f"relpose n_hyp={n_hyp}: best_hyp {r['best_hyp'].tolist()}, inliers {r['n_inliers'].tolist()}; worst raw E against the truth {worst:.2e} "
          f"(the reference's solver on the same samples {worst_ref:.2e})")
    assert seen >= 1


@pytest.mark.parametrize("n_hyp", HC.call_sizes(HC.PLANE_PLAN))
def test_homography_planted_winner(solver, n_hyp):
    pairs = HC.plane_pairs()
    p1, p2, off = HC.concatenated(pairs)
    r = solver.homography(K, p1, p2, off, n_hyp=n_hyp, **RAW)
    bound = 100.0 * max(c["solver_error"] for c in pairs) + 1e-12
    seen, worst, worst_ref = 0, 0.0, 0.0
    for i, c in enumerate(pairs):
        got = r["match_inlier"][off[i]:off[i + 1]]
        assert r["n_inliers"][i] == got.sum() and r["best_hyp"][i] < n_hyp
        what = HC.expectation(c["h_star"], c["limit"], n_hyp)
        if what == "planted":
            assert r["best_hyp"][i] == c["h_star"], (i, r["best_hyp"][i])
            assert r["status"][i] in (HOMOGRAPHY_STATUS["ok"], HOMOGRAPHY_STATUS["ambiguous"])
            assert np.array_equal(got, c["inlier"]) and r["n_inliers"][i] == HC.PLANE_I
            d = HG.H_distance(HG.normalised_H(K, r["H"][i]), c["Ht"])
            assert d <= bound, (i, d, bound)
            worst, worst_ref = max(worst, d), max(worst_ref, c["solver_error"])
        elif what == "outside":
            assert r["best_hyp"][i] != c["h_star"] and r["n_inliers"][i] < HC.PLANE_I and not np.array_equal(got, c["inlier"])
        seen += what is not None
    print(f"homography n_hyp={n_hyp}: best_hyp {r['best_hyp'].tolist()}, inliers {r['n_inliers'].tolist()}; worst raw H~ against the truth {worst:.2e} "
          f"(the reference's solver on the same samples {worst_ref:.2e}, bound {bound:.2e})")
    assert seen >= 1


def _upload(solver, prob):
    """-> intr of resect_ransac (None: the pinhole problem's K4)."""
    return solver._set_bal(prob) if prob.cams.shape[1] == 9 else solver.set_problem(prob)


@pytest.mark.parametrize("n_hyp", HC.call_sizes(HC.P3P_PLAN))
@pytest.mark.parametrize("model", HC.MODELS)
def test_p3p_planted_winner(solver, model, n_hyp):
    case = HC.p3p_problem(model)
    prob = case["prob"]
    intr = _upload(solver, prob)
    assert np.array_equal(solver.debug_layout("c_orig"), np.arange(prob.n_obs))      # the generator indexes the caller's order
    out = solver.resect_ransac(intr=intr, n_hyp=n_hyp, refine_iters=0, **RAW)
    seen, worst, worst_px = 0, 0.0, 0.0
    for cam, (h_star, limit) in enumerate(case["plan"]):
        sel = prob.cam_idx == cam
        got, I = out["obs_inlier"][sel], case["inlier"][sel]
        assert out["n_inliers"][cam] == got.sum()
        what = HC.expectation(h_star, limit, n_hyp)
        if what == "planted":
            assert out["status"][cam] == RS.OK and np.array_equal(got, I) and out["n_inliers"][cam] == HC.P3P_I, (cam, out["n_inliers"][cam])
            res, _, depth = rr.obs_of(prob, cam).project(out["poses"][cam])
            e = np.linalg.norm(res[I], axis=1)
            assert (depth[I] > 0.0).all() and e.max() <= 1e-3, (cam, e.max())
            worst, worst_px = max(worst, float(rr.pose_diff(out["poses"][cam], case["truth"][cam])[0])), max(worst_px, float(e.max()))
        elif what == "outside":
            assert out["n_inliers"][cam] < HC.P3P_I and not np.array_equal(got, I)
        seen += what is not None
    print(f"P3P {model} n_hyp={n_hyp}: inliers {out['n_inliers'].tolist()}; worst raw pose against the truth {worst:.2e}, worst planted inlier {worst_px:.2e} px "
          f"(the reference's solver on the same samples {case['solver_error'].max():.2e})")
    assert seen >= 1


# ---------------------------------------------------------------------------------------------------- (b) the running best
# cameras of ransac_reference.outlier_problem(model, 0.5): seven and six records, every prefix clear by 2.7e-3 and 1.7e-3 (in the
# other cameras the first hypotheses fit nothing but their own three observations and tie)
P3P_CAM = {"pinhole": 3, "bal": 7}
PLANE_CALL_SEED = 2    # of the homography case: with seed 0 the first record is a hypothesis that fits no match, tied with others


def _prefixes(cost):
    """[(n_hyp, the reference's winner)] for n_hyp = r and r + 1 at every record r > 0; asserts the margin of each prefix."""
    rec = HC.records(cost)
    out = sorted({N for r in rec if r > 0 for N in (r, r + 1)})
    for N in out:
        assert HC.margin(cost, N) >= 1.0 + 1e-4, (N, HC.margin(cost, N))
    assert len(out) >= 6
    return rec, [(N, RS.winner(cost, N)) for N in out]


@pytest.fixture(scope="module")
def ordinary():
    """The reference's costs of the first 256 hypotheses on the files' outlier cases."""
    out = {}
    for name, planar, share in (("general", False, 0.5), ("planar", True, 0.3)):
        c = RP.outlier_case(planar, share)
        out[name] = (c, RP.hypothesis_costs(K, c["p1"], c["p2"], n_hyp=256))
    c = HG.outlier_case(0.5)
    out["plane"] = (c, HG.hypothesis_costs(K, c["p1"], c["p2"], n_hyp=256, seed=PLANE_CALL_SEED))
    for model, cam in P3P_CAM.items():
        prob = RS.outlier_problem(model, 0.5)[0]
        out[model] = (prob, RS.hypothesis_costs(rr.obs_of(prob, cam), cam=cam, n_hyp=256))
    return out


@pytest.mark.parametrize("name", ["general", "planar"])
def test_relpose_running_best(solver, ordinary, name):
    c, (cost, _, Es) = ordinary[name]
    rec, prefixes = _prefixes(cost)
    worst = 0.0
    for n_hyp, want in prefixes:
        r = solver.relative_pose(K, c["p1"], c["p2"], n_hyp=n_hyp, lo_rounds=0)
        assert r["best_hyp"][0] == want, (n_hyp, r["best_hyp"][0], want)
        if want < 0:                              # (every hypothesis of the prefix is void)
            assert not r["match_inlier"].any()
            continue
        assert np.array_equal(r["match_inlier"], HC.relpose_outcome(c["p1"], c["p2"], Es[want])), n_hyp
        worst = max(worst, RP.E_distance(RP.essential(r["R"][0], r["t"][0]), Es[want]))
    print(f"relpose {name}: records {rec}; {len(prefixes)} prefixes agree; worst raw E against the reference's on the same sample {worst:.2e}")
    assert worst <= 1e-6


def test_homography_running_best(solver, ordinary):
    c, (cost, _, Hs) = ordinary["plane"]
    rec, prefixes = _prefixes(cost)
    x1, x2 = RP.normalise(K, c["p1"]), RP.normalise(K, c["p2"])
    worst, worst_ref = 0.0, 0.0
    for n_hyp, want in prefixes:
        r = solver.homography(K, c["p1"], c["p2"], n_hyp=n_hyp, lo_rounds=0, seed=PLANE_CALL_SEED)
        assert r["best_hyp"][0] == want, (n_hyp, r["best_hyp"][0], want)
        if want < 0:                              # (every hypothesis of the prefix is void)
            assert r["status"][0] == HOMOGRAPHY_STATUS["degenerate"] and not r["match_inlier"].any()
            continue
        assert np.array_equal(r["match_inlier"], HC.plane_outcome(c["p1"], c["p2"], Hs[want])), n_hyp
        worst = max(worst, HG.H_distance(HG.normalised_H(K, r["H"][0]), Hs[want]))
        idx = list(HG.sample4(PLANE_CALL_SEED, 0, want, len(x1)))
        worst_ref = max(worst_ref, HG.H_distance(Hs[want], HG.four_point_dlt(x1[idx], x2[idx])))
    # the bound of test_gpu_homography.py, with the reference's own error measured as the distance of its two routes (closed
    # form and DLT null vector) on the same noisy samples
    bound = 100.0 * worst_ref + 1e-12
    print(f"homography: records {rec}; {len(prefixes)} prefixes agree; worst raw H~ against the reference's on the same sample {worst:.2e} "
          f"(the reference's two routes differ by {worst_ref:.2e}, bound {bound:.2e})")
    assert worst <= bound


@pytest.mark.parametrize("model", HC.MODELS)
def test_p3p_running_best(solver, ordinary, model):
    """ba_resect_ransac returns no best_hyp: the winner is the hypothesis whose reference pose the raw pose equals.  1e-6 in
    pose_diff is 1e-3 px at 700 px of focal length, the bound of the minimal solver's own test; the reference poses of any two
    hypotheses differ by 1e-4 and more (asserted)."""
    prob, (cost, _, poses) = ordinary[model]
    cam = P3P_CAM[model]
    rec, prefixes = _prefixes(cost)
    intr = _upload(solver, prob)
    c_orig = solver.debug_layout("c_orig")
    rows = np.nonzero(prob.cam_idx == cam)[0]
    assert np.array_equal(c_orig[prob.cam_idx[c_orig] == cam], rows)                      # the generator indexes the caller's order
    o = rr.obs_of(prob, cam)
    assert o.bearings()[1].all()
    ref = {h: HC.pose_of(*p) for h, p in enumerate(poses) if p is not None}
    worst = 0.0
    for n_hyp, want in prefixes:
        out = solver.resect_ransac(intr=intr, cams=[cam], n_hyp=n_hyp, lo_rounds=0, refine_iters=0)
        pose = out["poses"][cam]
        if want < 0:                              # (every hypothesis of the prefix is void)
            assert out["status"][cam] == RS.DEGENERATE and not out["obs_inlier"].any()
            continue
        others = min((float(rr.pose_diff(ref[want], ref[h])[0]) for h in ref if h < n_hyp and h != want), default=np.inf)
        assert others >= 1e-4, (n_hyp, others)
        d = float(rr.pose_diff(pose, ref[want])[0])
        assert d <= 1e-6, (n_hyp, want, d)
        assert np.array_equal(out["obs_inlier"][rows], HC.p3p_outcome(o, ref[want])), n_hyp
        worst = max(worst, d)
    print(f"P3P {model} camera {cam}: records {rec}; {len(prefixes)} prefixes agree; worst raw pose against the reference's on the same sample {worst:.2e}")


# ---------------------------------------------------------------------------------------------------- (c) the tie rule
@pytest.mark.parametrize("feature", ["relpose", "homography"])
def test_ties_go_to_the_lower_hypothesis(solver, feature):
    p1, p2, off = HC.tie_pairs(feature)
    n = int(off[1])
    sample = RP.sample5 if feature == "relpose" else HG.sample4
    call = solver.relative_pose if feature == "relpose" else solver.homography
    r = call(K, p1, p2, off, n_hyp=HC.MAX_HYP, lo_rounds=0, seed=HC.TIE_SEED, min_inliers=n)
    recurring = 0
    for i in range(HC.TIE_PAIRS):
        count = HC.recurrence(sample, HC.TIE_SEED, i, n)
        once = sum(1 for v in count.values() if v == 1)
        # the premise (tests/test_hypothesis_cases_host.py): homography -- every sample recurs; relative pose -- 4096 draws
        # over 720 ordered samples leave some 14 drawn once, at most 4 % of those that occur
        assert once <= (0.04 * len(count) if feature == "relpose" else 0), (i, once)
        best = int(r["best_hyp"][i])
        assert 0 <= best < HC.MAX_HYP and r["n_inliers"][i] == n, (i, best, r["n_inliers"][i])
        first = HC.first_with_the_same_sample(sample, HC.TIE_SEED, i, best, n)
        assert first == best, (i, best, first)
        recurring += count[sample(HC.TIE_SEED, i, best, n)] >= 2
    print(f"{feature}: best_hyp {r['best_hyp'].tolist()}; the winner's sample is drawn again in {recurring} of {HC.TIE_PAIRS} pairs")
    assert recurring >= (12 if feature == "relpose" else HC.TIE_PAIRS)       # the rule is exercised, not met by default


# ---------------------------------------------------------------------------------------------------- (d) the maximum
def test_the_maximum_is_reproducible_and_leaves_a_resident_problem_alone(solver):
    from bundle_adjustment_amd.synthetic import make_problem
    prob = make_problem(6, 200, 4, seed=3)
    solver.set_problem(prob)
    cams0, pts0 = solver.get_params()
    cost0 = solver.residuals("huber", want_vector=False)[2]
    p1, p2, off = HC.concatenated(HC.relpose_pairs())
    a = solver.relative_pose(K, p1, p2, off, n_hyp=HC.MAX_HYP, **RAW)
    b = solver.relative_pose(K, p1, p2, off, n_hyp=HC.MAX_HYP, **RAW)
    assert all(np.array_equal(a[k], b[k], equal_nan=True) for k in a) and a["best_hyp"][-1] == HC.MAX_HYP - 1
    p1, p2, off = HC.concatenated(HC.plane_pairs())
    a = solver.homography(K, p1, p2, off, n_hyp=HC.MAX_HYP, **RAW)
    b = solver.homography(K, p1, p2, off, n_hyp=HC.MAX_HYP, **RAW)
    assert all(np.array_equal(a[k], b[k], equal_nan=True) for k in a) and a["best_hyp"][-1] == HC.MAX_HYP - 1
    cams1, pts1 = solver.get_params()
    assert np.array_equal(cams0, cams1) and np.array_equal(pts0, pts1)
    assert solver.residuals("huber", want_vector=False)[2] == cost0
    for model in HC.MODELS:
        intr = _upload(solver, HC.p3p_problem(model)["prob"])
        cams0, pts0 = solver.get_params()
        a = solver.resect_ransac(intr=intr, n_hyp=HC.MAX_HYP, refine_iters=0, **RAW)
        b = solver.resect_ransac(intr=intr, n_hyp=HC.MAX_HYP, refine_iters=0, **RAW)
        assert all(np.array_equal(a[k], b[k], equal_nan=True) for k in a) and a["n_inliers"][-1] == HC.P3P_I
        cams1, pts1 = solver.get_params()
        assert np.array_equal(cams0, cams1) and np.array_equal(pts0, pts1)
