"""Planted cases for the hypothesis stage of ba_relative_pose, ba_homography and ba_resect_ransac (include/ba_hip.h: the sample is a
pure function of (seed, pair or camera, h, n); the lowest cost wins, ties go to the lower h).  Deterministic, numpy only.

A case plants ONE uncontaminated hypothesis h* among the first `limit`: the samples of h = 0 .. limit (one past the end on
purpose) are enumerated with the reference's generator, the inlier set I is the sample of h* plus a few further indices, redrawn
until no other h of 0 .. limit has its whole sample inside I.  Matches (observations) in I are noise-free and unrounded; every
other one is a uniform mismatch, redrawn until it lies more than 6 px from the true model.  So with n_hyp in h* + 1 .. limit
the winner is h* with exactly I as inliers, and with n_hyp = h* it is some contaminated hypothesis.  A scene on which the
reference's own minimal solver does not reproduce the true model from sample h* to 1e-10 is passed over by the builders' loop
(`attempt`), so the planted winner is never an ill-conditioned sample.  tests/test_hypothesis_cases_host.py proves all of this
on the reference alone; tests/test_gpu_hypothesis_stage.py holds the device against it.

The pairs (cameras) of a feature go into one call, each at its own index with its own h*: the index term of the generator is
then pinned for h > 0 too.  Test infrastructure only."""
import functools

import numpy as np

from bundle_adjustment_amd.bal import BALProblem
from bundle_adjustment_amd.problem import BAProblem
from bundle_adjustment_amd.rotations import rvecs_to_matrices
from tests import homography_reference as HG
from tests import ransac_reference as RS
from tests import relpose_reference as RP
from tests import resect_reference as rr

K = RP.K_TEST
K4 = RS.K4
SEED = 7                       # of the calls on the planted cases
SOLVER_TOL = 1e-10             # the reference's solver on sample h* against the true model
FAR_PX = 6.0                   # a mismatch lies further than this from the true model
IMAGE_WH = (1280.0, 720.0)
MAX_HYP = 4096

# h* -> limit (the largest n_hyp the case is planned and proven for).  Relative pose: 6 straddles two waves of k_relpose_score
# (candidates 60 .. 69), 15 | 16 two workgroups of k_relpose_solve, 25 two score blocks (candidates 250 .. 259), 255 | 256 the
# 256th hypothesis, 1023 the 40th score block, 4095 the maximum.  One pair runs the reference at 4096 (8 s of numpy).
RELPOSE_PLAN = {0: 257, 6: 257, 15: 257, 16: 257, 25: 257, 26: 257, 255: 257, 256: 257, 1023: 1024, 4095: 4096}
# Homography and P3P: lane = hypothesis, 64 per wave, 256 per block.
PLANE_PLAN = {0: 4096, 63: 258, 64: 258, 255: 258, 256: 4096, 257: 258, 4095: 4096}
P3P_PLAN = PLANE_PLAN
RELPOSE_N, RELPOSE_I = 80, 14
PLANE_N, PLANE_N_LONG, PLANE_I = 80, 120, 12          # 120 matches where 4096 samples have to miss I
MODELS = ("pinhole", "bal")                           # ba_resect_ransac's kernels are instantiated per camera model
P3P_N, P3P_I = 400, 10                               # C(10, 3) / C(400, 3) x 4096 = 5 % of the draws of I clash


def call_sizes(plan):
    """The n_hyp a feature is called with: h* + 1 (the winner is the last hypothesis), h* (it is just outside), the maximum."""
    return sorted({h + 1 for h in plan} | {h for h in plan if h > 0} | {MAX_HYP})


def expectation(h_star, limit, n_hyp):
    """What a call with n_hyp says about a case: "planted" (h* wins with I), "outside" (h* is not drawn), None (nothing)."""
    if h_star < n_hyp <= limit:
        return "planted"
    return "outside" if n_hyp == h_star else None


# ------------------------------------------------------------------------------------------------------------ the planner
def plan_inliers(sample, seed, index, n, h_star, limit, size, rng):
    """I (sorted indices, `size` of them): sample(h*) plus further indices such that no other h of 0 .. limit draws inside I."""
    samples = [frozenset(sample(seed, index, h, n)) for h in range(limit + 1)]
    own = samples[h_star]
    if any(s <= own for h, s in enumerate(samples) if h != h_star):
        raise ValueError(f"hypothesis {h_star} of (seed {seed}, index {index}, n {n}) shares its sample: take another seed")
    rest = np.setdiff1d(np.arange(n), sorted(own))
    while True:
        I = own | frozenset(int(i) for i in rng.choice(rest, size - len(own), replace=False))
        if not any(s <= I for h, s in enumerate(samples) if h != h_star):
            return np.array(sorted(I))


def _rng(feature, seed, index, h_star, limit, attempt):
    return np.random.default_rng([feature, seed, index, h_star, limit, attempt])


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


# ------------------------------------------------------------------------------------------------------------ relative pose
@functools.lru_cache(maxsize=None)
def relpose_pair(index, h_star, limit, n=RELPOSE_N, size=RELPOSE_I, seed=SEED):
    """The box scene of relpose_reference, exact pixels on I, mismatches (Sampson distance > 6 px) elsewhere.  -> dict(p1, p2,
    R, t, inlier (bool), index, h_star, limit, solver_error (the reference's five-point solver on sample h* against the truth))."""
    fbar = 0.5 * (K[0, 0] + K[1, 1])
    for attempt in range(100):
        rng = _rng(0, seed, index, h_star, limit, attempt)
        p1, p2, R, t = RP.make_scene(rng, n)
        inlier = np.zeros(n, dtype=bool)
        inlier[plan_inliers(RP.sample5, seed, index, n, h_star, limit, size, rng)] = True
        E = RP.essential(R, t)
        todo = np.nonzero(~inlier)[0]
        while todo.size:
            p2[todo] = np.c_[rng.uniform(0.0, IMAGE_WH[0], todo.size), rng.uniform(0.0, IMAGE_WH[1], todo.size)]
            r = RP.sampson(E, RP.normalise(K, p1[todo]), RP.normalise(K, p2[todo])) * fbar
            todo = todo[~(np.abs(r) > FAR_PX)]
        idx = list(RP.sample5(seed, index, h_star, n))
        err = min([RP.E_distance(Eh, E) for Eh in RP.five_point(RP.normalise(K, p1[idx]), RP.normalise(K, p2[idx]))], default=np.inf)
        if err <= SOLVER_TOL:
            return _frozen(dict(p1=p1, p2=p2, R=R, t=t, inlier=inlier, index=index, h_star=h_star, limit=limit, solver_error=err))
    raise RuntimeError("no well-conditioned scene in 100 attempts")


def relpose_pairs():
    return [relpose_pair(i, h, limit) for i, (h, limit) in enumerate(RELPOSE_PLAN.items())]


# ------------------------------------------------------------------------------------------------------------ homography
@functools.lru_cache(maxsize=None)
def plane_pair(index, h_star, limit, size=PLANE_I, seed=SEED):
    """The exact plane of homography_reference, exact pixels on I, mismatches (forward transfer error > 6 px) elsewhere.
    -> dict(p1, p2, Ht (the true H~), inlier, index, h_star, limit, solver_error)."""
    n = PLANE_N_LONG if limit > 1024 else PLANE_N
    for attempt in range(100):
        rng = _rng(1, seed, index, h_star, limit, attempt)
        p1, p2, _, _, Ht = HG.plane_scene(rng, n)
        inlier = np.zeros(n, dtype=bool)
        inlier[plan_inliers(HG.sample4, seed, index, n, h_star, limit, size, rng)] = True
        Hp = K @ Ht @ np.linalg.inv(K)
        todo = np.nonzero(~inlier)[0]
        while todo.size:
            p2[todo] = np.c_[rng.uniform(0.0, IMAGE_WH[0], todo.size), rng.uniform(0.0, IMAGE_WH[1], todo.size)]
            y = HG.hom(p1[todo]) @ Hp.T
            todo = todo[~(np.linalg.norm(y[:, :2] / y[:, 2:] - p2[todo], axis=1) > FAR_PX)]
        idx = list(HG.sample4(seed, index, h_star, n))
        Hh = HG.four_point(RP.normalise(K, p1[idx]), RP.normalise(K, p2[idx]))
        err = np.inf if Hh is None else HG.H_distance(Hh, Ht)
        if err <= SOLVER_TOL:
            return _frozen(dict(p1=p1, p2=p2, Ht=Ht, inlier=inlier, index=index, h_star=h_star, limit=limit, solver_error=err))
    raise RuntimeError("no well-conditioned scene in 100 attempts")


def plane_pairs():
    return [plane_pair(i, h, limit) for i, (h, limit) in enumerate(PLANE_PLAN.items())]


def concatenated(pairs):
    """(pts1, pts2, pair_off) of one call."""
    off = np.r_[0, np.cumsum([len(p["p1"]) for p in pairs])].astype(np.int64)
    return np.concatenate([p["p1"] for p in pairs]), np.concatenate([p["p2"] for p in pairs]), off


# ------------------------------------------------------------------------------------------------------------ P3P
def pose_of(R, t):
    return np.concatenate([rr.log_map(R), t])


def same_problem(prob, uv=None, cams=None):
    """The problem with other pixels or cameras, in its own class."""
    uv, cams = prob.uv if uv is None else uv, prob.cams if cams is None else cams
    if prob.cams.shape[1] == 9:
        return BALProblem(cams, prob.pts, prob.cam_idx, prob.pt_idx, uv).validate()
    return BAProblem(cams, prob.pts, prob.cam_idx, prob.pt_idx, uv, prob.K4, 0).validate()


@functools.lru_cache(maxsize=None)
def p3p_problem(model="pinhole", n=P3P_N, size=P3P_I, seed=SEED):
    """One problem in a camera model of ransac_reference.in_model ("pinhole" or "bal"), camera c planted at list(P3P_PLAN)[c]:
    every camera sees every one of the n points (a box 8 - 16 away, cameras on an arc), observations ordered by camera, then
    point -- with so few cameras that is the handle's camera-ordered list too, so the reference's generator and the device's
    index the same observations.  Exact pixels on I, uniform pixels over the image that have a bearing and lie further than 6
    px from the true projection elsewhere; the stored poses are the truth moved by 0.05 rad / 0.3 (ba_resect_ransac does not
    read them).  -> dict(prob, truth (n_cams, 6), inlier (n_obs,), plan [(h*, limit)], solver_error (n_cams,))."""
    plan = list(P3P_PLAN.items())
    n_cams = len(plan)
    cam_idx, pt_idx = np.repeat(np.arange(n_cams), n).astype(np.int32), np.tile(np.arange(n), n_cams).astype(np.int32)
    corner = np.array([IMAGE_WH[0] / 2, IMAGE_WH[1] / 2]) if model == "bal" else np.zeros(2)     # the BAL pixels' origin
    for attempt in range(100):
        rng = _rng(2 + (model == "bal"), seed, 0, 0, 0, attempt)
        s = np.linspace(0.0, 2.0, n_cams)
        centre = np.stack([1.5 * s, 0.15 * np.sin(2.0 * s), 0.2 * (1.0 - np.cos(1.5 * s))], axis=1)
        rvec = rng.normal(0.0, 0.05, size=(n_cams, 3))
        rvec[:, 1] -= 0.08 * s
        cams_true = np.concatenate([rvec, -np.einsum("nij,nj->ni", rvecs_to_matrices(rvec), centre)], axis=1)
        pts = np.stack([rng.uniform(-2.0, 5.0, n), rng.uniform(-1.5, 1.5, n), rng.uniform(8.0, 16.0, n)], axis=1)
        start = cams_true.copy()
        start[:, :3] += 0.05 / np.sqrt(3.0)
        start[:, 3:] += 0.3 / np.sqrt(3.0)
        clean, truth = RS.in_model(model, cams_true, pts, cam_idx, pt_idx, start, pts, rng, sigma=0.0, rounded=False)
        exact = clean.uv
        uv = exact.copy()
        inlier = np.zeros(n_cams * n, dtype=bool)
        errs = []
        for c, (h_star, limit) in enumerate(plan):
            rows = np.arange(c * n, (c + 1) * n)
            inlier[c * n + plan_inliers(RS.sample3, seed, c, n, h_star, limit, size, rng)] = True
            todo = rows[~inlier[rows]]
            while todo.size:
                uv[todo] = np.c_[rng.uniform(0.0, IMAGE_WH[0], todo.size), rng.uniform(0.0, IMAGE_WH[1], todo.size)] - corner
                usable = rr.obs_of(same_problem(clean, uv), c).bearings()[1][todo - c * n]
                todo = todo[~(usable & (np.linalg.norm(uv[todo] - exact[todo], axis=1) > FAR_PX))]
            o = rr.obs_of(same_problem(clean, uv), c)
            idx = list(RS.sample3(seed, c, h_star, n))
            y = RS.unit_rays(o.bearings()[0], model == "bal")
            errs.append(min([float(rr.pose_diff(pose_of(R, t), truth[c])[0]) for R, t in RS.p3p(y[idx], pts[idx])], default=np.inf))
        if max(errs) <= SOLVER_TOL:
            return _frozen(dict(prob=same_problem(clean, uv), truth=truth, inlier=inlier, plan=plan, solver_error=np.array(errs)))
    raise RuntimeError("no well-conditioned scene in 100 attempts")


# ------------------------------------------------------------------------------------------------------------ the reference's outcome
def relpose_outcome(p1, p2, E, max_epi_px=3.0, max_depth=50.0):
    """Steps 5 and 7 at a raw winner E (lo_rounds = 0) -> match_inlier."""
    x1, x2 = RP.normalise(K, p1), RP.normalise(K, p2)
    thr = max_epi_px / (0.5 * (K[0, 0] + K[1, 1]))
    R, t, _ = RP.recover(E, x1, x2, thr, max_depth)
    return RP.inlier_set(R, t, x1, x2, thr, max_depth)[0]


def plane_outcome(p1, p2, Hn, max_px=3.0):
    """Step 6 at a raw winner H~ (lo_rounds = 0) -> match_inlier."""
    return HG.consensus(Hn, RP.normalise(K, p1), RP.normalise(K, p2), max_px / (0.5 * (K[0, 0] + K[1, 1])))[0]


def p3p_outcome(o, pose, max_reproj_px=4.0):
    """Step 6 at a raw winner (lo_rounds = 0, refine_iters = 0) -> the consensus over o's observations."""
    return RS.consensus(o, pose, max_reproj_px, 0.0)


def records(cost):
    """The hypotheses that lower the running minimum of cost."""
    out, low = [], np.inf
    for h, c in enumerate(cost):
        if c < low:
            out.append(h)
            low = c
    return out


def margin(cost, n_hyp):
    """Second-lowest over lowest cost among the first n_hyp hypotheses (inf with fewer than two that are not void)."""
    c = np.sort(np.asarray(cost)[:n_hyp])
    return float(c[1] / c[0]) if len(c) > 1 and c[1] < np.inf and c[0] > 0.0 else np.inf


# ------------------------------------------------------------------------------------------------------------ the tie rule
TIE_PAIRS, TIE_SEED = 16, 3


@functools.lru_cache(maxsize=None)
def tie_pairs(feature):
    """16 pairs of noise-free unrounded matches, as few as the call takes (relpose: 6, homography: 5): with 4096 hypotheses
    every ordered sample (720 and 120 of them) is drawn again and again, and equal ordered samples give equal bits.
    -> (pts1, pts2, pair_off)."""
    rng = np.random.default_rng(41 + (feature == "homography"))
    n = 6 if feature == "relpose" else 5
    scenes = [RP.make_scene(rng, n) if feature == "relpose" else HG.plane_scene(rng, n) for _ in range(TIE_PAIRS)]
    p1, p2 = np.concatenate([s[0] for s in scenes]), np.concatenate([s[1] for s in scenes])
    for a in (p1, p2):
        a.setflags(write=False)
    return p1, p2, n * np.arange(TIE_PAIRS + 1, dtype=np.int64)


def first_with_the_same_sample(sample, seed, index, h, n):
    """The lowest hypothesis that draws the ordered sample of h."""
    want = sample(seed, index, h, n)
    return next(g for g in range(h + 1) if sample(seed, index, g, n) == want)


def recurrence(sample, seed, index, n, n_hyp=MAX_HYP):
    """How often each ordered sample that occurs among the first n_hyp is drawn: dict sample -> count."""
    count = {}
    for h in range(n_hyp):
        s = sample(seed, index, h, n)
        count[s] = count.get(s, 0) + 1
    return count
