"""numpy restatement of ba_resect_ransac (include/ba_hip.h), one camera at a time: the yardstick of the RANSAC resection tests,
built on tests/resect_reference.py (Obs, refine, pose_diff, obs_of).

Steps as in the header: (1) n < 4 usable observations: FEW_POINTS; (2) hypothesis h draws three distinct usable observations
from the counter-based generator below; (3) P3P -- here the classical two-conic form (Fischler-Bolles / Grunert): with the
distances s_i = |P_i| and u = s_2 / s_1, v = s_3 / s_1 the three cosine-law equations leave two quadratics in v whose
coefficients are polynomials in u; their resultant is a quartic in u (np.roots), v follows from the pair's linear
combination, s_1 from the first equation, and the pose from the three camera-frame points; the device uses another
formulation (Lambda Twist); (4) MSAC score sum min(|r|^2, thr^2) of every solution over all usable observations, lowest cost
first, ties to the lower h, then the lower solution; (5) lo_rounds times: consensus at the current pose, refinement on it
(resect_reference.refine); (6) ba_resect's measures and status at the final pose.

The samples index the usable observations in the order they are handed in; the device indexes them in its own
camera-ordered list (ascending in the point within a camera), so the two draw different triples from the same generator
unless the observations are handed in in that order.  The tests that compare hypothesis by hypothesis
(tests/test_gpu_hypothesis_stage.py) do that and assert it on the handle's layout; no other test depends on which are drawn.
"""
import numpy as np

from tests import resect_reference as rr
from tests.resect_reference import DEGENERATE, FEW_INLIERS, FEW_POINTS, HIGH_ERROR, OK, BEHIND  # noqa: F401

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
AREA_TOL = 1e-6


def mix64(z):
    """The splitmix64 finaliser."""
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw(seed, cam, h, d):
    """64 bits, a pure function of (seed, camera index, hypothesis, draw number)."""
    return mix64(mix64(mix64(mix64(int(seed) + GOLDEN) + int(cam)) + int(h)) + (int(d) + 1) * GOLDEN)


def sample(seed, item, h, n, k):
    """k distinct indices in [0, n), n >= k, of hypothesis h of an item (the camera or the pair): ranges n .. n - k + 1 (index =
    high word of draw * range), each raised past the indices already taken, in ascending order of those.  A longer sample
    begins with the shorter one."""
    out = []
    for d in range(k):
        i = (draw(seed, item, h, d) * (n - d)) >> 64
        for s in sorted(out):
            if i >= s:
                i += 1
        out.append(i)
    return tuple(out)


def sample3(seed, cam, h, n):
    return sample(seed, cam, h, n, 3)


def unit_rays(xy, bal):
    """(x, y) of step 1 -> unit vectors from the camera centre towards the points (the BAL camera looks down -z)."""
    d = np.concatenate([xy, np.ones((len(xy), 1))], axis=1)
    d /= np.linalg.norm(d, axis=1)[:, None]
    return -d if bal else d


def triple_void(X):
    """Collinear or coincident: twice the triangle's area against the square of its longest side."""
    d12, d13, d23 = X[0] - X[1], X[0] - X[2], X[1] - X[2]
    ext = max(d12 @ d12, d13 @ d13, d23 @ d23)
    return not np.linalg.norm(np.cross(d12, d13)) > AREA_TOL * ext


def pose_from_depths(s, y, X):
    """R, t with s_i y_i = R X_i + t, through the two edge vectors and their cross product."""
    P = s[:, None] * y
    A = np.stack([X[0] - X[1], X[0] - X[2], np.cross(X[0] - X[1], X[0] - X[2])], axis=1)
    B = np.stack([P[0] - P[1], P[0] - P[2], np.cross(P[0] - P[1], P[0] - P[2])], axis=1)
    R = B @ np.linalg.inv(A)
    U, _, Vt = np.linalg.svd(R)                    # the nearest rotation
    R = U @ Vt
    return R, P[0] - R @ X[0]


def p3p(y, X):
    """Unit rays y (3, 3), points X (3, 3) -> list of (R, t), every distance positive."""
    if triple_void(X):
        return []
    a12, a13, a23 = ((X[0] - X[1]) ** 2).sum(), ((X[0] - X[2]) ** 2).sum(), ((X[1] - X[2]) ** 2).sum()
    b12, b13, b23 = -2.0 * (y[0] @ y[1]), -2.0 * (y[0] @ y[2]), -2.0 * (y[1] @ y[2])
    # s1^2 (1 + u^2 + b12 u) = a12, s1^2 (1 + v^2 + b13 v) = a13, s1^2 (u^2 + v^2 + b23 u v) = a23; polynomials in u, highest first
    A2, A1, A0 = np.array([-a12]), np.array([-a12 * b23, 0.0]), np.array([a23 - a12, a23 * b12, a23])
    B2, B1, B0 = np.array([a23 - a13]), np.array([-a13 * b23, a23 * b13]), np.array([-a13, 0.0, a23])
    pm, ps = np.polymul, np.polysub
    lin, con = ps(pm(A2, B1), pm(A1, B2)), ps(pm(A2, B0), pm(A0, B2))          # lin v + con = 0
    quartic = ps(pm(con, con), pm(lin, ps(pm(A1, B0), pm(A0, B1))))
    if not np.all(np.isfinite(quartic)) or quartic[0] == 0.0:
        return []
    out = []
    for u in np.roots(quartic):
        if abs(u.imag) > 1e-6 * max(1.0, abs(u.real)):
            continue
        u = u.real
        den = np.polyval(lin, u)
        if u <= 0.0 or den == 0.0:
            continue
        v = -np.polyval(con, u) / den
        q = 1.0 + u * u + b12 * u
        if v <= 0.0 or q <= 0.0:
            continue
        s1 = np.sqrt(a12 / q)
        s = np.array([s1, u * s1, v * s1])
        for _ in range(3):                         # Gauss-Newton polish of the three cosine-law equations
            f = np.array([s[0] ** 2 + s[1] ** 2 + b12 * s[0] * s[1] - a12, s[0] ** 2 + s[2] ** 2 + b13 * s[0] * s[2] - a13,
                          s[1] ** 2 + s[2] ** 2 + b23 * s[1] * s[2] - a23])
            J = np.array([[2 * s[0] + b12 * s[1], 2 * s[1] + b12 * s[0], 0.0], [2 * s[0] + b13 * s[2], 0.0, 2 * s[2] + b13 * s[0]],
                          [0.0, 2 * s[1] + b23 * s[2], 2 * s[2] + b23 * s[1]]])
            if abs(np.linalg.det(J)) < 1e-300:
                break
            s = s - np.linalg.solve(J, f)
        if not (np.all(np.isfinite(s)) and (s > 0.0).all()):
            continue
        out.append(pose_from_depths(s, y, X))
    return out


def errors_at(o, R, t):
    """|r_i|^2 through the model's own projection and the depths, at the pose (R, t)."""
    P = o.X @ R.T + t
    z = np.where(P[:, 2] != 0.0, P[:, 2], 1.0)
    if o.intr is None:
        fx, fy, cx, cy = o.K4
        r = o.uv - np.stack([P[:, 0] / z * fx + cx, P[:, 1] / z * fy + cy], axis=1)
        return (r * r).sum(axis=1), P[:, 2]
    f, k1, k2 = o.intr
    p = -P[:, :2] / z[:, None]
    n2 = (p * p).sum(axis=1)
    r = o.uv - (f * (1.0 + n2 * (k1 + k2 * n2)))[:, None] * p
    return (r * r).sum(axis=1), -P[:, 2]


def msac(o, R, t, thr, min_depth):
    e2, depth = errors_at(o, R, t)
    return float(np.where(depth > min_depth, np.minimum(e2, thr * thr), thr * thr).sum())


def consensus(o, pose, thr, min_depth):
    r, _, depth = o.project(pose)
    return (depth > min_depth) & (np.sqrt((r * r).sum(axis=1)) <= thr)


def hypothesis_costs(o, cam=0, n_hyp=256, seed=0, max_reproj_px=4.0, min_depth=0.0):
    """Steps 2 - 4 of the header over the usable observations of o (n >= 4 of them), hypothesis by hypothesis -> (cost (n_hyp,):
    the lowest MSAC cost over the hypothesis's poses, inf when it has none; slot (n_hyp,): which of p3p's poses that is, the
    first of equal ones, -1 when void; poses: that (R, t), None when void).  The winner of step 4 among the first N
    hypotheses is the first lowest of cost[:N]: `winner`."""
    xy, ok = o.bearings()
    return _costs_of_usable(o.keep(ok), xy[ok], cam, n_hyp, seed, max_reproj_px, min_depth)


def _costs_of_usable(o, xy, cam, n_hyp, seed, max_reproj_px, min_depth):
    """hypothesis_costs on observations that all have a bearing (xy)."""
    n = len(o.uv)
    y = unit_rays(xy, o.intr is not None)
    cost, slot, poses = np.full(n_hyp, np.inf), np.full(n_hyp, -1, dtype=np.int64), [None] * n_hyp
    for h in range(n_hyp):
        idx = list(sample3(seed, cam, h, n))
        for s, (R, t) in enumerate(p3p(y[idx], o.X[idx])):
            P = o.X[idx] @ R.T + t
            depth = P[:, 2] if o.intr is None else -P[:, 2]
            if not (depth > min_depth).all():
                continue
            c = msac(o, R, t, max_reproj_px, min_depth)
            if c < cost[h]:
                cost[h], slot[h], poses[h] = c, s, (R, t)
    return cost, slot, poses


def winner(cost, n_hyp=None):
    """The hypothesis step 4 takes among the first n_hyp: the lowest cost, ties to the lower h; -1 when every one is void."""
    c = np.asarray(cost)[:n_hyp]
    h = int(np.argmin(c))
    return h if c[h] < np.inf else -1


def ransac(o, current, cam=0, n_hyp=256, lo_rounds=2, seed=0, max_reproj_px=4.0, loss="linear", refine_iters=20, f_scale=1.0,
           min_inliers=6, max_rms_px=0.0, min_depth=0.0):
    """One camera: dict(pose, status, n_inliers, rms_px, max_px, inlier (bool over o's observations), best_hyp (the winning
    hypothesis, -1 when there is none))."""
    current = np.asarray(current, dtype=np.float64)
    n_all = len(o.uv)
    bad = dict(pose=current, n_inliers=0, rms_px=np.nan, max_px=np.nan, inlier=np.zeros(n_all, dtype=bool), best_hyp=-1)
    xy, ok = o.bearings()
    o, xy = o.keep(ok), xy[ok]
    n = len(o.uv)
    if n < 4:
        return dict(bad, status=FEW_POINTS)
    thr = max_reproj_px
    cost, _, poses = _costs_of_usable(o, xy, cam, n_hyp, seed, thr, min_depth)
    best_hyp = winner(cost)
    if best_hyp < 0:
        return dict(bad, status=DEGENERATE)
    best = poses[best_hyp]
    pose = np.concatenate([rr.log_map(best[0]), best[1]])
    degenerate = False
    for _ in range(lo_rounds):
        cons = consensus(o, pose, thr, min_depth)
        if not cons.any():
            break
        pose, _, degenerate = rr.refine(o.keep(cons), pose, loss, f_scale, refine_iters, min_depth)
        if degenerate:
            break
    m = rr.resect(o, pose, init="current", refine_iters=0, min_inliers=min_inliers, max_reproj_px=thr, max_rms_px=max_rms_px,
                  min_depth=min_depth)
    inl = np.zeros(n_all, dtype=bool)
    inl[np.nonzero(ok)[0]] = consensus(o, pose, thr, min_depth)
    status = DEGENERATE if degenerate else m["status"]
    return dict(pose=pose, status=status, n_inliers=m["n_inliers"], rms_px=m["rms_px"], max_px=m["max_px"], inlier=inl, best_hyp=best_hyp)


def resect_ransac(prob, cams=None, known=None, **opts):
    """Every camera (or the listed ones) of a problem: ba_resect's arrays plus obs_inlier (n_obs,) in the problem's order."""
    cs = list(range(prob.n_cams)) if cams is None else list(cams)
    obs_inlier = np.zeros(prob.n_obs, dtype=bool)
    res = []
    for c in cs:
        sel = prob.cam_idx == c
        if known is not None:
            sel &= np.asarray(known, dtype=bool)[prob.pt_idx]
        r = ransac(rr.obs_of(prob, c, known), prob.cams[c, :6], cam=c, **opts)
        obs_inlier[np.nonzero(sel)[0]] = r["inlier"]
        res.append(r)
    return dict(poses=np.array([r["pose"] for r in res]).reshape(-1, 6), status=np.array([r["status"] for r in res], dtype=np.uint8),
                n_inliers=np.array([r["n_inliers"] for r in res], dtype=np.int32), rms_px=np.array([r["rms_px"] for r in res]),
                max_px=np.array([r["max_px"] for r in res]), obs_inlier=obs_inlier)


# ------------------------------------------------------------------------------------------------ fixtures of the tests
K4 = np.array([700.0, 700.0, 640.0, 360.0])
IMAGE_WH = (1280.0, 720.0)


def in_model(model, cams_true, pts_true, cam_idx, pt_idx, cams_start, pts_start, rng, sigma=0.5, rounded=True):
    """The problem in a camera model ("pinhole": K4; "bal": the same poses looking down -z with f = 700 (1 +- 2 %),
    k1 = -0.03 +- 0.01, k2 = +- 0.003): pixels = the truth projected + N(0, sigma), rounded to float32 unless told otherwise.
    -> (problem, true poses)."""
    from bundle_adjustment_amd.bal import BALProblem, from_pinhole
    from bundle_adjustment_amd.problem import BAProblem
    from bundle_adjustment_amd.synthetic import _project, bal_project
    if model == "bal":
        zero = np.zeros((len(cam_idx), 2))
        truth = from_pinhole(BAProblem(cams_true, pts_true, cam_idx, pt_idx, zero, K4, 0)).cams
        start = from_pinhole(BAProblem(cams_start, pts_true, cam_idx, pt_idx, zero, K4, 0)).cams
        n = len(truth)
        truth[:, 6] = 700.0 * (1.0 + 0.02 * rng.normal(size=n))
        truth[:, 7] = -0.03 + 0.01 * rng.normal(size=n)
        truth[:, 8] = 0.003 * rng.choice([-1.0, 1.0], size=n)
        start[:, 6:] = truth[:, 6:]
        uv = bal_project(truth, pts_true, cam_idx, pt_idx)
    else:
        truth, start = cams_true, cams_start
        uv = _project(cams_true, pts_true, cam_idx, pt_idx, K4)[0]
    if sigma > 0.0:
        uv = uv + rng.normal(0.0, sigma, size=uv.shape)
    if rounded:
        uv = uv.astype(np.float32).astype(np.float64)
    if model == "bal":
        return BALProblem(start.copy(), pts_start.copy(), cam_idx, pt_idx, uv).validate(), truth[:, :6].copy()
    return BAProblem(start.copy(), pts_start.copy(), cam_idx, pt_idx, uv, K4.copy(), 0).validate(), truth[:, :6].copy()


def plant_outliers(prob, share, rng):
    """Replace a share of the pixels by uniform draws over the 1280 x 720 image (mismatches; the BAL camera's pixels have
    their origin at the image centre), in place.  -> bool (n_obs,): planted."""
    n = int(round(share * prob.n_obs))
    idx = rng.choice(prob.n_obs, size=n, replace=False)
    uv = np.stack([rng.uniform(0.0, IMAGE_WH[0], n), rng.uniform(0.0, IMAGE_WH[1], n)], axis=1)
    if prob.cams.shape[1] == 9:
        uv -= np.array([IMAGE_WH[0] / 2, IMAGE_WH[1] / 2])
    prob.uv[idx] = uv
    planted = np.zeros(prob.n_obs, dtype=bool)
    planted[idx] = True
    return planted


def yardstick_poses(prob, truth, planted, cams=None):
    """The refinement from the true pose over the observations that were not planted, per camera."""
    cs = range(prob.n_cams) if cams is None else cams
    out = []
    for c in cs:
        o = rr.obs_of(prob, c)
        keep = ~planted[prob.cam_idx == c]
        out.append(rr.refine(o.keep(keep), truth[c])[0])
    return np.array(out)


def outlier_problem(model, share, seed=31, base=(8, 400, 4), plane=False):
    """make_problem(*base) with the true points, 0.5 px noise and a share of uniform outliers.
    -> (problem, true poses, planted (n_obs,), yardstick poses).  plane: the points put on z = 12 + 0.1 x."""
    from bundle_adjustment_amd.synthetic import make_problem
    b, cams_true, pts_true = make_problem(*base, K4=K4, return_truth=True)
    if plane:
        pts_true = pts_true.copy()
        pts_true[:, 2] = 12.0 + 0.1 * pts_true[:, 0]
    rng = np.random.default_rng(seed)
    prob, truth = in_model(model, cams_true, pts_true, b.cam_idx, b.pt_idx, b.cams, pts_true, rng)
    planted = plant_outliers(prob, share, rng)
    return prob, truth, planted, yardstick_poses(prob, truth, planted)
