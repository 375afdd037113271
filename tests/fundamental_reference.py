"""Yardstick of the fundamental-matrix tests: ba_fundamental restated in numpy (include/ba_hip.h, steps 0 - 6).  Where the
header's route could share a bug with the library another one is taken: the null space of the 7 x 9 system comes from LAPACK's
SVD (not from the pivoted elimination), the cubic from interpolating det at four values of a and numpy.roots (not from adjugates
and bisection), the canonical SVD from LAPACK (not from the library's Jacobi), and the Jacobian of the refinement from the seven
explicit 3 x 3 derivatives of F~ (not from the per-match cross products).  The generator, the Hartley normalisation, the MSAC
scoring of the Sampson distance in centred pixels, the chart, the damping and the acceptance rules are the header's.  Scenes on
top of tests/relpose_reference.py and tests/homography_reference.py.  Test infrastructure only."""
import functools

import numpy as np

from tests import homography_reference as HG
from tests import relpose_reference as RP
from tests.ransac_reference import sample, winner  # noqa: F401

OK, FEW_MATCHES, DEGENERATE, FEW_INLIERS = range(4)
K_TEST = RP.K_TEST
RANK_TOL = 1e-12      # the seventh singular value against the first: the header's pivot rule, restated for the SVD
MIN_SET = 8


# ------------------------------------------------------------------------------------------------------------ generator
def sample7(seed, pair, h, n):
    return sample(seed, pair, h, n, 7)


# ------------------------------------------------------------------------------------------------------------ geometry
hom = HG.hom


def unit_signed(v):
    """Unit norm, the largest-magnitude entry positive (the first of equal ones)."""
    v = np.asarray(v, dtype=np.float64)
    flat = v.ravel()
    k = int(np.argmax(np.abs(flat)))
    return v * ((-1.0 if flat[k] < 0.0 else 1.0) / np.linalg.norm(flat))


def F_distance(Fa, Fb):
    """The largest entry difference of two pixel matrices at unit Frobenius norm, the sign taken out."""
    Fa, Fb = Fa / np.linalg.norm(Fa), Fb / np.linalg.norm(Fb)
    return float(min(np.abs(Fa - Fb).max(), np.abs(Fa + Fb).max()))


def true_F(R, t, K1=K_TEST, K2=None):
    """The pixel F of x2 ~ K2 (R x1 + t): K2^-T [t]x R K1^-1 (p2^T F p1 = 0), unit norm and signed."""
    K2 = K1 if K2 is None else K2
    return unit_signed(np.linalg.inv(K2).T @ RP.skew(t) @ R @ np.linalg.inv(K1))


def hartley(p):
    """Step 1 for one image -> (c (2,), s), or None when the mean distance from the centroid is zero or not finite."""
    c = p.mean(axis=0)
    m = np.linalg.norm(p - c, axis=1).mean()
    if not (m > 0.0 and np.isfinite(m)):
        return None
    return c, np.sqrt(2.0) / m


def centred(Fn, s1, s2):
    """F_c = S2 F~ S1."""
    return np.diag([s2, s2, 1.0]) @ Fn @ np.diag([s1, s1, 1.0])


def _shift(c):
    return np.array([[1.0, 0.0, -c[0]], [0.0, 1.0, -c[1]], [0.0, 0.0, 1.0]])


def pixel_F(Fc, c1, c2):
    """T2^T F_c T1, unit norm and signed."""
    return unit_signed(_shift(c2).T @ Fc @ _shift(c1))


def normalised_F(F, c1, s1, c2, s2):
    """The pixel F back in normalised coordinates, at unit norm."""
    Fc = np.linalg.inv(_shift(c2)).T @ F @ np.linalg.inv(_shift(c1))
    Fn = np.diag([1.0 / s2, 1.0 / s2, 1.0]) @ Fc @ np.diag([1.0 / s1, 1.0 / s1, 1.0])
    return Fn / np.linalg.norm(Fn)


def sampson2(Fc, q1, q2):
    """Squared Sampson distance per match in the units of q; NaN where the denominator is zero."""
    return RP.sampson(Fc, q1, q2) ** 2


def msac(Fc, q1, q2, thr):
    return RP.msac(Fc, q1, q2, thr)


def consensus(Fc, q1, q2, thr):
    d2 = sampson2(Fc, q1, q2)
    with np.errstate(invalid="ignore"):
        return d2 <= thr * thr, d2


# ------------------------------------------------------------------------------------------------------------ seven points
def seven_point(x1, x2):
    """Step 2 on normalised points (7, 2) by the other route -> the list of F~ at unit norm by ascending root; [] for a void
    sample (rank below 7)."""
    A = np.array([np.kron(np.r_[b, 1.0], np.r_[a, 1.0]) for a, b in zip(x1, x2)])
    if not np.isfinite(A).all():
        return []
    _, s, Vt = np.linalg.svd(A)
    if not s[6] > RANK_TOL * s[0]:
        return []
    F1, F2 = Vt[7].reshape(3, 3), Vt[8].reshape(3, 3)
    nodes = np.array([-1.0, 0.0, 1.0, 2.0])
    dets = np.array([np.linalg.det(a * F1 + (1.0 - a) * F2) for a in nodes])
    coef = np.linalg.solve(np.vander(nodes, 4), dets)
    roots = np.roots(coef)
    out = []
    for a in sorted(float(r.real) for r in roots if np.isreal(r)):
        F = a * F1 + (1.0 - a) * F2
        nrm = np.linalg.norm(F)
        if np.isfinite(nrm) and nrm > 0.0:
            out.append(F / nrm)
    return out


# ------------------------------------------------------------------------------------------------------------ refinement
def canon_svd(Fn):
    """F~ = U diag(d) V^T by LAPACK, the third columns the cross products of the first two (det U = det V = +1) -> U, V, d2 / d1."""
    U, d, Vt = np.linalg.svd(Fn)
    V = Vt.T.copy()
    U[:, 2] = np.cross(U[:, 0], U[:, 1])
    V[:, 2] = np.cross(V[:, 0], V[:, 1])
    return U, V, d[1] / d[0]


def compose(U, V, sg):
    F = U @ np.diag([1.0, sg, 0.0]) @ V.T
    return F / np.linalg.norm(F)


def _derivatives(U, V, sg):
    """dF~ of U diag(1, sg, 0) V^T for U <- U exp([a]x), V <- V exp([b]x), sg <- sg + ds: seven 3 x 3 matrices."""
    S = np.diag([1.0, sg, 0.0])
    out = []
    for k in range(3):
        out.append(U @ RP.skew(np.eye(3)[k]) @ S @ V.T)
    for k in range(3):
        out.append(U @ S @ RP.skew(np.eye(3)[k]).T @ V.T)
    out.append(np.outer(U[:, 1], V[:, 1]))
    return out


def residual_jacobian(U, V, sg, q1, q2, s1, s2):
    """The signed Sampson distances r (m,) in centred pixels at U diag(1, sg, 0) V^T and their Jacobian (m, 7); matches with a
    zero denominator are left out."""
    S1, S2 = np.diag([s1, s1, 1.0]), np.diag([s2, s2, 1.0])
    Fc = S2 @ U @ np.diag([1.0, sg, 0.0]) @ V.T @ S1
    h1, h2 = hom(q1), hom(q2)
    l, m = h1 @ Fc.T, h2 @ Fc
    den = l[:, 0] ** 2 + l[:, 1] ** 2 + m[:, 0] ** 2 + m[:, 1] ** 2
    keep = den > 0.0
    h1, h2, l, m, den = h1[keep], h2[keep], l[keep], m[keep], den[keep]
    num = (h2 * l).sum(axis=1)
    r = num / np.sqrt(den)
    J = np.empty((len(r), 7))
    for k, dF in enumerate(_derivatives(U, V, sg)):
        dFc = S2 @ dF @ S1
        dl, dm = h1 @ dFc.T, h2 @ dFc
        dnum = (h2 * dl).sum(axis=1)
        J[:, k] = dnum / np.sqrt(den) - r / den * (l[:, 0] * dl[:, 0] + l[:, 1] * dl[:, 1] + m[:, 0] * dm[:, 0] + m[:, 1] * dm[:, 1])
    return r, J


def refine(Fn, q1, q2, s1, s2, iters=20):
    """Step 4's refinement on 0.5 sum r^2 over the given matches, ba_resect's step (3) in the seven local parameters -> (F~, ok)."""
    U, V, sg = canon_svd(Fn)
    if not (np.isfinite(U).all() and np.isfinite(V).all() and np.isfinite(sg)):
        return Fn, False
    lam, first, small, it = 1e-4, True, False, 0
    trial = (U, V, sg)
    cur = cost = A = g = None
    while True:
        r, J = residual_jacobian(*trial, q1, q2, s1, s2)
        c = 0.5 * float(r @ r)
        if first or c <= cost * (1.0 + 1e-12):
            cost, A, g, cur = c, J.T @ J, J.T @ r, trial
            if not first:
                lam = max(0.1 * lam, 1e-12)
        else:
            lam *= 10.0
        first = False
        if small or it >= iters:
            break
        it += 1
        try:
            L = np.linalg.cholesky(A + lam * np.diag(np.diag(A)))
        except np.linalg.LinAlgError:
            return compose(*cur), False
        dx = -np.linalg.solve(L.T, np.linalg.solve(L, g))
        if not np.isfinite(dx).all():
            return compose(*cur), False
        trial = (cur[0] @ RP.exp_so3(dx[0:3]), cur[1] @ RP.exp_so3(dx[3:6]), cur[2] + dx[6])
        small = np.linalg.norm(dx) <= 1e-14
    return compose(*cur), True


# ------------------------------------------------------------------------------------------------------------ the call
def hypothesis_costs(p1, p2, pair=0, n_hyp=1024, seed=0, max_epi_px=3.0):
    """Steps 1 - 3 of the header, hypothesis by hypothesis -> (cost (n_hyp,): the lowest MSAC cost over the hypothesis's
    solutions, inf when it has none; F: that F~, None when void).  The winner of step 3 among the first N hypotheses is
    winner(cost, N).  None when step 1 fails."""
    n1, n2 = hartley(p1), hartley(p2)
    if n1 is None or n2 is None:
        return None
    (c1, s1), (c2, s2) = n1, n2
    q1, q2 = p1 - c1, p2 - c2
    x1, x2 = s1 * q1, s2 * q2
    cost, Fs = np.full(n_hyp, np.inf), [None] * n_hyp
    for h in range(n_hyp):
        idx = list(sample7(seed, pair, h, len(p1)))
        for Fn in seven_point(x1[idx], x2[idx]):
            c = msac(centred(Fn, s1, s2), q1, q2, max_epi_px)
            if c < cost[h]:
                cost[h], Fs[h] = c, Fn
    return cost, Fs


def epipoles(Fn, c1, s1, c2, s2):
    U, V, _ = canon_svd(Fn)
    e1 = np.array([V[0, 2] / s1 + c1[0] * V[2, 2], V[1, 2] / s1 + c1[1] * V[2, 2], V[2, 2]])
    e2 = np.array([U[0, 2] / s2 + c2[0] * U[2, 2], U[1, 2] / s2 + c2[1] * U[2, 2], U[2, 2]])
    return unit_signed(e1), unit_signed(e2)


def fundamental(p1, p2, pair=0, n_hyp=1024, lo_rounds=2, seed=0, max_epi_px=3.0, refine_iters=20, min_inliers=16):
    """One pair (its index in the call: `pair`), steps 0 - 6 of the header.  Fn is F~ (normalised coordinates), F the pixel one."""
    p1, p2 = np.asarray(p1, dtype=np.float64), np.asarray(p2, dtype=np.float64)
    n = len(p1)
    out = dict(F=np.zeros((3, 3)), Fn=None, status=OK, n_inliers=0, rms_px=float("nan"), best_hyp=-1, match_inlier=np.zeros(n, dtype=bool),
               epipole1=np.zeros(3), epipole2=np.zeros(3), F_raw=None, cost=None)
    if n < 8:
        out["status"] = FEW_MATCHES
        return out
    hc = hypothesis_costs(p1, p2, pair, n_hyp, seed, max_epi_px)
    if hc is None:
        out["status"] = DEGENERATE
        return out
    cost, Fs = hc
    out["cost"] = cost
    h = winner(cost)
    if h < 0 or Fs[h] is None:
        out["status"] = DEGENERATE
        return out
    (c1, s1), (c2, s2) = hartley(p1), hartley(p2)
    q1, q2 = p1 - c1, p2 - c2
    Fn = Fs[h]
    out["best_hyp"], out["F_raw"] = h, pixel_F(centred(Fn, s1, s2), c1, c2)
    status = OK
    for _ in range(lo_rounds):
        cons, _ = consensus(centred(Fn, s1, s2), q1, q2, max_epi_px)
        if cons.sum() < MIN_SET:
            break
        Fn, ok = refine(Fn, q1[cons], q2[cons], s1, s2, refine_iters)
        if not ok:
            status = DEGENERATE
            break
    Fc = centred(Fn, s1, s2)
    inl, d2 = consensus(Fc, q1, q2, max_epi_px)
    out.update(Fn=Fn, F=pixel_F(Fc, c1, c2), match_inlier=inl, n_inliers=int(inl.sum()))
    out["epipole1"], out["epipole2"] = epipoles(Fn, c1, s1, c2, s2)
    if inl.any():
        out["rms_px"] = float(np.sqrt(d2[inl].mean()))
    if status == OK and out["n_inliers"] < min_inliers:
        status = FEW_INLIERS
    out["status"] = status
    return out


def tie_set(cost, n_hyp=None, rel=1e-9):
    """The hypotheses among the first n_hyp whose cost lies within `rel` relative of the lowest.  More than one: a near-tie, the
    arg-min is decided by rounding and is not pinned."""
    c = np.asarray(cost[:n_hyp], dtype=np.float64)
    return np.nonzero(c - c.min() <= rel * c)[0] if np.isfinite(c.min()) else np.zeros(0, dtype=np.int64)


def same_sample(ties, pair, n, seed=0):
    """Every hypothesis of `ties` drew the same seven matches, in whatever order: the same F~ up to rounding.  Such a near-tie
    is structural -- a pair of 8 matches has 8 distinct samples, one of 9 has 36, and n_hyp of them are drawn -- and no choice
    of scene cures it."""
    return len({tuple(sorted(sample7(seed, pair, int(h), n))) for h in ties}) == 1


# ------------------------------------------------------------------------------------------------------------ scenes
def yardstick(p1, p2, F, rounds=3):
    """The refinement of step 4 from the pixel F given (the truth) on the given matches (the true inliers), repeated: the
    minimum the library should reach.  -> the pixel F."""
    (c1, s1), (c2, s2) = hartley(p1), hartley(p2)
    Fn = normalised_F(F, c1, s1, c2, s2)
    for _ in range(rounds):
        Fn, ok = refine(Fn, p1 - c1, p2 - c2, s1, s2, 20)
        assert ok
    return pixel_F(centred(Fn, s1, s2), c1, c2)


def exact_scenes(count=8, n=12, seed=21):
    """`count` box scenes of n exact matches -> [(p1, p2, F true)]."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        p1, p2, R, t = RP.make_scene(rng, n)
        out.append((p1, p2, true_F(R, t)))
    return out


OUTLIER_CASES = ((0.3, 256, 0), (0.5, 2048, 0))       # (share of mismatches, n_hyp, seed)


@functools.lru_cache(maxsize=None)
def outlier_case(share, n_hyp, seed=0):
    """relpose_reference's box scene with planted mismatches (each more than 6 px, Sampson, from the true geometry) -> dict(p1, p2,
    planted, F_true, yard (pixel F), ref (the reference's own call), d_ref (its distance to the yardstick))."""
    c = RP.outlier_case(False, share)
    p1, p2, planted = c["p1"], c["p2"], c["planted"]
    Ft = true_F(c["R"], c["t"])
    yard = yardstick(p1[~planted], p2[~planted], Ft)
    ref = fundamental(p1, p2, n_hyp=n_hyp, seed=seed)
    return dict(p1=p1, p2=p2, planted=planted, F_true=Ft, yard=yard, ref=ref, d_ref=F_distance(ref["F"], yard))


COUNTS = (0, 7, 8, 9, 0, 255, 256, 0, 257, 0, 1100)      # eleven pairs, empty ones between
EDGE_N_HYP = (1, 85, 86, 255, 256, 257, 1000)
EDGE_SEED0 = 300                                          # pair i is noisy_scene(COUNTS[i], seed=EDGE_SEED0 + i, sigma=0.02)


@functools.lru_cache(maxsize=None)
def edge_pairs():
    """The pairs of the edge test: box scenes with 0.02 px of noise, so that one sample explains every match.  -> (pairs
    [(p1, p2, F true)], yard [pixel F or None], d_ref [float or None], cost [the reference's hypothesis costs up to the largest
    n_hyp, or None])."""
    pairs, yard, d_ref, cost = [], [], [], []
    for i, n in enumerate(COUNTS):
        p1, p2, R, t = RP.noisy_scene(n, seed=EDGE_SEED0 + i, sigma=0.02)
        pairs.append((p1, p2, true_F(R, t)))
        if n < 8:
            yard.append(None), d_ref.append(None), cost.append(None)
            continue
        yard.append(yardstick(p1, p2, pairs[-1][2]))
        ref = fundamental(p1, p2, pair=i, n_hyp=max(EDGE_N_HYP), min_inliers=8)
        assert ref["status"] == OK and ref["n_inliers"] == n
        d_ref.append(F_distance(ref["F"], yard[-1]))
        cost.append(ref["cost"])
    return pairs, yard, d_ref, cost


def line_case(n=20, seed=3):
    """Matches whose first-image points lie on one line: every 7 x 9 system has rank at most 6."""
    rng = np.random.default_rng(seed)
    u = np.sort(rng.uniform(0.0, 1.0, n))
    p1 = np.c_[100.0 + 1000.0 * u, 80.0 + 520.0 * u]
    p2 = np.c_[rng.uniform(0.0, 1280.0, n), rng.uniform(0.0, 720.0, n)]
    return p1, p2


def point_case(n=20, seed=4):
    """Matches at one pixel in the second image: step 1's mean distance is zero."""
    rng = np.random.default_rng(seed)
    p1 = np.c_[rng.uniform(0.0, 1280.0, n), rng.uniform(0.0, 720.0, n)]
    return p1, np.tile(np.array([[640.0, 360.0]]), (n, 1))
