"""Yardstick of the relative-pose tests: ba_relative_pose restated in numpy (include/ba_hip.h, steps 0 - 7), with another
minimal solver -- the five-point problem by the action-matrix route (Stewenius, Engels, Nister 2006: Gauss-Jordan of the ten
cubic constraints in graded order, eigenvectors of the 10 x 10 multiplication matrix by numpy.linalg.eig) instead of the
library's polynomial route -- and LAPACK's SVD instead of the library's Jacobi.  The generator, the Sampson / MSAC scoring, the
candidate poses and their votes, the local optimisation (same parametrisation, same damping and acceptance rules) and the
measures are the header's.  Scene builders for the tests.  Test infrastructure only."""
import functools

import numpy as np

from tests.ransac_reference import sample, winner

OK, FEW_MATCHES, DEGENERATE, BEHIND, FEW_INLIERS, LOW_PARALLAX = range(6)
W = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])


# ------------------------------------------------------------------------------------------------------------ generator
def sample5(seed, pair, h, n):
    return sample(seed, pair, h, n, 5)


# ------------------------------------------------------------------------------------------------------------ geometry
def normalise(K, p):
    return np.stack([(p[:, 0] - K[0, 2]) / K[0, 0], (p[:, 1] - K[1, 2]) / K[1, 1]], axis=1)


def skew(t):
    return np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])


def essential(R, t):
    return skew(t) @ R


def exp_so3(w):
    th = float(np.linalg.norm(w))
    Kx = skew(w)
    if th < 1e-8:
        return np.eye(3) + (1.0 - th * th / 6.0) * Kx + (0.5 - th * th / 24.0) * Kx @ Kx
    return np.eye(3) + np.sin(th) / th * Kx + (1.0 - np.cos(th)) / (th * th) * Kx @ Kx


def unit_E(E):
    return E / np.linalg.norm(E)


def E_distance(Ea, Eb):
    """Distance of two essential matrices of unit Frobenius norm, up to sign."""
    Ea, Eb = unit_E(Ea), unit_E(Eb)
    return float(min(np.abs(Ea - Eb).max(), np.abs(Ea + Eb).max()))


def pose_distance(Ra, ta, Rb, tb):
    """(rotation angle of Ra Rb^T, angle between the translation directions), radians."""
    c = (np.trace(Ra @ Rb.T) - 1.0) / 2.0
    s = np.linalg.norm(Ra @ Rb.T - Rb @ Ra.T) / (2.0 * np.sqrt(2.0))
    return float(np.arctan2(s, c)), float(np.arctan2(np.linalg.norm(np.cross(ta, tb)), ta @ tb))


def sampson(E, x1, x2):
    """Signed Sampson distance per match (normalised units); NaN where the denominator is zero."""
    h1 = np.c_[x1, np.ones(len(x1))]
    h2 = np.c_[x2, np.ones(len(x2))]
    l = h1 @ E.T
    m = h2 @ E
    den = l[:, 0] ** 2 + l[:, 1] ** 2 + m[:, 0] ** 2 + m[:, 1] ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0.0, (h2 * l).sum(axis=1) / np.sqrt(den), np.nan)


def msac(E, x1, x2, thr):
    r = sampson(E, x1, x2)
    return float(np.where(np.isnan(r), thr * thr, np.minimum(r * r, thr * thr)).sum())


def in_front(R, t, x1, x2, max_depth):
    """Both least-squares depths of lambda2 x2~ = lambda1 R x1~ + t in (0, max_depth]; also a = R x1~."""
    a = np.c_[x1, np.ones(len(x1))] @ R.T
    b = np.c_[x2, np.ones(len(x2))]
    aa, bb, ab = (a * a).sum(1), (b * b).sum(1), (a * b).sum(1)
    at, bt = a @ t, b @ t
    det = aa * bb - ab * ab
    ok = det > 1e-24 * aa * bb
    with np.errstate(divide="ignore", invalid="ignore"):
        l1 = (ab * bt - at * bb) / det
        l2 = (aa * bt - ab * at) / det
    ok &= (l1 > 0.0) & (l2 > 0.0)
    if max_depth > 0.0:
        ok &= (l1 <= max_depth) & (l2 <= max_depth)
    return ok, a


# ------------------------------------------------------------------------------------------------------------ five points
def _mul_lin(p, l):
    """Polynomial p (exponent array) times a linear polynomial l = (x, y, z, 1 coefficients)."""
    out = np.zeros(tuple(s + 1 for s in p.shape))
    sx, sy, sz = p.shape
    out[1:sx + 1, :sy, :sz] += l[0] * p
    out[:sx, 1:sy + 1, :sz] += l[1] * p
    out[:sx, :sy, 1:sz + 1] += l[2] * p
    out[:sx, :sy, :sz] += l[3] * p
    return out


# graded order of the action-matrix route: the ten cubics lead, the basis of the quotient ring follows
_GRADED = [(3, 0, 0), (2, 1, 0), (2, 0, 1), (1, 2, 0), (1, 1, 1), (1, 0, 2), (0, 3, 0), (0, 2, 1), (0, 1, 2), (0, 0, 3),
           (2, 0, 0), (1, 1, 0), (1, 0, 1), (0, 2, 0), (0, 1, 1), (0, 0, 2), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]


def constraints(N):
    """The ten cubics of E = x N[0] + y N[1] + z N[2] + N[3] as exponent arrays (4, 4, 4): E E^T E - tr(E E^T) E / 2, det E."""
    lin = [[N[:, 3 * i + j] for j in range(3)] for i in range(3)]
    one = np.ones((1, 1, 1))
    e = [[_mul_lin(one, lin[i][j]) for j in range(3)] for i in range(3)]
    eet = [[sum(_mul_lin(e[i][k], lin[l][k]) for k in range(3)) for l in range(3)] for i in range(3)]
    tr = eet[0][0] + eet[1][1] + eet[2][2]
    out = []
    for i in range(3):
        for j in range(3):
            out.append(sum(_mul_lin(eet[i][l], lin[l][j]) for l in range(3)) - 0.5 * _mul_lin(tr, lin[i][j]))
    det = np.zeros((4, 4, 4))
    for c in range(3):
        p, q = (c + 1) % 3, (c + 2) % 3
        minor = _mul_lin(e[1][p], lin[2][q]) - _mul_lin(e[1][q], lin[2][p])
        det += _mul_lin(minor, lin[0][c])
    out.append(det)
    return out


def five_point(x1, x2):
    """Every real essential matrix (unit Frobenius norm) of five normalised matches; [] for a degenerate sample."""
    A = np.stack([np.kron(np.r_[x2[i], 1.0], np.r_[x1[i], 1.0]) for i in range(5)])
    _, s, vt = np.linalg.svd(A)
    if not s[4] > 1e-12 * s[0]:
        return []
    N = vt[5:9]
    M = np.array([[c[m] for m in _GRADED] for c in constraints(N)])
    # Gauss-Jordan in graded order, rows pivoted
    for c in range(10):
        p = c + int(np.argmax(np.abs(M[c:, c])))
        if not abs(M[p, c]) > 1e-12 * np.abs(M[:, c]).max():
            return []
        M[[c, p]] = M[[p, c]]
        M[c] /= M[c, c]
        for r in range(10):
            if r != c:
                M[r] -= M[r, c] * M[c]
    B = M[:, 10:]
    At = np.zeros((10, 10))
    At[:6] = -B[[0, 1, 2, 3, 4, 5]]              # x (x2, xy, xz, y2, yz, z2) = x3, x2y, x2z, xy2, xyz, xz2
    At[6, 0] = At[7, 1] = At[8, 2] = At[9, 6] = 1.0   # x (x, y, z, 1) = x2, xy, xz, x
    w, V = np.linalg.eig(At)
    out = []
    for k in range(10):
        if abs(w[k].imag) > 1e-10 * max(1.0, abs(w[k])) or abs(V[9, k]) == 0.0:
            continue
        v = (V[:, k] / V[9, k]).real
        E = v[6] * N[0] + v[7] * N[1] + v[8] * N[2] + N[3]
        E = unit_E(E.reshape(3, 3))
        if np.isfinite(E).all():
            out.append(E)
    return out


def cubic_residual(E):
    """max |E E^T E - tr(E E^T) E / 2| and |det E| of a unit-norm E."""
    return float(np.abs(E @ E.T @ E - 0.5 * np.trace(E @ E.T) * E).max()), float(abs(np.linalg.det(E)))


# ------------------------------------------------------------------------------------------------------------ decomposition
def candidates(E):
    """(R_a, +t), (R_a, -t), (R_b, +t), (R_b, -t); u3 = u1 x u2, v3 = v1 x v2."""
    U, _, Vt = np.linalg.svd(E)
    V = Vt.T
    U[:, 2] = np.cross(U[:, 0], U[:, 1])
    V[:, 2] = np.cross(V[:, 0], V[:, 1])
    Ra, Rb, t = U @ W @ V.T, U @ W.T @ V.T, U[:, 2].copy()
    return [(Ra, t), (Ra, -t), (Rb, t), (Rb, -t)]


def recover(E, x1, x2, thr, max_depth):
    """-> (R, t, any vote)."""
    r = sampson(E, x1, x2)
    near = np.abs(r) <= thr
    cands = candidates(E)
    votes = [int((in_front(R, t, x1, x2, max_depth)[0] & near).sum()) for R, t in cands]
    w = int(np.argmax(votes))
    return cands[w][0], cands[w][1], votes[w] > 0


# ------------------------------------------------------------------------------------------------------------ refinement
def tangent(t):
    k = int(np.argmin(np.abs(t)))
    b1 = np.cross(np.eye(3)[k], t)
    b1 /= np.linalg.norm(b1)
    return b1, np.cross(t, b1)


def move(R, t, dx):
    b1, b2 = tangent(t)
    tn = t + dx[3] * b1 + dx[4] * b2
    return exp_so3(dx[:3]) @ R, tn / np.linalg.norm(tn)


def residual_jacobian(R, t, x1, x2):
    """r (n,) and its analytic Jacobian (n, 5) in the local parameters (w | tau) through E = [t]x R."""
    h1 = np.c_[x1, np.ones(len(x1))]
    h2 = np.c_[x2, np.ones(len(x2))]
    b1, b2 = tangent(t)
    E = essential(R, t)
    D = [skew(t) @ skew(np.eye(3)[k]) @ R for k in range(3)] + [skew(b1) @ R, skew(b2) @ R]
    l, m = h1 @ E.T, h2 @ E
    num = (h2 * l).sum(1)
    den = l[:, 0] ** 2 + l[:, 1] ** 2 + m[:, 0] ** 2 + m[:, 1] ** 2
    r = num / np.sqrt(den)
    J = np.empty((len(x1), 5))
    for q, Dq in enumerate(D):
        dl, dm = h1 @ Dq.T, h2 @ Dq
        dnum = (h2 * dl).sum(1)
        dden = 2.0 * (l[:, 0] * dl[:, 0] + l[:, 1] * dl[:, 1] + m[:, 0] * dm[:, 0] + m[:, 1] * dm[:, 1])
        J[:, q] = dnum / np.sqrt(den) - 0.5 * num * dden / den ** 1.5
    return r, J


def refine(R, t, x1, x2, iters=20):
    """ba_resect's step 3 in the five local parameters on 0.5 sum r^2; -> (R, t, ok)."""
    lam, first, small, it = 1e-4, True, False, 0
    Rt, tt = R, t
    cost = H = g = None
    while True:
        r, J = residual_jacobian(Rt, tt, x1, x2)
        c = 0.5 * float(r @ r)
        if first or c <= cost * (1.0 + 1e-12):
            cost, H, g = c, J.T @ J, J.T @ r
            R, t = Rt, tt
            if not first:
                lam = max(0.1 * lam, 1e-12)
        else:
            lam *= 10.0
        first = False
        if small or it >= iters:
            break
        it += 1
        try:
            L = np.linalg.cholesky(H + lam * np.diag(np.diag(H)))
        except np.linalg.LinAlgError:
            return R, t, False
        dx = -np.linalg.solve(L.T, np.linalg.solve(L, g))
        Rt, tt = move(R, t, dx)
        small = np.linalg.norm(dx) <= 1e-14
    return R, t, True


def inlier_set(R, t, x1, x2, thr, max_depth):
    r = sampson(essential(R, t), x1, x2)
    front, a = in_front(R, t, x1, x2, max_depth)
    return (np.abs(r) <= thr) & front, r, a


# ------------------------------------------------------------------------------------------------------------ the call
def hypothesis_costs(K, p1, p2, pair=0, n_hyp=256, seed=0, max_epi_px=3.0):
    """Steps 2 - 4 of the header, hypothesis by hypothesis -> (cost (n_hyp,): the lowest MSAC cost over the hypothesis's
    solutions, inf when it has none; slot (n_hyp,): which of five_point's solutions that is, the first of equal ones, -1 when
    void; E: that solution, None when void).  The winner of step 4 among the first N hypotheses is the first lowest of
    cost[:N]: `winner`."""
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    x1, x2 = normalise(K, p1), normalise(K, p2)
    thr = max_epi_px / (0.5 * (K[0, 0] + K[1, 1]))
    cost, slot, Es = np.full(n_hyp, np.inf), np.full(n_hyp, -1, dtype=np.int64), [None] * n_hyp
    for h in range(n_hyp):
        idx = list(sample5(seed, pair, h, len(p1)))
        for s, E in enumerate(five_point(x1[idx], x2[idx])):
            c = msac(E, x1, x2, thr)
            if c < cost[h]:
                cost[h], slot[h], Es[h] = c, s, E
    return cost, slot, Es


def relative_pose(K, p1, p2, pair=0, n_hyp=256, lo_rounds=2, seed=0, max_epi_px=3.0, refine_iters=20, min_inliers=8,
                  min_parallax_deg=0.0, max_depth=50.0):
    """One pair (its index in the call: `pair`), steps 0 - 7 of the header."""
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    n = len(p1)
    nan = float("nan")
    out = dict(R=np.eye(3), t=np.zeros(3), status=OK, n_inliers=0, rms_px=nan, parallax_deg=nan, best_hyp=-1,
               match_inlier=np.zeros(n, dtype=bool), E_raw=None)
    if n < 6:
        out["status"] = FEW_MATCHES
        return out
    x1, x2 = normalise(K, p1), normalise(K, p2)
    fbar = 0.5 * (K[0, 0] + K[1, 1])
    thr = max_epi_px / fbar
    cost, _, Es = hypothesis_costs(K, p1, p2, pair, n_hyp, seed, max_epi_px)
    h = winner(cost)
    best = (cost[h], h, Es[h]) if h >= 0 else (np.inf, -1, None)
    if best[2] is None:
        out["status"] = DEGENERATE
        return out
    out["best_hyp"], out["E_raw"] = best[1], best[2]
    R, t, voted = recover(best[2], x1, x2, thr, max_depth)
    status = OK if voted else BEHIND
    for _ in range(lo_rounds if status == OK else 0):
        cons, _, _ = inlier_set(R, t, x1, x2, thr, max_depth)
        if not cons.any():
            break
        R, t, ok = refine(R, t, x1[cons], x2[cons], refine_iters)
        if not ok:
            status = DEGENERATE
            break
    inl, r, a = inlier_set(R, t, x1, x2, thr, max_depth)
    out.update(R=R, t=t, match_inlier=inl, n_inliers=int(inl.sum()))
    if inl.any():
        b = np.c_[x2, np.ones(n)][inl]
        ang = np.arctan2(np.linalg.norm(np.cross(a[inl], b), axis=1), (a[inl] * b).sum(1))
        out["rms_px"] = float(fbar * np.sqrt((r[inl] ** 2).mean()))
        out["parallax_deg"] = float(np.degrees(ang.mean()))
    if status == OK:
        if out["n_inliers"] < min_inliers:
            status = FEW_INLIERS
        elif min_parallax_deg > 0.0 and not out["parallax_deg"] >= min_parallax_deg:
            status = LOW_PARALLAX
    out["status"] = status
    return out


# ------------------------------------------------------------------------------------------------------------ scenes
BASELINE = 2.0     # of the scenes, in their own unit: depths of 2 .. 4 baselines, a parallax of about 17 degrees
# Exactly coplanar matches admit TWO essential matrices (the plane's twisted pair), both with zero Sampson cost; only the
# cheirality votes tell them apart, and step 4 chooses by cost before step 5 votes (planar model selection is out of scope).
# The tests' "planar" scene is therefore a desk: a tilted plane with a relief of +-RELIEF (10 % of its depth), on which the twisted pair costs more than the truth.
RELIEF = 0.6
K_TEST = np.array([[820.0, 0.0, 640.0], [0.0, 790.0, 360.0], [0.0, 0.0, 1.0]])


def make_pose(rng):
    """A rotation of about 8 degrees and a unit translation, mostly sideways (depths of 8 .. 16 baselines in the scenes below)."""
    w = rng.normal(size=3)
    R = exp_so3(0.14 * w / np.linalg.norm(w))
    t = np.array([1.0, 0.0, 0.0]) + 0.3 * rng.normal(size=3)
    return R, t / np.linalg.norm(t)


def make_scene(rng, n, planar=False, baseline=BASELINE, relief=0.0):
    """n points in front of both views (a box 4 x 3 x 4 at depth 4 .. 8, or a tilted plane in it with a uniform relief of
    +-`relief` across it), a pose, exact pixels.  -> (p1, p2, R, t) with |t| = 1; the scene's unit is `baseline`."""
    R, t = make_pose(rng)
    X = np.c_[rng.uniform(-2.0, 2.0, n), rng.uniform(-1.5, 1.5, n), rng.uniform(4.0, 8.0, n)]
    if planar:
        X[:, 2] = 6.0 + 0.35 * X[:, 0] - 0.25 * X[:, 1] + rng.uniform(-1.0, 1.0, n) * relief
    Y = X @ R.T + baseline * t
    p1 = (X / X[:, 2:]) @ K_TEST.T
    p2 = (Y / Y[:, 2:]) @ K_TEST.T
    return p1[:, :2].copy(), p2[:, :2].copy(), R, t


def truncated_noise(rng, shape, sigma=0.3, limit=1.0):
    e = rng.normal(scale=sigma, size=shape)
    bad = np.abs(e) > limit
    while bad.any():
        e[bad] = rng.normal(scale=sigma, size=int(bad.sum()))
        bad = np.abs(e) > limit
    return e


def noisy_scene(n, planar=False, seed=0, sigma=0.3):
    """Inlier noise of sigma px, truncated at 1 px, on both views; no mismatches."""
    rng = np.random.default_rng(seed)
    p1, p2, R, t = make_scene(rng, n, planar, relief=RELIEF)
    return p1 + truncated_noise(rng, p1.shape, sigma), p2 + truncated_noise(rng, p2.shape, sigma), R, t


def yardstick(K, p1, p2, R, t, rounds=3):
    """The refinement of step 6 from the truth on the given matches, repeated: the minimum the library should reach."""
    x1, x2 = normalise(K, p1), normalise(K, p2)
    for _ in range(rounds):
        R, t, ok = refine(R, t, x1, x2, 20)
        assert ok
    return R, t


@functools.lru_cache(maxsize=None)
def outlier_case(planar, share, n=300, seed=5):
    """Case 3: n matches, a share of them uniform mismatches re-drawn until each lies more than 6 px (Sampson) from the true
    epipolar geometry.  -> dict(p1, p2, R, t, planted (bool: a mismatch), yard (R, t), ref (the reference's own call),
    d_ref (its distance to the yardstick))."""
    rng = np.random.default_rng(seed + 100 * int(planar) + int(round(share * 10)))
    p1, p2, R, t = make_scene(rng, n, planar, relief=RELIEF)
    p1 = p1 + truncated_noise(rng, p1.shape)
    p2 = p2 + truncated_noise(rng, p2.shape)
    planted = np.zeros(n, dtype=bool)
    planted[rng.choice(n, int(round(share * n)), replace=False)] = True
    E = essential(R, t)
    fbar = 0.5 * (K_TEST[0, 0] + K_TEST[1, 1])
    todo = np.nonzero(planted)[0]
    while todo.size:
        p2[todo] = np.c_[rng.uniform(0.0, 1280.0, todo.size), rng.uniform(0.0, 720.0, todo.size)]
        r = sampson(E, normalise(K_TEST, p1[todo]), normalise(K_TEST, p2[todo])) * fbar
        todo = todo[~(np.abs(r) > 6.0)]
    yard = yardstick(K_TEST, p1[~planted], p2[~planted], R, t)
    ref = relative_pose(K_TEST, p1, p2, n_hyp=256)
    d_ref = pose_distance(ref["R"], ref["t"], *yard)
    for a in (p1, p2, planted):
        a.setflags(write=False)
    return dict(p1=p1, p2=p2, R=R, t=t, planted=planted, yard=yard, ref=ref, d_ref=d_ref)
