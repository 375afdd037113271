"""Yardstick of the homography tests: ba_homography restated in numpy (include/ba_hip.h, steps 0 - 8).  Where the header's route
could share a bug with the library another one is taken as well: the minimal solver is also the SVD null vector of the 8 x 9
DLT (`four_point_dlt`), the decomposition uses LAPACK's SVD instead of the library's Jacobi, the backward transfer uses
numpy.linalg.inv instead of the adjugate.  The generator, the MSAC scoring of the symmetric transfer error, the refinement (same
parametrisation, same damping and acceptance rules), the votes and the ordering of the two poses are the header's.  Scene
builders on top of tests/relpose_reference.py: the exact plane, a pure rotation, planted mismatches.  Test infrastructure only."""
import functools
import itertools

import numpy as np

from tests import relpose_reference as RP
from tests.ransac_reference import sample

OK, FEW_MATCHES, DEGENERATE, FEW_INLIERS, ROTATION, AMBIGUOUS = range(6)
K_TEST = RP.K_TEST
AREA_TOL = 1e-6
DET_TOL = 1e-12
# the default of ba_homography_options.min_translation: the geometric mean of the largest (d1 - d3) / d2 of the pure rotation
# under 0.3 px of noise and the smallest of the tests' plane (test_homography_host.py measures both)
MIN_TRANSLATION = 0.024


# ------------------------------------------------------------------------------------------------------------ generator
def sample4(seed, pair, h, n):
    return sample(seed, pair, h, n, 4)


# ------------------------------------------------------------------------------------------------------------ geometry
def hom(x):
    return np.c_[x, np.ones(len(x))]


def unit_H(H):
    """Unit Frobenius norm and det > 0."""
    H = H / np.linalg.norm(H)
    return -H if np.linalg.det(H) < 0.0 else H


def H_distance(Ha, Hb):
    return float(np.abs(unit_H(Ha) - unit_H(Hb)).max())


def adj(M):
    """Adjugate of a 3 x 3 by cofactors."""
    c = np.empty((3, 3))
    for i in range(3):
        for j in range(3):
            r, s = [k for k in range(3) if k != i], [k for k in range(3) if k != j]
            c[j, i] = (-1) ** (i + j) * (M[r[0], s[0]] * M[r[1], s[1]] - M[r[0], s[1]] * M[r[1], s[0]])
    return c


def true_homography(R, t, n, d):
    """H~ of the plane n . X = d (first camera's frame) under x2 ~ R x1 + t: R + t n^T / d."""
    return R + np.outer(t, n) / d


def pixel_H(K, Hn):
    return unit_H(K @ Hn @ np.linalg.inv(K))


def normalised_H(K, H):
    return unit_H(np.linalg.inv(K) @ H @ K)


def transfer(Hn, x1, x2, backward=None):
    """Squared forward and backward transfer errors per match and whether both third components are positive.  `backward`:
    the matrix of the backward map (default numpy.linalg.inv, scaled to a positive multiple of the adjugate)."""
    Hb = np.linalg.inv(Hn) * np.sign(np.linalg.det(Hn)) if backward is None else backward
    y, z = hom(x1) @ Hn.T, hom(x2) @ Hb.T
    with np.errstate(divide="ignore", invalid="ignore"):
        f = ((y[:, :2] / y[:, 2:] - x2) ** 2).sum(1)
        b = ((z[:, :2] / z[:, 2:] - x1) ** 2).sum(1)
    return f, b, y[:, 2] > 0.0, z[:, 2] > 0.0


def msac(Hn, x1, x2, thr):
    f, b, pf, pb = transfer(Hn, x1, x2)
    t2 = thr * thr
    return float(np.where(pf, np.minimum(f, t2), t2).sum() + np.where(pb, np.minimum(b, t2), t2).sum())


def consensus(Hn, x1, x2, thr):
    f, b, pf, pb = transfer(Hn, x1, x2)
    t2 = thr * thr
    with np.errstate(invalid="ignore"):
        return pf & pb & (f <= t2) & (b <= t2), f, b


# ------------------------------------------------------------------------------------------------------------ four points
def collinear(x):
    """A triple of the four points (4, 2) with |d12 x d13| <= AREA_TOL max |d_ij|^2."""
    for a, b, c in itertools.combinations(range(4), 3):
        d12, d13, d23 = x[b] - x[a], x[c] - x[a], x[c] - x[b]
        ext = max(d12 @ d12, d13 @ d13, d23 @ d23)
        cr = abs(d12[0] * d13[1] - d12[1] * d13[0])
        if not (cr > AREA_TOL * ext) or not np.isfinite(ext):
            return True
    return False


def _basis(x):
    M = hom(x[:3]).T
    lam = adj(M) @ np.r_[x[3], 1.0]
    return M * lam[None, :]


def four_point(x1, x2):
    """The header's closed form: H~ = B2 adj(B1) at unit norm and det > 0; None for a void sample."""
    if collinear(x1) or collinear(x2):
        return None
    H = _basis(x2) @ adj(_basis(x1))
    nrm = np.linalg.norm(H)
    if not np.isfinite(nrm) or not nrm > 0.0:
        return None
    H = H / nrm
    det = np.linalg.det(H)
    if not abs(det) > DET_TOL:
        return None
    if det < 0.0:
        H = -H
    if not ((hom(x1) @ H.T)[:, 2] > 0.0).all():
        return None
    return H


def four_point_dlt(x1, x2):
    """The other route: the null vector of the 8 x 9 DLT by LAPACK's SVD."""
    A = []
    for (u, v), (p, q) in zip(x1, x2):
        A.append([-u, -v, -1.0, 0.0, 0.0, 0.0, p * u, p * v, p])
        A.append([0.0, 0.0, 0.0, -u, -v, -1.0, q * u, q * v, q])
    return unit_H(np.linalg.svd(np.array(A))[2][8].reshape(3, 3))


# ------------------------------------------------------------------------------------------------------------ refinement
def _delta(p):
    return np.array([[p[0], p[1], p[2]], [p[3], p[4], p[5]], [p[6], p[7], -(p[0] + p[4])]])


def residual_jacobian(Hn, x1, x2):
    """r (m, 4) = (r_f | r_b) and its Jacobian (m, 4, 8) in the entries of the traceless D of H (I + D); the backward residual
    sees (I - D) H^-1.  Matches with a non-positive third component are left out; `all_in_front` says that there was none."""
    Hb = np.linalg.inv(Hn) * np.sign(np.linalg.det(Hn))
    h1, h2 = hom(x1), hom(x2)
    y, z = h1 @ Hn.T, h2 @ Hb.T
    keep = (y[:, 2] > 0.0) & (z[:, 2] > 0.0)
    h1, h2, y, z = h1[keep], h2[keep], y[keep], z[keep]
    m = len(y)
    r = np.c_[y[:, :2] / y[:, 2:] - h2[:, :2], z[:, :2] / z[:, 2:] - h1[:, :2]]
    J = np.zeros((m, 4, 8))
    for k in range(8):
        e = np.zeros(8)
        e[k] = 1.0
        D = _delta(e)
        dy = h1 @ (Hn @ D).T
        dz = -(z @ D.T)
        J[:, 0:2, k] = (dy[:, :2] - y[:, :2] / y[:, 2:] * dy[:, 2:]) / y[:, 2:]
        J[:, 2:4, k] = (dz[:, :2] - z[:, :2] / z[:, 2:] * dz[:, 2:]) / z[:, 2:]
    return r.reshape(-1), J.reshape(-1, 8), bool(keep.all())


def refine(Hn, x1, x2, iters=20):
    """ba_resect's step (3) in the eight local parameters on 0.5 sum (|r_f|^2 + |r_b|^2); -> (H~, ok)."""
    lam, first, small, it = 1e-4, True, False, 0
    Ht = Hn
    cost = A = g = None
    while True:
        r, J, all_in_front = residual_jacobian(Ht, x1, x2)
        c = 0.5 * float(r @ r) if all_in_front else np.inf          # a trial that puts a match behind a camera is rejected
        if first or c <= cost * (1.0 + 1e-12):
            cost, A, g = c, J.T @ J, J.T @ r
            Hn = Ht
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
            return Hn, False
        dx = -np.linalg.solve(L.T, np.linalg.solve(L, g))
        if not np.isfinite(dx).all():
            return Hn, False
        Ht = unit_H(Hn @ (np.eye(3) + _delta(dx)))
        small = np.linalg.norm(dx) <= 1e-14
    return Hn, True


# ------------------------------------------------------------------------------------------------------------ decomposition
def singular_values(Hn):
    return np.linalg.svd(Hn)[1]


def candidates(Hn):
    """The four d' = +d2 candidates of Faugeras & Lustman (1988) for det H~ > 0: (R, t, n, t / d), |t| = |n| = 1, in the order
    (e1, e3) = (+, +), (-, -), (+, -), (-, +): the first two and the last two share R and differ by the sign of both t and n.
    H~ / d2 = R + (t / d) n^T for each."""
    U, d, Vt = np.linalg.svd(Hn)
    V = Vt.T
    U[:, 2] = np.cross(U[:, 0], U[:, 1])
    V[:, 2] = np.cross(V[:, 0], V[:, 1])
    d1, d2, d3 = d
    den = d1 * d1 - d3 * d3
    a1, a3 = np.sqrt(max(d1 * d1 - d2 * d2, 0.0) / den), np.sqrt(max(d2 * d2 - d3 * d3, 0.0) / den)
    ct = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2)
    out = []
    for e1, e3 in ((1.0, 1.0), (-1.0, -1.0), (1.0, -1.0), (-1.0, 1.0)):
        st = e1 * e3 * np.sqrt(max(d1 * d1 - d2 * d2, 0.0) * max(d2 * d2 - d3 * d3, 0.0)) / ((d1 + d3) * d2)
        Rp = np.array([[ct, 0.0, -st], [0.0, 1.0, 0.0], [st, 0.0, ct]])
        out.append((U @ Rp @ V.T, U @ np.array([e1 * a1, 0.0, -e3 * a3]), V @ np.array([e1 * a1, 0.0, e3 * a3]), (d1 - d3) / d2))
    return out


def decompose(Hn, x1, x2, inl, thr, max_depth, min_translation, ambiguity_ratio):
    """Step 7 -> dict(rotation (bool), n_pose, R (2, 3, 3), t, normal (2, 3), t_over_d, votes, pose_cost (2,), ambiguous)."""
    nan = float("nan")
    out = dict(rotation=False, ambiguous=False, n_pose=0, R=np.tile(np.eye(3), (2, 1, 1)), t=np.zeros((2, 3)), normal=np.zeros((2, 3)),
               t_over_d=np.zeros(2), votes=np.zeros(2, dtype=np.int64), pose_cost=np.full(2, nan))
    U, d, Vt = np.linalg.svd(Hn)
    ratio = (d[0] - d[2]) / d[1]
    if not ratio > min_translation:
        V = Vt.T
        U[:, 2] = np.cross(U[:, 0], U[:, 1])
        V[:, 2] = np.cross(V[:, 0], V[:, 1])
        out["R"][0] = U @ V.T
        out.update(rotation=True, n_pose=1)
        out["t_over_d"][0] = ratio
        return out
    cands = candidates(Hn)
    h1 = hom(x1)
    poses = []
    for k in (0, 2):
        R, t, n, s = cands[k]
        side = h1[inl] @ n
        if (side < 0.0).sum() > (side > 0.0).sum():
            R, t, n, s = cands[k + 1]
        front, _ = RP.in_front(R, t, x1, x2, max_depth)
        votes = int((front & inl & (h1 @ n > 0.0)).sum())
        poses.append((R, t, n, s, votes, RP.msac(RP.essential(R, t), x1, x2, thr), k // 2))
    poses.sort(key=lambda p: (-p[4], p[5], p[6]))
    for i, (R, t, n, s, votes, cost, _) in enumerate(poses):
        out["R"][i], out["t"][i], out["normal"][i], out["t_over_d"][i], out["votes"][i], out["pose_cost"][i] = R, t, n, s, votes, cost
    out["n_pose"] = int((out["votes"] > 0).sum())
    out["ambiguous"] = bool(out["votes"][1] >= ambiguity_ratio * out["votes"][0])
    return out


# ------------------------------------------------------------------------------------------------------------ the call
def hypothesis_costs(K, p1, p2, pair=0, n_hyp=256, seed=0, max_px=3.0):
    """Steps 2 - 4 of the header, hypothesis by hypothesis -> (cost (n_hyp,): the MSAC cost of the hypothesis's H~, inf when it
    is void; slot (n_hyp,): 0, -1 when void (a sample has one solution); H: that H~, None when void).  The winner of step 4
    among the first N hypotheses is relpose_reference.winner(cost, N)."""
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    x1, x2 = RP.normalise(K, p1), RP.normalise(K, p2)
    thr = max_px / (0.5 * (K[0, 0] + K[1, 1]))
    cost, slot, Hs = np.full(n_hyp, np.inf), np.full(n_hyp, -1, dtype=np.int64), [None] * n_hyp
    for h in range(n_hyp):
        idx = list(sample4(seed, pair, h, len(p1)))
        Hh = four_point(x1[idx], x2[idx])
        if Hh is None:
            continue
        c = msac(Hh, x1, x2, thr)
        if c < np.inf:
            cost[h], slot[h], Hs[h] = c, 0, Hh
    return cost, slot, Hs


winner = RP.winner


def homography(K, p1, p2, pair=0, n_hyp=256, lo_rounds=2, seed=0, max_px=3.0, refine_iters=20, min_inliers=8, max_depth=50.0,
               ambiguity_ratio=0.75, min_translation=MIN_TRANSLATION):
    """One pair (its index in the call: `pair`), steps 0 - 8 of the header.  Hn is H~ (normalised coordinates), H the pixel one."""
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    n = len(p1)
    nan = float("nan")
    out = dict(H=np.eye(3), Hn=np.eye(3), status=OK, n_inliers=0, rms_px=nan, best_hyp=-1, match_inlier=np.zeros(n, dtype=bool),
               n_pose=0, R=np.tile(np.eye(3), (2, 1, 1)), t=np.zeros((2, 3)), normal=np.zeros((2, 3)), t_over_d=np.zeros(2),
               votes=np.zeros(2, dtype=np.int64), pose_cost=np.full(2, nan), H_raw=None)
    if n < 5:
        out["status"] = FEW_MATCHES
        return out
    x1, x2 = RP.normalise(K, p1), RP.normalise(K, p2)
    fbar = 0.5 * (K[0, 0] + K[1, 1])
    thr = max_px / fbar
    cost, _, Hs = hypothesis_costs(K, p1, p2, pair, n_hyp, seed, max_px)
    h = winner(cost)
    best = (cost[h], h, Hs[h]) if h >= 0 else (np.inf, -1, None)
    if best[2] is None:
        out["status"] = DEGENERATE
        return out
    Hn = best[2]
    out["best_hyp"], out["H_raw"] = best[1], Hn
    status = OK
    for _ in range(lo_rounds):
        cons, _, _ = consensus(Hn, x1, x2, thr)
        if not cons.any():
            break
        Hn, ok = refine(Hn, x1[cons], x2[cons], refine_iters)
        if not ok:
            status = DEGENERATE
            break
    inl, f, b = consensus(Hn, x1, x2, thr)
    out.update(Hn=Hn, H=pixel_H(K, Hn), match_inlier=inl, n_inliers=int(inl.sum()))
    if inl.any():
        out["rms_px"] = float(fbar * np.sqrt(0.5 * (f[inl] + b[inl]).mean()))
    dec = decompose(Hn, x1, x2, inl, thr, max_depth, min_translation, ambiguity_ratio)
    for k in ("n_pose", "R", "t", "normal", "t_over_d", "votes", "pose_cost"):
        out[k] = dec[k]
    if status == OK:
        if out["n_inliers"] < min_inliers:
            status = FEW_INLIERS
        elif dec["rotation"]:
            status = ROTATION
        elif dec["ambiguous"]:
            status = AMBIGUOUS
    out["status"] = status
    return out


# ------------------------------------------------------------------------------------------------------------ scenes
PLANE_N = np.array([-0.35, 0.25, 1.0])     # make_scene's plane: z = 6 + 0.35 x - 0.25 y, that is PLANE_N . X = 6
PLANE_D = 6.0


def plane_scene(rng, n):
    """relpose_reference's exactly planar scene (relief 0), exact pixels, and the plane's true H~ (unit norm, det > 0)."""
    p1, p2, R, t = RP.make_scene(rng, n, planar=True, relief=0.0)
    return p1, p2, R, t, unit_H(true_homography(R, RP.BASELINE * t, PLANE_N, PLANE_D))


def true_plane_pose(R, t):
    """(R, t, unit normal towards the camera's +z) of the plane scene."""
    return R, t, PLANE_N / np.linalg.norm(PLANE_N)


@functools.lru_cache(maxsize=None)
def noisy_plane(seed, n=300, sigma=0.3):
    """The issue's draws: the exact plane, n matches, truncated noise on both views.  -> (p1, p2, R, t, H~ true)."""
    rng = np.random.default_rng(seed)
    p1, p2, R, t, Ht = plane_scene(rng, n)
    p1 = p1 + RP.truncated_noise(rng, p1.shape, sigma)
    p2 = p2 + RP.truncated_noise(rng, p2.shape, sigma)
    for a in (p1, p2):
        a.setflags(write=False)
    return p1, p2, R, t, Ht


@functools.lru_cache(maxsize=None)
def rotation_scene(seed, n=300, sigma=0.3):
    """A pure rotation of the box scene: x2 ~ K R K^-1 x1, truncated noise on both views.  -> (p1, p2, R)."""
    rng = np.random.default_rng(1000 + seed)
    p1, _, R, _ = RP.make_scene(rng, n)
    Y = hom(RP.normalise(K_TEST, p1)) @ R.T
    p2 = ((Y / Y[:, 2:]) @ K_TEST.T)[:, :2]
    p1 = p1 + RP.truncated_noise(rng, p1.shape, sigma)
    p2 = p2 + RP.truncated_noise(rng, p2.shape, sigma)
    for a in (p1, p2):
        a.setflags(write=False)
    return p1, p2, R


def yardstick(K, p1, p2, Hn, rounds=3):
    """The refinement of step 5 from the true H~ on the given matches, repeated: the minimum the library should reach."""
    x1, x2 = RP.normalise(K, p1), RP.normalise(K, p2)
    for _ in range(rounds):
        Hn, ok = refine(Hn, x1, x2, 20)
        assert ok
    return Hn


@functools.lru_cache(maxsize=None)
def outlier_case(share, n=300, seed=5):
    """The exact plane, n matches, truncated noise, a share of them uniform mismatches re-drawn until each lies more than 6 px
    (forward transfer error) from the true H.  -> dict(p1, p2, R, t, Ht, planted (bool: a mismatch), yard (H~), ref (the
    reference's own call), d_ref (its distance to the yardstick))."""
    rng = np.random.default_rng(seed + int(round(share * 10)))
    p1, p2, R, t, Ht = plane_scene(rng, n)
    p1 = p1 + RP.truncated_noise(rng, p1.shape)
    p2 = p2 + RP.truncated_noise(rng, p2.shape)
    planted = np.zeros(n, dtype=bool)
    planted[rng.choice(n, int(round(share * n)), replace=False)] = True
    Hp = K_TEST @ Ht @ np.linalg.inv(K_TEST)
    todo = np.nonzero(planted)[0]
    while todo.size:
        p2[todo] = np.c_[rng.uniform(0.0, 1280.0, todo.size), rng.uniform(0.0, 720.0, todo.size)]
        y = hom(p1[todo]) @ Hp.T
        err = np.linalg.norm(y[:, :2] / y[:, 2:] - p2[todo], axis=1)
        todo = todo[~(err > 6.0)]
    yard = yardstick(K_TEST, p1[~planted], p2[~planted], Ht)
    ref = homography(K_TEST, p1, p2, n_hyp=256)
    for a in (p1, p2, planted):
        a.setflags(write=False)
    return dict(p1=p1, p2=p2, R=R, t=t, Ht=Ht, planted=planted, yard=yard, ref=ref, d_ref=H_distance(ref["Hn"], yard))
