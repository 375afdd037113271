"""CPU: the numpy yardstick of ba_fundamental (tests/fundamental_reference.py) against the truth, the conditions the GPU tests
rely on, the host-side closed form for the focal lengths and the Python helpers on a stub solver.  No GPU, no library."""
import numpy as np
import pytest

from bundle_adjustment_amd import features, pose_estimator
from tests import fundamental_reference as FR
from tests import homography_reference as HG
from tests import relpose_reference as RP


# ---------------------------------------------------------------------------------------------------- (a) the solver alone
def test_reference_solver_holds_the_true_F_on_exact_matches():
    """8 scenes of 12 exact matches, 16 seeds, one hypothesis: every solve that is not void holds the true F (the best of its
    up to three solutions), and at most 2 of 128 are void.  Bound 1e-8: the seven-point problem on exact pixels loses about six
    digits to its conditioning in the worst of these samples (measured: 0 void, worst 8.0e-11)."""
    scenes = FR.exact_scenes()
    worst, void = 0.0, 0
    for seed in range(16):
        for p, (p1, p2, Ft) in enumerate(scenes):
            r = FR.fundamental(p1, p2, pair=p, n_hyp=1, lo_rounds=0, seed=seed, min_inliers=8)
            if r["best_hyp"] < 0:
                void += 1
                assert r["status"] == FR.DEGENERATE and not r["F"].any()
                continue
            assert r["status"] == FR.OK and r["n_inliers"] == 12
            worst = max(worst, FR.F_distance(r["F"], Ft))
    print(f"reference, one seven-point sample of 12 exact matches: {void} void of 128, worst distance to the true F {worst:.2e}")
    assert void <= 2 and worst <= 1e-8


def test_reference_generator_draws_distinct_indices():
    for n in (7, 8, 9, 300):
        for h in range(50):
            idx = FR.sample7(3, 5, h, n)
            assert len(set(idx)) == 7 and min(idx) >= 0 and max(idx) < n
    assert FR.sample7(0, 0, 0, 300)[:5] == RP.sample5(0, 0, 0, 300)      # the same generator, two more draws


def test_reference_jacobian_matches_finite_differences():
    p1, p2, Ft = FR.exact_scenes()[0]
    (c1, s1), (c2, s2) = FR.hartley(p1), FR.hartley(p2)
    U, V, sg = FR.canon_svd(FR.normalised_F(Ft, c1, s1, c2, s2))
    rng = np.random.default_rng(0)
    q1, q2 = p1 - c1 + rng.normal(size=p1.shape), p2 - c2
    _, J = FR.residual_jacobian(U, V, sg, q1, q2, s1, s2)
    eps, Jn = 1e-6, np.empty_like(J)
    for k in range(7):
        dx = np.zeros(7)
        dx[k] = eps
        rp, _ = FR.residual_jacobian(U @ RP.exp_so3(dx[:3]), V @ RP.exp_so3(dx[3:6]), sg + dx[6], q1, q2, s1, s2)
        rm, _ = FR.residual_jacobian(U @ RP.exp_so3(-dx[:3]), V @ RP.exp_so3(-dx[3:6]), sg - dx[6], q1, q2, s1, s2)
        Jn[:, k] = (rp - rm) / (2.0 * eps)
    assert np.abs(J - Jn).max() <= 1e-6 * np.abs(J).max()


# ---------------------------------------------------------------------------------------------------- (b) outliers
@pytest.mark.parametrize("share,n_hyp,seed", FR.OUTLIER_CASES)
def test_reference_ends_with_the_planted_inliers(share, n_hyp, seed):
    """Both cases at seed 0, as the issue has them.  The mismatches lie more than 6 px from the true geometry and the noise is
    truncated at 1 px, so the final consensus set at 3 px is exactly the true inliers."""
    c = FR.outlier_case(share, n_hyp, seed)
    ref = c["ref"]
    print(f"share={share} n_hyp={n_hyp}: status {ref['status']}, {ref['n_inliers']} inliers, best_hyp {ref['best_hyp']}, rms {ref['rms_px']:.3f} px, "
          f"F to the yardstick {c['d_ref']:.2e}, to the true F {FR.F_distance(ref['F'], c['F_true']):.2e}")
    assert ref["status"] == FR.OK and np.array_equal(ref["match_inlier"], ~c["planted"])
    assert c["d_ref"] <= 1e-9
    assert np.linalg.norm(ref["F"] @ ref["epipole1"]) <= 1e-12 and np.linalg.norm(ref["F"].T @ ref["epipole2"]) <= 1e-12
    assert abs(np.linalg.norm(ref["F"]) - 1.0) <= 1e-15 and ref["F"].ravel()[np.argmax(np.abs(ref["F"]))] > 0.0


# ---------------------------------------------------------------------------------------------------- (c) the GPU file's edges
def test_reference_solves_every_edge_case_and_pins_the_winner():
    """Every pair of the edge call is one the reference solves with status OK and all matches inliers (edge_pairs asserts it),
    for every n_hyp of the GPU test (the winner of a prefix of the hypotheses' costs).  Near-ties: the arg-min is pinned when the
    two lowest costs differ by more than 1e-9 relative.  The pairs of 8 and 9 matches tie from n_hyp = 85 on because the same
    seven matches are drawn again in another order (8 and 36 distinct samples; same_sample says so): no scene seed cures that,
    so the GPU test asks such a pair for a winner inside the tie set instead, and the budget of one (pair, n_hyp) in ten left
    out is checked here on the ties that a scene could cause."""
    pairs, yard, d_ref, cost = FR.edge_pairs()
    combos, structural, other = 0, 0, 0
    for n_hyp in FR.EDGE_N_HYP:
        for i, n in enumerate(FR.COUNTS):
            if n < 8:
                continue
            combos += 1
            assert np.isfinite(cost[i][:n_hyp]).any()
            ties = FR.tie_set(cost[i], n_hyp)
            assert FR.winner(cost[i], n_hyp) in ties
            if len(ties) > 1:
                if FR.same_sample(ties, i, n):
                    structural += 1
                else:
                    other += 1
    print(f"{combos} (pair, n_hyp): {structural} near-ties of one sample drawn twice, {other} other near-ties; d_ref {[f'{d:.1e}' for d in d_ref if d is not None]}")
    assert 10 * other <= combos
    assert max(d for d in d_ref if d is not None) <= 1e-9


def test_reference_degenerate_inputs():
    r = FR.fundamental(*FR.line_case(), n_hyp=64)
    assert r["status"] == FR.DEGENERATE and r["best_hyp"] == -1 and not r["F"].any()
    r = FR.fundamental(*FR.point_case(), n_hyp=64)
    assert r["status"] == FR.DEGENERATE and r["best_hyp"] == -1
    c = FR.outlier_case(0.3, 256)
    assert FR.fundamental(c["p1"][:7], c["p2"][:7])["status"] == FR.FEW_MATCHES


def test_reference_does_not_move_under_a_shift():
    """The Hartley step: the 0.3 case moved by (5e4, -3e4) px in both images gives the same inliers and T^T F T."""
    c = FR.outlier_case(0.3, 256)
    sh = np.array([5e4, -3e4])
    r = FR.fundamental(c["p1"] + sh, c["p2"] + sh, n_hyp=256)
    T = np.array([[1.0, 0.0, sh[0]], [0.0, 1.0, sh[1]], [0.0, 0.0, 1.0]])
    d = FR.F_distance(T.T @ r["F"] @ T, c["ref"]["F"])
    print(f"reference under a shift of (5e4, -3e4) px: T^T F T to the unshifted F {d:.2e}")
    assert np.array_equal(r["match_inlier"], c["ref"]["match_inlier"]) and d <= 1e-9


# ---------------------------------------------------------------------------------------------------- (d) focal lengths
def test_focal_from_fundamental_on_exact_F():
    rng = np.random.default_rng(7)
    worst = 0.0
    for _ in range(200):
        R, t = RP.make_pose(rng)
        f1, f2 = rng.uniform(500.0, 1500.0, 2)
        pp1, pp2 = np.array([640.0, 360.0]) + 30.0 * rng.normal(size=2), np.array([600.0, 380.0]) + 30.0 * rng.normal(size=2)
        K1 = np.array([[f1, 0.0, pp1[0]], [0.0, f1, pp1[1]], [0.0, 0.0, 1.0]])
        K2 = np.array([[f2, 0.0, pp2[0]], [0.0, f2, pp2[1]], [0.0, 0.0, 1.0]])
        g1, g2 = pose_estimator.focal_from_fundamental(FR.true_F(R, t, K1, K2), pp1, pp2)
        worst = max(worst, abs(g1 / f1 - 1.0), abs(g2 / f2 - 1.0))
    print(f"Bougnoux on the exact F of 200 poses: worst relative error {worst:.2e}")
    assert worst <= 1e-8


def test_focal_from_fundamental_says_nan_for_a_negative_square():
    """The exact F of a pair read with principal points 400 px off makes one squared focal length negative; a pure sideways
    translation (parallel optical axes, which intersect at infinity) has a vanishing denominator."""
    R, t = RP.make_pose(np.random.default_rng(1))
    F = FR.true_F(R, t)
    ok = pose_estimator.focal_from_fundamental(F, (640.0, 360.0), (640.0, 360.0))
    assert all(np.isfinite(ok))
    seen_nan = False
    for off in ((400.0, 0.0), (-400.0, 0.0), (0.0, 400.0), (0.0, -400.0), (900.0, 900.0), (-900.0, -900.0)):
        g = pose_estimator.focal_from_fundamental(F, (640.0 + off[0], 360.0 + off[1]), (640.0 - off[0], 360.0 - off[1]))
        assert all(np.isnan(x) or x > 0.0 for x in g)
        seen_nan = seen_nan or any(np.isnan(x) for x in g)
    assert seen_nan
    g = pose_estimator.focal_from_fundamental(FR.true_F(np.eye(3), np.array([1.0, 0.0, 0.0])), (640.0, 360.0), (640.0, 360.0))
    assert all(np.isnan(x) for x in g)


# ---------------------------------------------------------------------------------------------------- (e) the helpers on a stub
class _StubSolver:
    """Records what the helpers pass on; answers with fixed arrays of the library's shapes."""

    def __init__(self, n_f=10, n_h=3):
        self.calls, self.n_f, self.n_h, self.closed = [], n_f, n_h, False

    def close(self):
        self.closed = True

    def fundamental(self, pts1, pts2, pair_off=None, **opts):
        self.calls.append(("fundamental", np.asarray(pts1), np.asarray(pts2), pair_off, opts))
        n = len(pts1)
        inl = np.zeros(n, dtype=bool)
        inl[:self.n_f] = True
        return dict(F=np.arange(9.0).reshape(1, 3, 3), status=np.array([0], dtype=np.uint8), n_inliers=np.array([self.n_f], dtype=np.int32),
                    rms_px=np.array([0.5]), best_hyp=np.array([4], dtype=np.int32), match_inlier=inl, epipole1=np.ones((1, 3)),
                    epipole2=np.full((1, 3), 2.0))

    def homography(self, K, pts1, pts2, pair_off=None, **opts):
        self.calls.append(("homography", np.asarray(K), np.asarray(pts1), np.asarray(pts2), opts))
        n = len(pts1)
        return dict(H=np.eye(3)[None], status=np.array([0], dtype=np.uint8), n_inliers=np.array([self.n_h], dtype=np.int32), rms_px=np.array([0.1]),
                    best_hyp=np.array([0], dtype=np.int32), n_pose=np.array([1], dtype=np.int32), match_inlier=np.zeros(n, dtype=bool),
                    R=np.zeros((1, 2, 3, 3)), t=np.zeros((1, 2, 3)), normal=np.zeros((1, 2, 3)), t_over_d=np.zeros((1, 2)),
                    votes=np.zeros((1, 2), dtype=np.int32), pose_cost=np.zeros((1, 2)))

    def match_guided(self, sets, keypoints, pairs=None, *, window=None, fundamental=None, **opts):
        self.calls.append(("match_guided", sets, keypoints, window, fundamental, opts))
        n = len(sets[0])
        return dict(row_off=np.array([0, n]), best=np.arange(n, dtype=np.int32), second=np.zeros(n, dtype=np.int32), dist1=np.full(n, 7, dtype=np.int32),
                    dist2=np.full(n, 9, dtype=np.int32), good=np.arange(n) % 2 == 0, n_good=np.array([(n + 1) // 2], dtype=np.int32))


class _Match:
    def __init__(self, q, t):
        self.queryIdx, self.trainIdx = q, t


class _KeyPoint:
    def __init__(self, pt):
        self.pt = (float(pt[0]), float(pt[1]))


def test_one_pair_helper_forwards_options_and_drops_the_pair_axis():
    s = _StubSolver()
    p1, p2 = np.zeros((12, 2)), np.ones((12, 2))
    out = pose_estimator.fundamental(p1, p2, solver=s, n_hyp=77, seed=3, max_epi_px=1.5)
    name, a1, a2, off, opts = s.calls[0]
    assert name == "fundamental" and a1 is p1 and a2 is p2 and off is None and opts == dict(n_hyp=77, seed=3, max_epi_px=1.5)
    assert out["F"].shape == (3, 3) and out["epipole1"].shape == (3,) and out["epipole2"].shape == (3,) and out["match_inlier"].shape == (12,)
    assert (out["status"], out["n_inliers"], out["best_hyp"]) == (0, 10, 4) and out["rms_px"] == 0.5
    assert all(type(out[k]) is int for k in ("status", "n_inliers", "best_hyp")) and type(out["rms_px"]) is float
    assert not s.closed                            # a solver passed in is the caller's to close


def test_estimate_uncalibrated_on_the_stub():
    rng = np.random.default_rng(2)
    p1, p2 = rng.uniform(0.0, 1000.0, (12, 2)), rng.uniform(0.0, 1000.0, (12, 2))
    matches = [_Match(i, 11 - i) for i in range(12)]
    kp1, kp2 = [_KeyPoint(p) for p in p1], [_KeyPoint(p) for p in p2[::-1]]
    s = _StubSolver(n_f=10, n_h=3)
    F, i1, i2, idx, info = pose_estimator.estimate_uncalibrated(matches, kp1, kp2, solver=s, quiet=True, n_hyp=64, max_epi_px=2.0, max_px=4.0)
    (fn, f1, f2, _, fo), (hn, K0, h1, h2, ho) = s.calls
    assert fn == "fundamental" and fo == dict(n_hyp=64, max_epi_px=2.0) and hn == "homography" and ho == dict(n_hyp=64, max_px=4.0)
    assert f1.dtype == np.float32 and np.array_equal(f1, np.float32(p1)) and np.array_equal(f2, np.float32(p2)) and h1 is f1 and h2 is f2
    centre = np.concatenate([np.float32(p1), np.float32(p2)]).astype(np.float64).mean(axis=0)
    assert K0[0, 0] == K0[1, 1] > 0.0 and np.allclose(K0[:2, 2], centre) and np.array_equal(K0[2], [0.0, 0.0, 1.0]) and K0[0, 1] == K0[1, 0] == 0.0
    assert info["model"] == "fundamental" and info["unique"] and F.shape == (3, 3) and np.array_equal(idx, np.arange(10))
    assert i1.shape == i2.shape == (10, 2) and i1.dtype == np.float32
    # COLMAP's rule, at the boundary: 8 >= 0.8 * 10 is planar, 7 is not
    assert pose_estimator.estimate_uncalibrated(matches, kp1, kp2, solver=_StubSolver(10, 8), quiet=True)[4]["model"] == "planar"
    assert pose_estimator.estimate_uncalibrated(matches, kp1, kp2, solver=_StubSolver(10, 7), quiet=True)[4]["model"] == "fundamental"
    assert pose_estimator.estimate_uncalibrated(matches, kp1, kp2, solver=_StubSolver(10, 7), quiet=True, planar_ratio=0.7)[4]["model"] == "planar"
    with pytest.raises(TypeError):
        pose_estimator.estimate_uncalibrated(matches, kp1, kp2, solver=s, quiet=True, max_depth=5.0)


def test_estimate_uncalibrated_prints_and_flags_a_plane(capsys):
    matches = [_Match(i, i) for i in range(12)]
    kp = [_KeyPoint((10.0 * i, 7.0 * i)) for i in range(12)]
    F, _, _, _, info = pose_estimator.estimate_uncalibrated(matches, kp, kp, solver=_StubSolver(10, 9))
    out = capsys.readouterr().out
    assert info["model"] == "planar" and not info["unique"] and F is not None and "not unique" in out and "10 inliers out of 12" in out


def test_match_by_fundamental_passes_F_to_the_epipolar_gate():
    s = _StubSolver()
    des1, des2 = np.zeros((6, 32), dtype=np.uint8), np.ones((5, 32), dtype=np.uint8)
    kp1, kp2 = np.zeros((6, 2)), np.ones((5, 2))
    F = np.arange(9.0).reshape(3, 3)
    q, t, d = features.match_by_fundamental(des1, kp1, des2, kp2, F, max_epi_px=2.5, solver=s, ratio=0.9)
    name, sets, kps, window, Fp, opts = s.calls[0]
    assert name == "match_guided" and window is None and Fp.shape == (1, 3, 3) and np.array_equal(Fp[0], F) and opts == dict(max_epi_px=2.5, ratio=0.9)
    assert np.array_equal(q, [0, 2, 4]) and np.array_equal(t, [0, 2, 4]) and np.array_equal(d, [7, 7, 7])
    assert all(len(x) == 0 for x in features.match_by_fundamental(None, kp1, des2, kp2, F, solver=s)) and len(s.calls) == 1


def test_the_package_exports_the_new_names():
    import bundle_adjustment_amd as pkg
    assert pkg.estimate_uncalibrated is pose_estimator.estimate_uncalibrated and pkg.focal_from_fundamental is pose_estimator.focal_from_fundamental
    assert pkg.match_by_fundamental is features.match_by_fundamental and pkg.fundamental_matrix is pose_estimator.fundamental
    assert pkg.fundamental is features.fundamental               # the name the package already had stays what it was


def test_planar_scene_is_one_the_homography_explains():
    """What the GPU surface test leans on: homography_reference's exact plane with 0.3 px of noise is within 3 px of its H."""
    p1, p2, _, _, Ht = HG.noisy_plane(0)
    inl, _, _ = HG.consensus(Ht, RP.normalise(HG.K_TEST, p1), RP.normalise(HG.K_TEST, p2), 3.0 / 805.0)
    assert inl.all()
