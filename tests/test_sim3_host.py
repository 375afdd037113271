"""CPU: the numpy yardstick of ba_sim3 (tests/sim3_reference.py) checked against itself, posegraph.edge_information against a
finite-difference Hessian of the numpy edge residual, and posegraph.loop_measurement's bookkeeping (frames, K, the BAL
conjugation, the error path) against a solver double whose sim3 is the yardstick.  The figures printed here are the
reference-side columns of DESIGN.md 4t."""
import numpy as np
import pytest

from bundle_adjustment_amd import posegraph as pg
from bundle_adjustment_amd.bal import BALProblem
from bundle_adjustment_amd.hip_backend import SIM3_STATUS
from bundle_adjustment_amd.posegraph import edge_information, loop_measurement  # noqa: F401
from bundle_adjustment_amd.problem import BAProblem
from tests import posegraph_reference as PG
from tests import sim3_reference as S
from tests.fake_solver import OracleSolver

K = S.K_TEST
FLIP = np.array([1.0, -1.0, -1.0])


# ---------------------------------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("with_scale", [True, False])
def test_true_model_from_noise_free_triples(with_scale):
    scenes, refs, worst_ref = S.minimal_cases(with_scale)
    void = sum(r is None for r in refs.values())
    print(f"with_scale={with_scale}: the reference's worst distance from the truth on 8 pairs x 16 seeds {worst_ref:.2e}; {void} void of 128")
    assert worst_ref <= 1e-12 and void <= 2
    if not with_scale:
        assert all(r[2] == 1.0 for r in refs.values() if r is not None)


def test_void_samples():
    rng = np.random.default_rng(3)
    X1, X2, _ = S.exact_scene(rng, 3)
    assert S.three_point(X1, X2) is not None
    line = X1[0] + np.outer([0.0, 1.0, 2.5], X1[1] - X1[0])
    assert S.three_point(line, X2) is None and S.three_point(X1, line) is None          # collinear in either frame
    assert S.three_point(X1[[0, 0, 1]], X2[[0, 0, 1]]) is None                           # coincident
    bad = X1.copy()
    bad[1, 2] = -1.0
    assert S.three_point(bad, X2) is None                                                # behind its own camera
    bad[1, 2] = np.nan
    assert S.three_point(bad, X2) is None


@pytest.mark.parametrize("with_scale", [True, False])
def test_batched_solver_and_scores_are_the_scalar_ones(with_scale):
    a, b, _ = S.noisy_scene(5, 6, 0.002, with_scale)
    X1, X2 = np.concatenate([a, a[:2]]), np.concatenate([b, b[:2]])          # two duplicates: coincident samples are void
    X1[5, 0] = np.nan
    idx = np.array([S.sample3(1, 2, h, 8) for h in range(200)])
    many = S.three_point_many(X1[idx], X2[idx], with_scale)
    one = [S.three_point(X1[list(i)], X2[list(i)], with_scale) for i in idx]
    assert [m is None for m in many] == [m is None for m in one] and 20 < sum(m is None for m in one) < 180
    live = [h for h in range(200) if one[h] is not None]
    # (two orders of the same fp64 sums: the bound the device's solver gets, 10 x the solver's own error on exact data + 1e-12)
    assert max(max(S.model_distance(many[h], one[h])) for h in live) <= 10.0 * S.minimal_cases(with_scale)[2] + 1e-12
    thr = 4.0 / S.fbar(K)
    c_many = S.msac_many([one[h] for h in live], X1, X2, thr)
    c_one = np.array([S.msac(one[h], X1, X2, thr) for h in live])
    assert np.abs(c_many - c_one).max() <= 1e-12 * c_one.max()
    cost, models = S.hypothesis_costs(K, X1, X2, pair=2, n_hyp=200, seed=1, with_scale=with_scale)
    assert np.array_equal(np.isinf(cost), [m is None for m in one])


@pytest.mark.parametrize("with_scale", [True, False])
def test_analytic_jacobians_against_central_differences(with_scale):
    X1, X2, model = S.noisy_scene(3, 40, 0.01, with_scale)
    J = S.jacobian(model, X1, X2, with_scale)
    worst = 0.0
    for h in (1e-5, 1e-6):
        Jn = np.zeros_like(J)
        for k in range(7 if with_scale else 6):
            d = np.zeros(7)
            d[k] = h
            Jn[:, :, k] = (S.residuals(S.move(model, d), X1, X2)[0] - S.residuals(S.move(model, -d), X1, X2)[0]) / (2.0 * h)
        worst = max(worst, float(np.abs(J - Jn).max()))
    print(f"with_scale={with_scale}: analytic against central differences {worst:.2e} (largest entry {np.abs(J).max():.2f})")
    assert worst <= 1e-8 * max(1.0, np.abs(J).max())
    assert np.all(J[:, 2:, 6] == 0.0)                    # the backward residual does not see the scale
    if with_scale:
        assert np.abs(J[:, :2, 6]).max() > 1e-3


def test_reference_call_recovers_the_planted_set():
    c = S.outlier_case(0.3)
    ref = c["ref"]
    print(f"d_ref {c['d_ref']}, worst planted inlier {c['worst_px']:.2f} px, rms {ref['rms_px']:.3f} px, best_hyp {ref['best_hyp']}")
    assert ref["status"] == S.OK and np.array_equal(ref["match_inlier"], ~c["planted"])
    assert max(c["d_ref"]) <= 1e-12 and c["worst_px"] < 2.0
    H = ref["hessian"]
    assert np.array_equal(H, H.T) and np.linalg.eigvalsh(H).min() > 0.0


def test_statuses_of_the_reference():
    X1, X2, model = S.noisy_scene(4, 40)
    assert S.sim3(K, X1[:3], X2[:3])["status"] == S.FEW_MATCHES
    line = X1[0] + np.outer(np.linspace(0.0, 1.0, 12), X1[1] - X1[0])
    assert S.sim3(K, line, S.forward(model, line))["status"] == S.DEGENERATE
    rng = np.random.default_rng(0)
    r = S.sim3(K, X1, X2[rng.permutation(40)], n_hyp=64)
    assert r["status"] == S.FEW_INLIERS and r["n_inliers"] < 8


# ---------------------------------------------------------------------------------------------------- edge_information
@pytest.mark.parametrize("with_scale", [True, False])
def test_edge_information_against_a_finite_difference_hessian(with_scale):
    """q(d) = 0.5 e(d)^T info e(d), e the numpy edge residual of the relative pose retract(meas, d) against meas, has the
    Hessian H / sigma^2 at d = 0 in the call's chart: second differences at h = 1e-3 (error h^2)."""
    X1, X2, model = S.noisy_scene(7, 60, 0.002, with_scale)
    H = S.hessian(K, model, X1, X2, with_scale)
    meas = np.r_[S.rvec_of(model[0]), model[1], model[2]]
    sigma = 1.7
    info = pg.edge_information(meas, H, sigma)
    assert info.shape == (7, 7) and np.array_equal(info, info.T)
    assert np.array_equal(pg.edge_information(meas[None], H[None], sigma)[0], info)
    node_i = np.r_[np.zeros(6), 1.0][None]

    def q(d):
        e = PG.edge_residual(node_i, PG.retract(meas[None], d[None]), meas[None])[0]
        return 0.5 * e @ info @ e

    h, Hfd = 1e-3, np.zeros((7, 7))
    for a in range(7):
        for b in range(7):
            ea, eb = np.eye(7)[a] * h, np.eye(7)[b] * h
            Hfd[a, b] = (q(ea + eb) - q(ea - eb) - q(eb - ea) + q(-ea - eb)) / (4.0 * h * h)
    err = float(np.abs(Hfd - H / sigma ** 2).max() / np.abs(H / sigma ** 2).max())
    print(f"with_scale={with_scale}: finite-difference Hessian of the edge cost against H / sigma^2: {err:.2e} relative")
    assert err <= 1e-5
    if not with_scale:
        assert not info[6].any() and not info[:, 6].any()


# ---------------------------------------------------------------------------------------------------- loop_measurement
class Sim3Oracle(OracleSolver):
    """fake_solver's double with the one method loop_measurement calls, answered by the numpy reference."""

    def sim3(self, K, X1, X2, pair_off=None, **opts):
        self.seen = dict(K=np.array(K), X1=np.array(X1), X2=np.array(X2), opts=dict(opts))
        r = S.sim3(K, X1, X2, **opts)
        return dict(sim=r["sim"][None], R=r["R"][None], t=r["t"][None], s=np.array([r["s"]]), status=np.array([r["status"]], dtype=np.uint8),
                    n_inliers=np.array([r["n_inliers"]], dtype=np.int32), rms_px=np.array([r["rms_px"]]),
                    best_hyp=np.array([r["best_hyp"]], dtype=np.int32), match_inlier=r["match_inlier"], hessian=r["hessian"][None])


def _revisit(bal, n=40, seed=11, mismatches=6):
    """Two cameras i = 1, j = 3 of a four-camera problem, n old map points in front of camera i and their duplicates in the
    (drifted) new map such that X_j = s R X_i + t exactly for the model returned (in the problem's own camera frames), the
    first `mismatches` duplicates paired wrongly.  -> (prob, pt_i, pt_j, model)."""
    rng = np.random.default_rng(seed)
    model = S.make_model(rng)
    Xi = S.make_points(rng, n, model)                       # pinhole frames, z forward
    Xj = S.forward(model, Xi)
    if bal:                                                 # the problem's frames look down -z
        Xi, Xj, model = Xi * FLIP, Xj * FLIP, (model[0] * np.outer(FLIP, FLIP), model[1] * FLIP, model[2])
    cams = np.zeros((4, 9 if bal else 6))
    cams[:, :3] = 0.3 * rng.normal(size=(4, 3))
    cams[:, 3:6] = rng.normal(size=(4, 3))
    if bal:
        cams[:, 6] = [500.0, 510.0, 520.0, 530.0]
    Ri, Rj = PG.rodrigues(cams[1, :3]), PG.rodrigues(cams[3, :3])
    old, new = (Xi - cams[1, 3:6]) @ Ri, (Xj - cams[3, 3:6]) @ Rj
    pts = np.concatenate([old, new])
    pt_i, pt_j = np.arange(n), n + np.arange(n)
    pt_j[:mismatches] = n + (np.arange(mismatches) + 17) % n
    obs_c, obs_p = np.zeros(2 * n, np.int32), np.arange(2 * n, dtype=np.int32)
    if bal:
        prob = BALProblem(cams, pts, obs_c, obs_p, np.zeros((2 * n, 2)))
    else:
        prob = BAProblem(cams, pts, obs_c, obs_p, np.zeros((2 * n, 2)), np.array([700.0, 720.0, 320.0, 240.0]), 0)
    return prob, pt_i, pt_j, model


@pytest.mark.parametrize("bal", [False, True])
def test_loop_measurement_bookkeeping(bal):
    prob, pt_i, pt_j, model = _revisit(bal)
    s = Sim3Oracle()
    meas, info, inlier, out = pg.loop_measurement(prob, 1, 3, pt_i, pt_j, solver=s, sigma_px=2.0, n_hyp=64, seed=3)
    assert s.seen["opts"] == dict(n_hyp=64, seed=3)
    want_K = np.diag([530.0, 530.0, 1.0]) if bal else np.array([[700.0, 0.0, 320.0], [0.0, 720.0, 240.0], [0.0, 0.0, 1.0]])
    assert np.array_equal(s.seen["K"], want_K)
    assert (s.seen["X1"][:, 2] > 0.0).all() and (s.seen["X2"][6:, 2] > 0.0).all()      # the call sees pinhole frames
    assert np.array_equal(inlier, np.r_[np.zeros(6, bool), np.ones(34, bool)]) and out["n_inliers"][0] == 34
    got = (PG.rodrigues(meas[:3]), meas[3:6], meas[6])
    d = S.model_distance(got, model)
    print(f"bal={bal}: meas against the planted model {d}")
    assert max(d) <= 1e-9
    # the same through world coordinates instead of indices
    meas2, info2, _, _ = pg.loop_measurement(prob, 1, 3, prob.pts[pt_i], prob.pts[pt_j], solver=s, sigma_px=2.0, n_hyp=64, seed=3)
    assert np.array_equal(meas, meas2) and np.array_equal(info, info2)
    # info: the Hessian of the inliers' residuals in the problem's own frames (x flips sign with the frame, |r| does not)
    Xi, Xj = pg._camera_frame(prob, 1, pt_i)[6:], pg._camera_frame(prob, 3, pt_j)[6:]
    H = S.hessian(want_K, got, Xi, Xj)
    want = pg.edge_information(meas, H, 2.0)
    err = float(np.abs(info - want).max() / np.abs(want).max())
    print(f"bal={bal}: info against the Hessian formed in the problem's frames {err:.2e} relative")
    assert err <= 1e-9 and np.array_equal(info, info.T)
    # an explicit K goes through
    pg.loop_measurement(prob, 1, 3, pt_i, pt_j, K=K, solver=s)
    assert np.array_equal(s.seen["K"], K)


def test_bal_conjugation_round_trip():
    """F (F R F) F = R, F (F t) = t, and the conjugated Hessian conjugated again is the Hessian: a BAL problem whose frames are
    the flipped pinhole ones gives the flipped measurement of its pinhole twin."""
    pin, pt_i, pt_j, model = _revisit(False)
    cams = np.zeros((4, 9))
    R = PG.rodrigues(pin.cams[:, :3]) * FLIP[None, :, None]                      # F R_c: the camera turned over
    cams[:, :3], cams[:, 3:6], cams[:, 6] = PG.log_map(R), pin.cams[:, 3:6] * FLIP, 700.0
    bal = BALProblem(cams, pin.pts, pin.cam_idx, pin.pt_idx, pin.uv)
    s = Sim3Oracle()
    Kp = np.diag([700.0, 700.0, 1.0])
    mp, ip, _, _ = pg.loop_measurement(pin, 1, 3, pt_i, pt_j, K=Kp, solver=s)
    mb, ib, _, _ = pg.loop_measurement(bal, 1, 3, pt_i, pt_j, solver=s)
    T = np.r_[FLIP, FLIP, 1.0]
    back = (PG.rodrigues(mb[:3]) * np.outer(FLIP, FLIP), mb[3:6] * FLIP, mb[6])
    d = S.model_distance(back, (PG.rodrigues(mp[:3]), mp[3:6], mp[6]))
    # info = T_e H T_e^T with T_e = diag(R_ij^T, I, 1): R_ij^T F = F (F R_ij F)^T, so the BAL info is the pinhole one conjugated
    err = float(np.abs(ib * np.outer(T, T) - ip).max() / np.abs(ip).max())
    print(f"round trip: model {d}, info {err:.2e} relative")
    assert max(d) <= 1e-12 and err <= 1e-9


def test_loop_measurement_refuses_a_bad_status_and_bad_lengths():
    prob, pt_i, pt_j, _ = _revisit(False)
    s = Sim3Oracle()
    with pytest.raises(ValueError, match="few_matches"):
        pg.loop_measurement(prob, 1, 3, pt_i[:3], pt_j[:3], solver=s)
    with pytest.raises(ValueError, match="few_inliers"):
        pg.loop_measurement(prob, 1, 3, pt_i, pt_j, solver=s, min_inliers=35)
    with pytest.raises(ValueError, match="different numbers"):
        pg.loop_measurement(prob, 1, 3, pt_i, pt_j[:-1], solver=s)


def test_exports_and_binding_tables():
    import ctypes as C

    import bundle_adjustment_amd as pkg
    from bundle_adjustment_amd import hip_backend as hb
    assert pkg.loop_measurement is pg.loop_measurement
    assert hb.SIM3_STATUS is SIM3_STATUS and SIM3_STATUS == dict(ok=S.OK, few_matches=S.FEW_MATCHES, degenerate=S.DEGENERATE, few_inliers=S.FEW_INLIERS)
    assert C.sizeof(hb.BASim3Options) == 40 and "ba_sim3" in hb.SYMBOLS and "ba_default_sim3_options" in hb.SYMBOLS
    import __graft_entry__ as g
    g.build()
    o = hb.BASim3Options()
    assert hb.load_library().ba_default_sim3_options(C.byref(o)) == 0                   # (no device needed)
    assert (o.n_hyp, o.lo_rounds, o.seed, o.max_px, o.refine_iters, o.min_inliers, o.with_scale) == (256, 2, 0, 4.0, 20, 8, 1)
