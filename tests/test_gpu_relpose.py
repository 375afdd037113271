"""GPU: ba_relative_pose (five-point RANSAC on the device) against the numpy yardstick of tests/relpose_reference.py.

Tolerances.  1e-6 on a unit-norm essential matrix (cases 1 and 2) is the bound set for the polynomial route; the yardstick's own
worst error on the same samples is printed next to the device's.  Poses after the local optimisation (cases 3 and 4) must lie
within 10 x d_ref + 1e-12 rad of the yardstick pose (the refinement of step 6 from the truth on the planted inliers), d_ref the
numpy reference's own distance to it.  The "planar" scenes carry a relief (relpose_reference.RELIEF): exactly coplanar matches
admit two essential matrices of zero cost, and choosing between them is planar model selection, which the call does not do."""
import numpy as np
import pytest

from tests import relpose_reference as R

pytestmark = pytest.mark.gpu

K = R.K_TEST
ST = dict(ok=0, few_matches=1, degenerate=2, behind=3, few_inliers=4, low_parallax=5)
OUTS = ("R", "t", "status", "n_inliers", "rms_px", "parallax_deg", "best_hyp")
COUNTS = (0, 5, 6, 7, 63, 64, 65, 255, 256, 257, 1100)


@pytest.fixture(scope="module")
def solver():
    import __graft_entry__ as g
    g.build()
    from bundle_adjustment_amd import hip_backend
    with hip_backend.Solver(0) as s:
        yield s


def _offsets(counts):
    return np.r_[0, np.cumsum(counts)].astype(np.int64)


def _close_to(r, i, yard, d_ref):
    d = R.pose_distance(r["R"][i], r["t"][i], *yard)
    return d, d[0] <= 10.0 * d_ref[0] + 1e-12 and d[1] <= 10.0 * d_ref[1] + 1e-12


# ---------------------------------------------------------------------------------------------------- 1, 2: the solver alone
@pytest.fixture(scope="module")
def minimal(solver):
    """Per scene: 8 pairs of 8 noise-free unrounded matches in one call, 16 seeds, n_hyp = 1, lo_rounds = 0."""
    out = {}
    for planar in (False, True):
        rng = np.random.default_rng(11 + planar)
        scenes = [R.make_scene(rng, 8, planar, relief=R.RELIEF if planar else 0.0) for _ in range(8)]
        p1, p2 = np.concatenate([s[0] for s in scenes]), np.concatenate([s[1] for s in scenes])
        runs = [solver.relative_pose(K, p1, p2, _offsets([8] * 8), n_hyp=1, lo_rounds=0, seed=seed) for seed in range(16)]
        out[planar] = (scenes, runs)
    return out


@pytest.mark.parametrize("planar", [False, True])
def test_solver_alone_finds_the_true_essential_matrix(minimal, planar):
    scenes, runs = minimal[planar]
    fails, worst, worst_ref = 0, 0.0, 0.0
    for seed, r in enumerate(runs):
        for p, (p1, p2, Rt, tt) in enumerate(scenes):
            Et = R.essential(Rt, tt)
            err = R.E_distance(R.essential(r["R"][p], r["t"][p]), Et) if r["status"][p] == ST["ok"] else np.inf
            good = err <= 1e-6 and r["n_inliers"][p] == 8
            fails += not good
            if good:
                worst = max(worst, err)
            idx = list(R.sample5(seed, p, 0, 8))
            worst_ref = max(worst_ref, min(R.E_distance(E, Et) for E in R.five_point(R.normalise(K, p1[idx]), R.normalise(K, p2[idx]))))
    allowed = int((0.10 if planar else 0.02) * 128)
    print(f"planar={planar}: {fails} of 128 (pair, seed) cases miss 1e-6 ({allowed} allowed); worst error of the others {worst:.2e}; "
          f"the numpy reference's worst on the same samples {worst_ref:.2e} (1e-6 is {1e-6 / worst_ref:.0f} x that)")
    assert fails <= allowed


@pytest.mark.parametrize("planar", [False, True])
def test_generator_and_solver_are_coherent_with_the_reference(minimal, planar):
    scenes, runs = minimal[planar]
    void, worst = 0, 0.0
    for seed, r in enumerate(runs):
        for p, (p1, p2, _, _) in enumerate(scenes):
            if r["status"][p] == ST["degenerate"]:
                void += 1
                assert r["best_hyp"][p] == -1
                continue
            assert r["best_hyp"][p] == 0
            idx = list(R.sample5(seed, p, r["best_hyp"][p], 8))
            Es = R.five_point(R.normalise(K, p1[idx]), R.normalise(K, p2[idx]))
            d = min(R.E_distance(E, R.essential(r["R"][p], r["t"][p])) for E in Es)
            worst = max(worst, d)
    print(f"planar={planar}: worst distance of the device's E to the nearest solution of the reference on the same sample {worst:.2e}; "
          f"{void} void")
    assert worst <= 1e-6
    assert void <= int((0.10 if planar else 0.02) * 128)


# ---------------------------------------------------------------------------------------------------- 3: outliers
@pytest.mark.parametrize("planar", [False, True])
@pytest.mark.parametrize("share", [0.3, 0.5])
def test_outcome_under_outliers(solver, planar, share):
    c = R.outlier_case(planar, share)
    r = solver.relative_pose(K, c["p1"], c["p2"], n_hyp=256)
    d, ok = _close_to(r, 0, c["yard"], c["d_ref"])
    print(f"planar={planar} share={share}: status {r['status'][0]}, {r['n_inliers'][0]} inliers ({(~c['planted']).sum()} planted), "
          f"rms {r['rms_px'][0]:.3f} px, parallax {r['parallax_deg'][0]:.2f} deg, best_hyp {r['best_hyp'][0]}; "
          f"to the yardstick: rotation {d[0]:.2e} rad, direction {d[1]:.2e} rad; d_ref {c['d_ref'][0]:.2e}, {c['d_ref'][1]:.2e}")
    assert r["status"][0] == ST["ok"]
    assert np.array_equal(r["match_inlier"], ~c["planted"]) and r["n_inliers"][0] == (~c["planted"]).sum()
    assert ok, d
    assert abs(np.linalg.norm(r["t"][0]) - 1.0) <= 1e-14
    ref = c["ref"]
    # (a pose within 1e-11 rad moves a residual by 1e-8 px at 800 px of focal length)
    assert abs(r["rms_px"][0] - ref["rms_px"]) <= 1e-6 and abs(r["parallax_deg"][0] - ref["parallax_deg"]) <= 1e-6
    inl = r["match_inlier"]
    _, valid = solver.triangulate(K, r["R"][0], r["t"][0], c["p1"][inl], c["p2"][inl])
    assert valid.all()


# ---------------------------------------------------------------------------------------------------- 4: edges of the mappings
@pytest.fixture(scope="module")
def edge_pairs():
    """Eleven pairs of one call (general scene, no mismatches), the yardstick pose of each and the reference's own distance to
    it (16 hypotheses: the minimum does not depend on their number).  The noise is 0.02 px: the cases cross n_hyp = 1, and with
    the 0.3 px of case 3 a single minimal sample need not bring the other matches within 3 px (the numpy reference with
    n_hyp = 1 ends FEW_INLIERS on the pair of 6 and on a wrong pose with 58 inliers on the pair of 1100); this case is about the
    mappings, case 3 about the outcome."""
    pairs = [R.noisy_scene(n, seed=100 + i, sigma=0.02) for i, n in enumerate(COUNTS)]
    yard, d_ref = [], []
    for i, (p1, p2, Rt, tt) in enumerate(pairs):
        if len(p1) < 6:
            yard.append(None)
            d_ref.append(None)
            continue
        yard.append(R.yardstick(K, p1, p2, Rt, tt))
        ref = R.relative_pose(K, p1, p2, pair=i, n_hyp=16, min_inliers=6)
        assert ref["status"] == R.OK and ref["n_inliers"] == len(p1)
        d_ref.append(R.pose_distance(ref["R"], ref["t"], *yard[-1]))
    return pairs, yard, d_ref


@pytest.mark.parametrize("n_hyp", [1, 15, 16, 17, 255, 256, 257, 1000])
def test_edges_of_the_mappings(solver, edge_pairs, n_hyp):
    pairs, yard, d_ref = edge_pairs
    p1, p2 = np.concatenate([p[0] for p in pairs]), np.concatenate([p[1] for p in pairs])
    off = _offsets(COUNTS)
    r = solver.relative_pose(K, p1, p2, off, n_hyp=n_hyp, min_inliers=6)
    for i, n in enumerate(COUNTS):
        sl = slice(off[i], off[i + 1])
        assert r["n_inliers"][i] == r["match_inlier"][sl].sum()
        if n < 6:
            assert r["status"][i] == ST["few_matches"] and r["best_hyp"][i] == -1 and r["n_inliers"][i] == 0
            assert np.array_equal(r["R"][i], np.eye(3)) and not r["t"][i].any() and np.isnan(r["rms_px"][i])
            continue
        d, ok = _close_to(r, i, yard[i], d_ref[i])
        print(f"n_hyp={n_hyp} n={n}: status {r['status'][i]}, {r['n_inliers'][i]} inliers, best_hyp {r['best_hyp'][i]}, to the yardstick "
              f"{d[0]:.2e} {d[1]:.2e} rad (d_ref {d_ref[i][0]:.2e} {d_ref[i][1]:.2e})")
        assert r["status"][i] == ST["ok"]
        assert 0 <= r["best_hyp"][i] < n_hyp
        assert ok, (n, d, d_ref[i])
    # every pair alone, at its own index of the call (the samples depend on it), the other pairs empty: bit-equal
    for i, n in enumerate(COUNTS):
        alone = np.zeros(len(COUNTS) + 1, dtype=np.int64)
        alone[i + 1:] = n
        a = solver.relative_pose(K, pairs[i][0], pairs[i][1], alone, n_hyp=n_hyp, min_inliers=6)
        for k in OUTS:
            assert np.array_equal(a[k][i], r[k][i], equal_nan=True), (n, k)
        assert np.array_equal(a["match_inlier"], r["match_inlier"][off[i]:off[i + 1]])


# ---------------------------------------------------------------------------------------------------- 5: statuses and errors
def test_statuses(solver):
    c = R.outlier_case(False, 0.3)
    same = np.tile([[400.0, 300.0]], (20, 1))
    r = solver.relative_pose(K, same, same + 3.0)
    assert r["status"][0] == ST["degenerate"] and np.array_equal(r["R"][0], np.eye(3)) and not r["t"][0].any()
    assert r["n_inliers"][0] == 0 and r["best_hyp"][0] == -1 and np.isnan(r["rms_px"][0]) and not r["match_inlier"].any()
    r = solver.relative_pose(K, c["p1"], c["p2"], min_inliers=250)
    assert r["status"][0] == ST["few_inliers"] and r["n_inliers"][0] == (~c["planted"]).sum()
    r = solver.relative_pose(K, c["p1"], c["p2"], max_depth=1e-3)
    assert r["status"][0] == ST["behind"] and r["n_inliers"][0] == 0
    # a pure rotation (pixel noise as in case 3): no finite depths, so the depth limit is lifted; the parallax is the noise's
    rng = np.random.default_rng(9)
    p1, _, Rt, _ = R.make_scene(rng, 300)
    Y = np.c_[R.normalise(K, p1), np.ones(300)] @ Rt.T
    p2 = ((Y / Y[:, 2:]) @ K.T)[:, :2] + R.truncated_noise(rng, (300, 2))
    r = solver.relative_pose(K, p1 + R.truncated_noise(rng, (300, 2)), p2, min_parallax_deg=0.5, max_depth=0.0)
    print(f"pure rotation: status {r['status'][0]}, {r['n_inliers'][0]} inliers, parallax {r['parallax_deg'][0]:.4f} deg, "
          f"rotation error {R.pose_distance(r['R'][0], np.ones(3), Rt, np.ones(3))[0]:.2e} rad")
    assert r["status"][0] == ST["low_parallax"] and r["parallax_deg"][0] < 0.5


def test_invalid_arguments_name_their_field(solver):
    from bundle_adjustment_amd import hip_backend as hb
    c = R.outlier_case(False, 0.3)
    p1, p2, n = c["p1"], c["p2"], len(c["p1"])

    def refused(word, Km=K, off=None, **opts):
        with pytest.raises(hb.BAHipError) as e:
            solver.relative_pose(Km, p1, p2, off, **opts)
        assert word in str(e.value) and word.encode() in hb.load_library().ba_last_error(), (word, str(e.value))

    for bad in (0, 4097):
        refused("n_hyp", n_hyp=bad)
    refused("lo_rounds", lo_rounds=-1)
    for bad in (0.0, -1.0, float("nan")):
        refused("max_epi_px", max_epi_px=bad)
    refused("refine_iters", refine_iters=-1)
    refused("min_inliers", min_inliers=-1)
    refused("pair_off", off=np.array([0, 200, 100, n]))
    refused("pair_off[0]", off=np.array([1, n]))
    refused("n_pairs", off=np.r_[np.zeros(65536, dtype=np.int64), n])
    for Kb in (np.array([[800.0, 1.0, 640.0], [0, 800.0, 360.0], [0, 0, 1.0]]), np.diag([0.0, 800.0, 1.0]), np.diag([800.0, -1.0, 1.0]),
               np.array([[800.0, 0, 640.0], [0, 800.0, 360.0], [0, 0, 2.0]])):
        refused("K", Km=Kb)
    r = solver.relative_pose(K, np.zeros((0, 2)), np.zeros((0, 2)), np.zeros(1, dtype=np.int64))     # n_pairs = 0: a no-op
    assert r["R"].shape == (0, 3, 3) and r["match_inlier"].shape == (0,)


# ---------------------------------------------------------------------------------------------------- 6: reproducibility
def test_reproducible_and_leaves_a_resident_problem_alone(solver):
    from bundle_adjustment_amd.synthetic import make_problem
    c = R.outlier_case(True, 0.5)
    prob = make_problem(6, 200, 4, seed=3)
    solver.set_problem(prob)
    cams0, pts0 = solver.get_params()
    cost0 = solver.residuals("huber", want_vector=False)[2]
    a = solver.relative_pose(K, c["p1"], c["p2"])
    b = solver.relative_pose(K, c["p1"], c["p2"])
    for k in OUTS + ("match_inlier",):
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    other = solver.relative_pose(K, c["p1"], c["p2"], seed=1)
    assert other["best_hyp"][0] != a["best_hyp"][0] or not np.array_equal(other["R"], a["R"])
    assert np.array_equal(other["match_inlier"], a["match_inlier"]) and np.array_equal(a["match_inlier"], ~c["planted"])
    cams1, pts1 = solver.get_params()
    assert np.array_equal(cams0, cams1) and np.array_equal(pts0, pts1)
    assert solver.residuals("huber", want_vector=False)[2] == cost0


# ---------------------------------------------------------------------------------------------------- 7: the drop-in
class _Match:
    def __init__(self, q, t):
        self.queryIdx, self.trainIdx = q, t


class _KeyPoint:
    def __init__(self, pt):
        self.pt = (float(pt[0]), float(pt[1]))


def test_estimate_pose_then_triangulate(solver, capsys):
    """The loop of pipeline.process_frame without cv2: matches -> estimate_pose -> triangulate_points."""
    from bundle_adjustment_amd import estimate_pose
    from bundle_adjustment_amd.triangulation import triangulate_points
    c = R.outlier_case(False, 0.3)
    n = len(c["p1"])
    kp1, kp2 = [_KeyPoint(p) for p in c["p1"]], [_KeyPoint(p) for p in c["p2"][::-1]]
    matches = [_Match(i, n - 1 - i) for i in range(n)]
    Rr, tr, i1, i2, idx = estimate_pose(matches, kp1, kp2, K, solver=solver)
    lines = capsys.readouterr().out.splitlines()
    assert lines == [f"    -> Pose Estimation: {len(idx)} inliers out of {n} matches (Ratio: {len(idx) / n:.2f})"]
    assert np.array_equal(idx, np.nonzero(~c["planted"])[0])          # float32 pixels move nothing across the 3 px threshold
    assert Rr.shape == (3, 3) and tr.shape == (3, 1) and i1.dtype == np.float32
    d = R.pose_distance(Rr, tr.ravel(), *c["yard"])
    assert max(d) <= 1e-6                                             # float32 pixels are off by <= 3e-5 px: 4e-8 rad at 800 px of focal length
    xyz, kept = triangulate_points(K, Rr, tr, i1, i2, solver=solver, quiet=True)
    assert len(kept) == len(idx) and (xyz[2] > 0).all()
    assert estimate_pose(matches[:5], kp1, kp2, K, solver=solver) == (None,) * 5
