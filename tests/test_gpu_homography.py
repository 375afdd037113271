"""GPU: ba_homography (four-point RANSAC, refinement and decomposition on the device) against the numpy yardstick of
tests/homography_reference.py.

Tolerances, on H~ at unit Frobenius norm and det > 0 (recovered from the call's pixel H as K^-1 H K).  The solver alone and its
coherence with the reference: 100 x the reference's own worst error against the true H~ on the same samples + 1e-12 (two fp64
routes to one null vector differ by conditioning, not by algorithm).  After the local optimisation: 10 x d_ref + 1e-12 of the
yardstick (the refinement of step 5 from the truth on the true inliers), d_ref the numpy reference's own distance to it.  The
measured figures are in DESIGN.md 4p."""
import numpy as np
import pytest

from bundle_adjustment_amd.hip_backend import HOMOGRAPHY_STATUS
from tests import homography_reference as H
from tests import relpose_reference as R

pytestmark = pytest.mark.gpu

K = H.K_TEST
ST = HOMOGRAPHY_STATUS
OUTS = ("H", "status", "n_inliers", "rms_px", "best_hyp", "n_pose", "R", "t", "normal", "t_over_d", "votes", "pose_cost")
COUNTS = (0, 3, 4, 5, 0, 255, 256, 0, 257, 0, 1100)      # eleven pairs, empty ones between
DRAWS = range(12)


@pytest.fixture(scope="module")
def solver():
    import __graft_entry__ as g
    g.build()
    from bundle_adjustment_amd import hip_backend
    with hip_backend.Solver(0) as s:
        yield s


def _offsets(counts):
    return np.r_[0, np.cumsum(counts)].astype(np.int64)


def _Hn(r, i=0):
    return H.normalised_H(K, r["H"][i])


# ---------------------------------------------------------------------------------------------------- the solver alone
@pytest.fixture(scope="module")
def minimal(solver):
    """8 pairs of 8 noise-free unrounded matches on the exact plane in one call, 16 seeds, n_hyp = 1, lo_rounds = 0; per (seed,
    pair) the reference's solution on the sample its generator drew (None: void)."""
    rng = np.random.default_rng(21)
    scenes = [H.plane_scene(rng, 8) for _ in range(8)]
    p1, p2 = np.concatenate([s[0] for s in scenes]), np.concatenate([s[1] for s in scenes])
    runs = [solver.homography(K, p1, p2, _offsets([8] * 8), n_hyp=1, lo_rounds=0, seed=seed) for seed in range(16)]
    refs = {}
    for seed in range(16):
        for p, s in enumerate(scenes):
            idx = list(H.sample4(seed, p, 0, 8))
            refs[seed, p] = H.four_point(R.normalise(K, s[0][idx]), R.normalise(K, s[1][idx]))
    worst_ref = max(H.H_distance(Hr, scenes[p][4]) for (_, p), Hr in refs.items() if Hr is not None)
    return scenes, runs, refs, worst_ref


def test_solver_alone_finds_the_true_homography(minimal):
    scenes, runs, refs, worst_ref = minimal
    bound = 100.0 * worst_ref + 1e-12
    worst, void = 0.0, 0
    for seed, r in enumerate(runs):
        for p, s in enumerate(scenes):
            assert r["best_hyp"][p] == (-1 if refs[seed, p] is None else 0), (seed, p)
            if refs[seed, p] is None:
                void += 1
                assert r["status"][p] == ST["degenerate"] and np.array_equal(r["H"][p], np.eye(3)) and r["n_pose"][p] == 0
                continue
            assert r["status"][p] in (ST["ok"], ST["ambiguous"]) and r["n_inliers"][p] == 8
            worst = max(worst, H.H_distance(_Hn(r, p), s[4]))
    print(f"worst distance of the device's H~ to the true homography {worst:.2e}; the numpy reference's worst on the same samples "
          f"{worst_ref:.2e}; bound {bound:.2e}; {void} void of 128")
    assert worst <= bound
    assert void <= 2


def test_generator_and_solver_are_coherent_with_the_reference(minimal):
    scenes, runs, refs, worst_ref = minimal
    bound = 100.0 * worst_ref + 1e-12
    worst, worst_dlt = 0.0, 0.0
    for seed, r in enumerate(runs):
        for p, s in enumerate(scenes):
            if refs[seed, p] is None:
                continue
            worst = max(worst, H.H_distance(_Hn(r, p), refs[seed, p]))
            idx = list(H.sample4(seed, p, 0, 8))
            worst_dlt = max(worst_dlt, H.H_distance(_Hn(r, p), H.four_point_dlt(R.normalise(K, s[0][idx]), R.normalise(K, s[1][idx]))))
    print(f"worst distance of the device's H~ to the reference's closed form on the sample the reference's generator drew {worst:.2e}, "
          f"to its DLT null vector {worst_dlt:.2e}; bound {bound:.2e}")
    assert worst <= bound and worst_dlt <= bound


# ---------------------------------------------------------------------------------------------------- outliers
@pytest.mark.parametrize("share", [0.3, 0.5])
def test_outcome_under_outliers(solver, share):
    c = H.outlier_case(share)
    r = solver.homography(K, c["p1"], c["p2"], n_hyp=256)
    d = H.H_distance(_Hn(r), c["yard"])
    bound = 10.0 * c["d_ref"] + 1e-12
    ref = c["ref"]
    print(f"share={share}: status {r['status'][0]}, {r['n_inliers'][0]} inliers ({(~c['planted']).sum()} planted), rms {r['rms_px'][0]:.3f} px, "
          f"best_hyp {r['best_hyp'][0]} (reference {ref['best_hyp']}), votes {r['votes'][0]} (reference {ref['votes']}); H~ to the "
          f"yardstick {d:.2e}, d_ref {c['d_ref']:.2e}, bound {bound:.2e}")
    assert r["status"][0] == ref["status"] == ST["ok"]
    assert np.array_equal(r["match_inlier"], ~c["planted"]) and r["n_inliers"][0] == (~c["planted"]).sum()
    assert d <= bound
    assert abs(np.linalg.norm(r["H"][0]) - 1.0) <= 1e-15 and np.linalg.det(r["H"][0]) > 0.0
    assert abs(r["rms_px"][0] - ref["rms_px"]) <= 1e-6          # (an H~ within 1e-12 moves a residual by 1e-9 px)
    assert np.array_equal(r["votes"][0], ref["votes"]) and r["n_pose"][0] == ref["n_pose"]
    assert max(R.pose_distance(r["R"][0, 0], r["t"][0, 0], ref["R"][0], ref["t"][0])) <= 1e-9
    assert abs(np.linalg.norm(r["t"][0, 0]) - 1.0) <= 1e-14 and abs(np.linalg.norm(r["normal"][0, 0]) - 1.0) <= 1e-14
    inl = r["match_inlier"]
    _, valid = solver.triangulate(K, r["R"][0, 0], r["t"][0, 0], c["p1"][inl], c["p2"][inl])
    assert valid.all()


# ---------------------------------------------------------------------------------------------------- edges of the mappings
@pytest.fixture(scope="module")
def edge_pairs():
    """Eleven pairs of one call (the exact plane, 0.02 px of noise, no mismatches: the cases cross n_hyp = 1, where a single
    four-point sample has to bring every other match within 3 px), the yardstick H~ of each and the reference's own distance to
    it (16 hypotheses: the minimum does not depend on their number)."""
    pairs = [H.noisy_plane(200 + i, n, 0.02) for i, n in enumerate(COUNTS)]
    yard, d_ref = [], []
    for i, (p1, p2, _, _, Ht) in enumerate(pairs):
        if len(p1) < 5:
            yard.append(None)
            d_ref.append(None)
            continue
        yard.append(H.yardstick(K, p1, p2, Ht))
        ref = H.homography(K, p1, p2, pair=i, n_hyp=16, min_inliers=5)
        assert ref["status"] in (H.OK, H.AMBIGUOUS) and ref["n_inliers"] == len(p1)
        d_ref.append(H.H_distance(ref["Hn"], yard[-1]))
    return pairs, yard, d_ref


@pytest.mark.parametrize("n_hyp", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_edges_of_the_mappings(solver, edge_pairs, n_hyp):
    pairs, yard, d_ref = edge_pairs
    p1, p2 = np.concatenate([p[0] for p in pairs]), np.concatenate([p[1] for p in pairs])
    off = _offsets(COUNTS)
    r = solver.homography(K, p1, p2, off, n_hyp=n_hyp, min_inliers=5)
    again = solver.homography(K, p1, p2, off, n_hyp=n_hyp, min_inliers=5)
    for k in OUTS + ("match_inlier",):
        assert np.array_equal(r[k], again[k], equal_nan=True), k
    for i, n in enumerate(COUNTS):
        sl = slice(off[i], off[i + 1])
        assert r["n_inliers"][i] == r["match_inlier"][sl].sum()
        if n < 5:
            assert r["status"][i] == ST["few_matches"] and r["best_hyp"][i] == -1 and r["n_inliers"][i] == 0 and r["n_pose"][i] == 0
            assert np.array_equal(r["H"][i], np.eye(3)) and np.isnan(r["rms_px"][i]) and not r["t"][i].any() and not r["votes"][i].any()
            continue
        d = H.H_distance(_Hn(r, i), yard[i])
        print(f"n_hyp={n_hyp} n={n}: status {r['status'][i]}, {r['n_inliers'][i]} inliers, best_hyp {r['best_hyp'][i]}, votes {r['votes'][i]}, "
              f"H~ to the yardstick {d:.2e} (d_ref {d_ref[i]:.2e})")
        assert r["status"][i] in (ST["ok"], ST["ambiguous"]) and r["n_inliers"][i] == n
        assert 0 <= r["best_hyp"][i] < n_hyp
        assert d <= 10.0 * d_ref[i] + 1e-12, (n, d, d_ref[i])
    # every pair alone, at its own index of the call (the samples depend on it), the other pairs empty: bit-equal
    for i, n in enumerate(COUNTS):
        alone = np.zeros(len(COUNTS) + 1, dtype=np.int64)
        alone[i + 1:] = n
        a = solver.homography(K, pairs[i][0], pairs[i][1], alone, n_hyp=n_hyp, min_inliers=5)
        for k in OUTS:
            assert np.array_equal(a[k][i], r[k][i], equal_nan=True), (n, k)
        assert np.array_equal(a["match_inlier"], r["match_inlier"][off[i]:off[i + 1]])


def test_reproducible_and_leaves_a_resident_problem_alone(solver):
    from bundle_adjustment_amd.synthetic import make_problem
    c = H.outlier_case(0.5)
    prob = make_problem(6, 200, 4, seed=3)
    solver.set_problem(prob)
    cams0, pts0 = solver.get_params()
    cost0 = solver.residuals("huber", want_vector=False)[2]
    out0 = solver.solve(loss="huber", max_iters=5)
    a = solver.homography(K, c["p1"], c["p2"])
    b = solver.homography(K, c["p1"], c["p2"])
    for k in OUTS + ("match_inlier",):
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    other = solver.homography(K, c["p1"], c["p2"], seed=1)
    assert other["best_hyp"][0] != a["best_hyp"][0] or not np.array_equal(other["H"], a["H"])
    assert np.array_equal(other["match_inlier"], a["match_inlier"])
    solver.set_params(cams0, pts0)
    assert solver.residuals("huber", want_vector=False)[2] == cost0
    out1 = solver.solve(loss="huber", max_iters=5)
    assert out1["final_cost"] == out0["final_cost"] and out1["iterations"] == out0["iterations"]


# ---------------------------------------------------------------------------------------------------- statuses and errors
def test_statuses(solver):
    c = H.outlier_case(0.3)
    r = solver.homography(K, c["p1"][:4], c["p2"][:4])
    assert r["status"][0] == ST["few_matches"] and r["best_hyp"][0] == -1 and not r["match_inlier"].any()
    # every match of the first view on one line: every sample holds a collinear triple
    line = np.c_[np.linspace(100.0, 1100.0, 40), np.linspace(80.0, 600.0, 40)]
    r = solver.homography(K, line, c["p2"][:40])
    assert r["status"][0] == ST["degenerate"] and np.array_equal(r["H"][0], np.eye(3)) and r["best_hyp"][0] == -1
    assert r["n_inliers"][0] == 0 and np.isnan(r["rms_px"][0]) and r["n_pose"][0] == 0 and not r["match_inlier"].any()
    r = solver.homography(K, c["p1"], c["p2"], min_inliers=250)
    assert r["status"][0] == ST["few_inliers"] and r["n_inliers"][0] == (~c["planted"]).sum() and r["n_pose"][0] >= 1
    assert solver.homography(K, c["p1"], c["p2"])["status"][0] == ST["ok"]
    # draw 2 of the exact plane: the second pose gets every vote too; a ratio of 0 makes any plane with a voted pose ambiguous
    p1, p2 = H.noisy_plane(2)[:2]
    r = solver.homography(K, p1, p2)
    assert r["status"][0] == ST["ambiguous"] and r["n_pose"][0] == 2 and np.array_equal(r["votes"][0], [300, 300])
    assert solver.homography(K, c["p1"], c["p2"], ambiguity_ratio=0.0)["status"][0] == ST["ambiguous"]
    p1, p2, Rt = H.rotation_scene(0)
    r = solver.homography(K, p1, p2)
    ang = R.pose_distance(r["R"][0, 0], np.ones(3), Rt, np.ones(3))[0]
    print(f"pure rotation: status {r['status'][0]}, {r['n_inliers'][0]} inliers, (d1 - d3) / d2 = {r['t_over_d'][0, 0]:.2e}, rotation error {ang:.2e} rad")
    assert r["status"][0] == ST["rotation"] and r["n_pose"][0] == 1 and r["n_inliers"][0] == 300
    assert not r["t"][0].any() and not r["normal"][0].any() and 0.0 < r["t_over_d"][0, 0] <= H.MIN_TRANSLATION
    assert ang <= 2e-3                            # 0.3 px of noise at 800 px of focal length: 4e-4 rad per match
    assert solver.homography(K, p1, p2, min_translation=0.0)["status"][0] != ST["rotation"]


def test_invalid_arguments_name_their_field(solver):
    from bundle_adjustment_amd import hip_backend as hb
    c = H.outlier_case(0.3)
    p1, p2, n = c["p1"], c["p2"], len(c["p1"])

    def refused(word, Km=K, off=None, **opts):
        with pytest.raises(hb.BAHipError) as e:
            solver.homography(Km, p1, p2, off, **opts)
        assert word in str(e.value) and word.encode() in hb.load_library().ba_last_error(), (word, str(e.value))

    for bad in (0, 4097):
        refused("n_hyp", n_hyp=bad)
    refused("lo_rounds", lo_rounds=-1)
    for bad in (0.0, -1.0, float("nan")):
        refused("max_px", max_px=bad)
    refused("refine_iters", refine_iters=-1)
    refused("min_inliers", min_inliers=-1)
    for bad in (-0.1, 1.5, float("nan")):
        refused("ambiguity_ratio", ambiguity_ratio=bad)
    for bad in (-1e-3, float("nan")):
        refused("min_translation", min_translation=bad)
    refused("pair_off", off=np.array([0, 200, 100, n]))
    refused("pair_off[0]", off=np.array([1, n]))
    refused("n_pairs", off=np.r_[np.zeros(65536, dtype=np.int64), n])
    for Kb in (np.array([[800.0, 1.0, 640.0], [0, 800.0, 360.0], [0, 0, 1.0]]), np.diag([0.0, 800.0, 1.0]), np.diag([800.0, -1.0, 1.0]),
               np.array([[800.0, 0, 640.0], [0, 800.0, 360.0], [0, 0, 2.0]])):
        refused("K", Km=Kb)
    r = solver.homography(K, np.zeros((0, 2)), np.zeros((0, 2)), np.zeros(1, dtype=np.int64))     # n_pairs = 0: a no-op
    assert r["H"].shape == (0, 3, 3) and r["R"].shape == (0, 2, 3, 3) and r["match_inlier"].shape == (0,)


# ---------------------------------------------------------------------------------------------------- decomposition
@pytest.fixture(scope="module")
def plane_draws(solver):
    """The 12 draws of the exact plane (300 matches, 0.3 px of truncated noise) in one call, and the reference on each."""
    draws = [H.noisy_plane(seed) for seed in DRAWS]
    p1, p2 = np.concatenate([d[0] for d in draws]), np.concatenate([d[1] for d in draws])
    r = solver.homography(K, p1, p2, _offsets([300] * 12))
    refs = [H.homography(K, d[0], d[1], pair=i) for i, d in enumerate(draws)]
    return draws, r, refs


def test_decomposition_returns_the_truth_or_says_ambiguous(plane_draws):
    """Either the first pose is the truth, or the status is AMBIGUOUS and the truth is one of the two.  "The truth" up to the
    noise: within 0.05 rad in rotation and direction (the other pose of the plane lies 0.29 rad and more away, the noise moves
    the estimate by 0.007 rad at most in these draws)."""
    draws, r, refs = plane_draws
    amb = []
    for i, (_, _, Rt, tt, _) in enumerate(draws):
        d = [R.pose_distance(r["R"][i, k], r["t"][i, k], Rt, tt) for k in range(2)]
        n_true = H.true_plane_pose(Rt, tt)[2]
        print(f"draw {i}: status {r['status'][i]} (reference {refs[i]['status']}), votes {r['votes'][i]} (reference {refs[i]['votes']}), "
              f"first pose {d[0][0]:.1e} {d[0][1]:.1e} rad, second {d[1][0]:.1e} {d[1][1]:.1e} rad from the truth")
        assert r["status"][i] in (ST["ok"], ST["ambiguous"]) and r["status"][i] == refs[i]["status"]
        assert np.array_equal(r["votes"][i], refs[i]["votes"]) and r["n_pose"][i] == refs[i]["n_pose"] and r["n_inliers"][i] == 300
        hit = [max(x) <= 0.05 for x in d]
        if r["status"][i] == ST["ok"]:
            assert hit[0] and r["votes"][i, 1] < 0.75 * r["votes"][i, 0]
        else:
            amb.append(i)
            assert hit[0] or hit[1]
            assert r["votes"][i, 1] >= 0.75 * r["votes"][i, 0]
        k = 0 if hit[0] else 1
        assert np.arccos(min(1.0, float(r["normal"][i, k] @ n_true))) <= 0.05
        assert abs(r["t_over_d"][i, k] - R.BASELINE * np.linalg.norm(H.PLANE_N) / H.PLANE_D) <= 0.01
        assert r["votes"][i, 0] >= r["votes"][i, 1] and np.all(r["pose_cost"][i] > 0.0)
        for k in range(2):
            assert max(R.pose_distance(r["R"][i, k], r["t"][i, k], refs[i]["R"][k], refs[i]["t"][k])) <= 1e-9
            assert abs(r["pose_cost"][i, k] - refs[i]["pose_cost"][k]) <= 1e-9 * refs[i]["pose_cost"][k]
    print(f"AMBIGUOUS draws: {amb}")
    assert {1, 2, 6} <= set(amb)                  # the draws whose second pose gets every vote without noise


# ---------------------------------------------------------------------------------------------------- the drop-ins
class _Match:
    def __init__(self, q, t):
        self.queryIdx, self.trainIdx = q, t


class _KeyPoint:
    def __init__(self, pt):
        self.pt = (float(pt[0]), float(pt[1]))


def _as_matches(p1, p2):
    n = len(p1)
    return [_Match(i, n - 1 - i) for i in range(n)], [_KeyPoint(p) for p in p1], [_KeyPoint(p) for p in p2[::-1]]


def test_estimate_two_view_on_planes(solver, plane_draws):
    """Pixels rounded to float32 first (estimate_two_view's arithmetic), so the yardstick sees the numbers the device sees; an
    H~ within 1e-12 of the yardstick decomposes to a pose within 1e-11 rad of the yardstick's: 1e-9."""
    from bundle_adjustment_amd import estimate_two_view
    draws, r, _ = plane_draws
    seen = 0
    for i, (p1, p2, Rt, tt, Ht) in enumerate(draws):
        if r["status"][i] != ST["ok"]:
            continue
        p1, p2 = np.float64(np.float32(p1)), np.float64(np.float32(p2))
        Rr, tr, i1, i2, idx, info = estimate_two_view(*_as_matches(p1, p2), K, solver=solver, quiet=True)
        yard = H.yardstick(K, p1, p2, Ht)
        x1, x2 = R.normalise(K, p1), R.normalise(K, p2)
        dec = H.decompose(yard, x1, x2, np.ones(300, dtype=bool), 3.0 / 805.0, 50.0, H.MIN_TRANSLATION, 0.75)
        d = R.pose_distance(Rr, tr.ravel(), dec["R"][0], dec["t"][0])
        print(f"draw {i}: model {info['model']}, {len(idx)} inliers, pose to the yardstick's {d[0]:.2e} {d[1]:.2e} rad")
        assert info["model"] == "homography" and len(idx) == 300 and i1.dtype == np.float32
        assert max(d) <= 1e-9 and np.abs(info["normal"] - dec["normal"][0]).max() <= 1e-9
        assert max(R.pose_distance(Rr, tr.ravel(), Rt, tt)) <= 0.05
        seen += 1
    assert seen == (r["status"] == ST["ok"]).sum() == 8          # every draw that is not AMBIGUOUS (draws 0, 1, 2 and 6 are)


@pytest.mark.parametrize("planar", [False, True])
def test_estimate_two_view_keeps_the_essential_pose_off_the_plane(solver, planar, capsys):
    """The box scene and the desk with a relief of 0.6: few matches follow any homography, so the essential pose is returned,
    bit-equal to estimate_pose's."""
    from bundle_adjustment_amd import estimate_pose, estimate_two_view
    p1, p2, _, _ = R.noisy_scene(300, planar=planar, seed=3)
    m = _as_matches(p1, p2)
    got = estimate_two_view(*m, K, solver=solver)
    lines = capsys.readouterr().out
    want = estimate_pose(*m, K, solver=solver)
    assert capsys.readouterr().out == lines
    info = got[5]
    print(f"planar={planar}: {info['homography']['n_inliers']} homography inliers, {info['essential']['n_inliers']} essential")
    assert info["model"] == "essential" and info["homography"]["n_inliers"] < 0.8 * info["essential"]["n_inliers"]
    for a, b in zip(got[:5], want):
        assert np.array_equal(a, b) and a.dtype == b.dtype and a.shape == b.shape


def test_estimate_two_view_on_a_pure_rotation(solver):
    from bundle_adjustment_amd import estimate_two_view
    p1, p2, Rt = H.rotation_scene(1)
    Rr, tr, i1, i2, idx, info = estimate_two_view(*_as_matches(p1, p2), K, solver=solver, quiet=True)
    assert info["model"] == "rotation" and not tr.any() and len(idx) == len(i1) == len(i2) == 0
    assert R.pose_distance(Rr, np.ones(3), Rt, np.ones(3))[0] <= 2e-3


def test_match_by_homography_equals_the_hand_built_window(solver):
    from bundle_adjustment_amd import match_by_homography
    rng = np.random.default_rng(4)
    n = 150
    des1 = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    perm = rng.permutation(n)
    des2 = des1[perm].copy()
    des2[rng.random(des2.shape) < 0.02] ^= 0x10                    # a few flipped bits
    c = H.outlier_case(0.3)
    Hp = H.pixel_H(K, c["Ht"])
    kp1 = np.c_[rng.uniform(100.0, 1180.0, n), rng.uniform(100.0, 620.0, n)]
    y = H.hom(kp1) @ Hp.T
    kp2 = (y[:, :2] / y[:, 2:])[perm] + rng.uniform(-2.0, 2.0, (n, 2))     # des2[j] = des1[perm[j]]: keypoint j is the image of perm[j]
    kp2[::7] += 40.0                                               # every seventh out of the window
    got = match_by_homography(des1, kp1, des2, kp2, Hp, 5.0, solver=solver)
    window = np.c_[y[:, :2] / y[:, 2:], np.full(n, 5.0)].astype(np.float32)
    out = solver.match_guided([des1, des2], [kp1, kp2], window=window)
    good = np.nonzero(out["good"])[0]
    assert np.array_equal(got[0], good) and np.array_equal(got[1], out["best"][good]) and np.array_equal(got[2], out["dist1"][good])
    inside = np.ones(n, dtype=bool)
    inside[::7] = False
    assert 0 < len(got[0]) <= inside.sum() and np.array_equal(perm[got[1]], got[0])
    assert not np.isin(got[1], np.nonzero(~inside)[0]).any()
    wide = match_by_homography(des1, kp1, des2, kp2, Hp, 100.0, solver=solver)
    assert len(wide[0]) > len(got[0])
