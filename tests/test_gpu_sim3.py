"""GPU: ba_sim3 (three-point Sim(3) RANSAC, closed form and refinement on the device) against the numpy yardstick of
tests/sim3_reference.py, and posegraph.loop_measurement -> close_loop end to end.

Tolerances, on a model (R, t, s) as (rotation angle of Ra Rb^T, |ta - tb| / max(1, |tb|), |sa / sb - 1|).  The solver alone: 10 x the
reference's own worst distance from the truth on the same samples + 1e-12.  After the local optimisation: 10 x d_ref + 1e-12 of the
yardstick (the refinement of step 5b from the truth on the planted inliers), d_ref the reference's own distance to it, component
by component.  The Hessian: 10 x what two summation orders of the reference differ by, relative to its largest entry.  End to
end: 10 x the distance from the truth that the reference's measurement gives through the same close_loop.

Scores.  The device's best_hyp must lie among the hypotheses whose reference cost is within 1e-9 relative of the lowest, and be
the lowest index among those that drew its sample (equal values in equal order give equal bits: the lower h wins).  Where every
hypothesis of that set drew one sample the index is the reference's.  A cell (n_hyp, pair) with more than one sample in the set
is a near tie; two orderings of one triple of correspondences differ by rounding alone (and not in the same way on both sides:
the device contracts a x b + c), so a pair with n (distinct) correspondences has a near tie for certain once n_hyp reaches
its n (n - 1) (n - 2) ordered triples -- 24 for n = 4, 60 for n = 5 and for the tie pair's five distinct correspondences: no seed
avoids those cells, they are counted apart, and the cap of 5 % holds on the rest of the grid.

Scenes under mismatches: seed 5 was tried first and left one of its four draws with a planted inlier at 2.05 px (the gate is
max_px / 2 = 2); seed 6, the second tried, keeps all four below it with the planted set returned by the reference.  The measured
figures are in DESIGN.md 4t."""
import functools

import numpy as np
import pytest

from bundle_adjustment_amd import hip_backend, posegraph
from bundle_adjustment_amd.hip_backend import SIM3_STATUS
from bundle_adjustment_amd.problem import BAProblem
from bundle_adjustment_amd.synthetic import make_problem
from tests import posegraph_reference as PG
from tests import sim3_reference as S

pytestmark = pytest.mark.gpu

K = S.K_TEST
ST = SIM3_STATUS
COUNTS = (0, 3, 4, 5, 255, 256, 257, 600)
N_HYP = (1, 63, 64, 65, 255, 256, 257, 1000, 4096)
SCENE_SEED = 6


@pytest.fixture(scope="module")
def solver():
    import __graft_entry__ as g
    g.build()
    with hip_backend.Solver(0) as s:
        yield s


def _offsets(counts):
    return np.r_[0, np.cumsum(counts)].astype(np.int64)


def _model(r, i=0):
    return r["R"][i], r["t"][i], float(r["s"][i])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_result(a, b, rows=None):
    """Bit equality of two results of Solver.sim3 (NaN-safe); rows: (pairs of a, pairs of b) to compare."""
    ia, ib = (slice(None), slice(None)) if rows is None else rows
    return all(np.array_equal(bits(a[k][ia]) if a[k].dtype == np.float64 else a[k][ia], bits(b[k][ib]) if b[k].dtype == np.float64 else b[k][ib])
               for k in ("sim", "R", "t", "s", "status", "n_inliers", "rms_px", "best_hyp", "hessian"))


def assert_void(r, p, status):
    assert r["status"][p] == status and r["best_hyp"][p] == -1 and r["n_inliers"][p] == 0 and np.isnan(r["rms_px"][p])
    assert np.array_equal(r["sim"][p], np.r_[np.zeros(6), 1.0]) and np.array_equal(r["R"][p], np.eye(3)) and not r["hessian"][p].any()


# ---------------------------------------------------------------------------------------------------- 1: the solver alone
@pytest.mark.parametrize("with_scale", [True, False])
def test_solver_alone(solver, with_scale):
    scenes, refs, worst_ref = S.minimal_cases(with_scale)
    X1, X2 = np.concatenate([s[0] for s in scenes]), np.concatenate([s[1] for s in scenes])
    bound = 10.0 * worst_ref + 1e-12
    worst_truth, worst, void = 0.0, 0.0, 0
    for seed in range(16):
        r = solver.sim3(K, X1, X2, _offsets([8] * 8), n_hyp=1, lo_rounds=0, seed=seed, with_scale=with_scale)
        for p, s in enumerate(scenes):
            if refs[seed, p] is None:
                void += 1
                assert_void(r, p, ST["degenerate"])
                continue
            assert r["best_hyp"][p] == 0 and r["status"][p] == ST["ok"] and r["n_inliers"][p] == 8, (seed, p)
            worst = max(worst, *S.model_distance(_model(r, p), refs[seed, p]))
            worst_truth = max(worst_truth, *S.model_distance(_model(r, p), s[2]))
            if not with_scale:
                assert r["s"][p] == 1.0 and r["sim"][p, 6] == 1.0
    print(f"with_scale={with_scale}: the device's model against the reference's on the same sample {worst:.2e}, against the truth "
          f"{worst_truth:.2e}; the reference's worst against the truth {worst_ref:.2e}; bound {bound:.2e}; {void} void of 128")
    assert worst <= bound and worst_truth <= bound


# ---------------------------------------------------------------------------------------------------- 2: scores
@functools.lru_cache(maxsize=None)
def score_pairs():
    """The eight counts and the tie pair (five correspondences, each twice) as one call; noise of 0.002, no mismatches; the
    reference's cost of every hypothesis of every pair."""
    pairs = [S.noisy_scene(300 + i, n)[:2] if n else (np.zeros((0, 3)), np.zeros((0, 3))) for i, n in enumerate(COUNTS)]
    a, b, _ = S.noisy_scene(399, 5)
    pairs.append((np.concatenate([a, a]), np.concatenate([b, b])))
    costs = [S.hypothesis_costs(K, x1, x2, pair=p, n_hyp=max(N_HYP), max_px=4.0) if len(x1) >= 4 else None for p, (x1, x2) in enumerate(pairs)]
    return pairs, costs, [_sample_keys(x1, x2, p) if len(x1) >= 4 else None for p, (x1, x2) in enumerate(pairs)]


def _sample_keys(x1, x2, pair):
    """(n_hyp, 18): the values every hypothesis of the pair draws, in the order it draws them."""
    idx = np.array([S.sample3(0, pair, h, len(x1)) for h in range(max(N_HYP))])
    return np.concatenate([x1[idx], x2[idx]], axis=2).reshape(len(idx), -1)


def _samples(keys, hs):
    """The number of different samples among the hypotheses hs."""
    return np.unique(keys[hs], axis=0).shape[0]


def _structural(n_distinct, n_hyp):
    return n_distinct * (n_distinct - 1) * (n_distinct - 2) <= n_hyp


def test_scores(solver):
    pairs, costs, keys = score_pairs()
    X1, X2 = np.concatenate([p[0] for p in pairs]), np.concatenate([p[1] for p in pairs])
    off = _offsets([len(p[0]) for p in pairs])
    distinct = [len(p[0]) for p in pairs[:-1]] + [5]
    thr = 4.0 / S.fbar(K)
    cells = near_free = near_struct = exact_ties = 0
    worst_cost = 0.0
    for n_hyp in N_HYP:
        r = solver.sim3(K, X1, X2, off, n_hyp=n_hyp, lo_rounds=0, min_inliers=0)
        for p, (x1, x2) in enumerate(pairs):
            if len(x1) < 4:
                assert_void(r, p, ST["few_matches"])
                continue
            cost, models = costs[p]
            c = cost[:n_hyp]
            want = S.winner(c)
            assert want >= 0
            h = int(r["best_hyp"][p])
            near = np.nonzero(c <= c[want] * (1.0 + 1e-9))[0]
            cells += 1
            if _samples(keys[p], near) > 1:
                if _structural(distinct[p], n_hyp):
                    near_struct += 1
                else:
                    near_free += 1
            else:
                assert h == want, (n_hyp, p, h, want)
            same = np.nonzero((keys[p][:n_hyp] == keys[p][h]).all(1))[0]
            assert h in near and h == same[0], (n_hyp, p, h, want, same[:4])
            exact_ties += int(same.size > 1)
            d = max(S.model_distance(_model(r, p), models[h]))
            assert d <= 10.0 * S.minimal_cases(True)[2] + 1e-12, (n_hyp, p, d)
            got = S.msac(_model(r, p), x1, x2, thr)
            worst_cost = max(worst_cost, abs(got - c[h]) / c[h])
    free_cells = sum(1 for n_hyp in N_HYP for p in range(len(pairs)) if distinct[p] >= 4 and not _structural(distinct[p], n_hyp))
    print(f"{cells} cells with a winner: near ties in {near_free} of the {free_cells} free ones and in {near_struct} structural ones; "
          f"{exact_ties} cells won by a sample drawn more than once; the cost of the device's model against the reference's {worst_cost:.2e} relative")
    assert near_free <= 0.05 * free_cells
    assert worst_cost <= 1e-9
    assert same.size >= 2                  # (the last cell: the tie pair at 4096) its winner's sample was drawn again: the lower h had to win


def test_near_ties_of_the_reference_alone():
    """The cap of 5 % on the reference alone (no device): the same count as test_scores makes."""
    pairs, costs, keys = score_pairs()
    distinct = [len(p[0]) for p in pairs[:-1]] + [5]
    free = near = 0
    for n_hyp in N_HYP:
        for p, cm in enumerate(costs):
            if cm is None or _structural(distinct[p], n_hyp):
                continue
            c = cm[0][:n_hyp]
            free += 1
            near += int(_samples(keys[p], np.nonzero(c <= c.min() * (1.0 + 1e-9))[0]) > 1)
    print(f"near ties of the reference in {near} of {free} free cells")
    assert near <= 0.05 * free


# ---------------------------------------------------------------------------------------------------- 3, 4: mismatches, Hessian
@pytest.mark.parametrize("with_scale", [True, False])
@pytest.mark.parametrize("share", [0.3, 0.5])
def test_outcome_under_mismatches(solver, share, with_scale):
    c = S.outlier_case(share, with_scale, seed=SCENE_SEED)
    ref, keep = c["ref"], ~c["planted"]
    assert c["worst_px"] < 2.0 and ref["status"] == S.OK and np.array_equal(ref["match_inlier"], keep)   # the draw is one the issue keeps
    r = solver.sim3(K, c["X1"], c["X2"], n_hyp=256, with_scale=with_scale)
    d = S.model_distance(_model(r), c["yard"])
    bound = [10.0 * x + 1e-12 for x in c["d_ref"]]
    print(f"share={share} with_scale={with_scale}: status {r['status'][0]}, {r['n_inliers'][0]} inliers ({keep.sum()} planted), rms "
          f"{r['rms_px'][0]:.3f} px (reference {ref['rms_px']:.3f}), best_hyp {r['best_hyp'][0]} (reference {ref['best_hyp']}), worst planted "
          f"inlier {c['worst_px']:.2f} px; model to the yardstick {d}, d_ref {c['d_ref']}, bound {bound}")
    assert r["status"][0] == ST["ok"]
    assert np.array_equal(r["match_inlier"], keep) and r["n_inliers"][0] == keep.sum()
    assert all(x <= b for x, b in zip(d, bound))
    assert abs(r["rms_px"][0] - ref["rms_px"]) <= 1e-6
    assert np.allclose(PG.rodrigues(r["sim"][0, :3]), r["R"][0], rtol=0.0, atol=1e-14) and np.array_equal(r["sim"][0, 3:], np.r_[r["t"][0], r["s"][0]])
    if not with_scale:
        assert r["s"][0] == 1.0


@pytest.mark.parametrize("with_scale", [True, False])
def test_hessian(solver, with_scale):
    c = S.outlier_case(0.3, with_scale, seed=SCENE_SEED)
    r = solver.sim3(K, c["X1"], c["X2"], n_hyp=256, with_scale=with_scale)
    inl = r["match_inlier"]
    H = r["hessian"][0]
    a, b = c["X1"][inl], c["X2"][inl]
    want = S.hessian(K, _model(r), a, b, with_scale)
    rng = np.random.default_rng(0)
    d_order = max(float(np.abs(S.hessian(K, _model(r), a, b, with_scale, order=rng.permutation(len(a))) - want).max()) for _ in range(8))
    d_order /= np.abs(want).max()
    err = float(np.abs(H - want).max() / np.abs(want).max())
    print(f"with_scale={with_scale}: hessian against the reference's at the device's model {err:.2e} of the largest entry; two summation "
          f"orders of the reference differ by {d_order:.2e}; bound {10.0 * d_order:.2e}; eigenvalues {np.linalg.eigvalsh(H)[[0, -1]]}")
    assert np.array_equal(H, H.T)
    assert err <= 10.0 * d_order
    if with_scale:
        assert np.linalg.eigvalsh(H).min() > 0.0
    else:
        assert not H[6].any() and not H[:, 6].any() and np.linalg.eigvalsh(H[:6, :6]).min() > 0.0


# ---------------------------------------------------------------------------------------------------- 5: invalid correspondences
def test_invalid_correspondences(solver):
    X1, X2, _ = S.noisy_scene(410, 40)
    X1, X2 = X1.copy(), X2.copy()
    X1[3, 1] = np.nan
    X2[7, 2] = -X2[7, 2]
    X1[11, 2] = 0.0
    X2[19, 0] = np.inf
    bad = [3, 7, 11, 19]
    a, b, _ = S.noisy_scene(411, 4)
    forced1, forced2 = a.copy(), b.copy()
    forced1[2, 0] = np.nan                                   # every sample but (0, 1, 3) draws it
    dead1 = forced1.copy()
    dead1[0, 2] = -1.0                                       # two of four invalid: every sample is void
    allX1, allX2 = np.concatenate([X1, forced1, dead1]), np.concatenate([X2, forced2, forced2])
    off = _offsets([40, 4, 4])
    bound = 10.0 * S.minimal_cases(True)[2] + 1e-12
    for n_hyp in (1, 64):
        r = solver.sim3(K, allX1, allX2, off, n_hyp=n_hyp, lo_rounds=0, min_inliers=3)
        for p in range(2):
            x1, x2 = allX1[off[p]:off[p + 1]], allX2[off[p]:off[p + 1]]
            ref = S.sim3(K, x1, x2, pair=p, n_hyp=n_hyp, lo_rounds=0, min_inliers=3)
            inl = r["match_inlier"][off[p]:off[p + 1]]
            print(f"n_hyp={n_hyp} pair {p}: status {r['status'][p]} (reference {ref['status']}), best_hyp {r['best_hyp'][p]} (reference "
                  f"{ref['best_hyp']}), {inl.sum()} inliers (reference {ref['n_inliers']})")
            assert r["status"][p] == ref["status"] and r["best_hyp"][p] == ref["best_hyp"]
            if ref["best_hyp"] < 0:
                assert_void(r, p, ST["degenerate"])          # the one hypothesis drew an invalid correspondence
                continue
            assert np.array_equal(inl, ref["match_inlier"]) and max(S.model_distance(_model(r, p), ref["model"])) <= bound
        assert not r["match_inlier"][bad].any() and not r["match_inlier"][40 + 2]
        assert_void(r, 2, ST["degenerate"])
        assert not r["match_inlier"][44:].any()
    assert r["status"][0] == ST["ok"] and r["n_inliers"][0] == 36 and r["status"][1] == ST["ok"] and r["n_inliers"][1] == 3
    # with the refinement: the invalid ones stay out of the consensus set and of the sums
    r = solver.sim3(K, X1, X2, n_hyp=64)
    ref = S.sim3(K, X1, X2, n_hyp=64)
    d = max(S.model_distance(_model(r), ref["model"]))
    print(f"refined on 36 valid of 40: model against the reference's {d:.2e}")
    assert r["status"][0] == ST["ok"] and np.array_equal(r["match_inlier"], ref["match_inlier"]) and not r["match_inlier"][bad].any()
    assert d <= 1e-9 and np.isfinite(r["hessian"]).all()


# ---------------------------------------------------------------------------------------------------- 6: statuses
def test_each_status_occurs(solver):
    X1, X2, model = S.noisy_scene(420, 40)
    line = X1[0] + np.outer(np.linspace(0.0, 1.0, 12), X1[1] - X1[0])
    rng = np.random.default_rng(0)
    sets = [(X1, X2), (X1[:3], X2[:3]), (line, S.forward(model, line)), (X1, X2[rng.permutation(40)])]
    r = solver.sim3(K, np.concatenate([s[0] for s in sets]), np.concatenate([s[1] for s in sets]), _offsets([len(s[0]) for s in sets]), n_hyp=64)
    refs = [S.sim3(K, a, b, pair=p, n_hyp=64) for p, (a, b) in enumerate(sets)]
    print(f"statuses {r['status']} (reference {[x['status'] for x in refs]}), inliers {r['n_inliers']}")
    assert list(r["status"]) == [ST["ok"], ST["few_matches"], ST["degenerate"], ST["few_inliers"]] == [x["status"] for x in refs]
    assert_void(r, 1, ST["few_matches"])
    assert_void(r, 2, ST["degenerate"])
    assert r["n_inliers"][0] == 40 and r["n_inliers"][3] < 8 and r["best_hyp"][3] >= 0
    assert r["n_inliers"][3] == r["match_inlier"][55:].sum()


# ---------------------------------------------------------------------------------------------------- 7: invalid arguments
def test_invalid_arguments_name_the_field(solver):
    X1, X2, _ = S.noisy_scene(420, 40)

    def refused(field, K_=K, off=None, **opts):
        with pytest.raises(hip_backend.BAHipError) as err:
            solver.sim3(K_, X1, X2, off, **opts)
        assert field in str(err.value), str(err.value)

    Kbad = K.copy()
    Kbad[0, 1] = 0.1
    refused("K must be", K_=Kbad)
    Kbad = K.copy()
    Kbad[0, 0] = -1.0
    refused("K must be", K_=Kbad)
    refused("n_hyp", n_hyp=0)
    refused("n_hyp", n_hyp=4097)
    refused("lo_rounds", lo_rounds=-1)
    refused("refine_iters", refine_iters=-1)
    refused("min_inliers", min_inliers=-1)
    refused("max_px", max_px=0.0)
    refused("max_px", max_px=float("nan"))
    refused("with_scale", with_scale=2)
    refused("pair_off[0]", off=np.array([1, 40], dtype=np.int64))
    refused("pair_off decreases", off=np.array([0, 30, 20, 40], dtype=np.int64))
    import ctypes as C
    o = solver.sim3_options()
    rc = solver._lib.ba_sim3(solver._h, hip_backend._dp(np.ascontiguousarray(K)), 65536, None, None, None, C.byref(o), *([None] * 8))
    assert rc == -1 and "n_pairs" in solver._lib.ba_last_error().decode()
    rc = solver._lib.ba_sim3(solver._h, hip_backend._dp(np.ascontiguousarray(K)), 0, None, None, None, C.byref(o), *([None] * 8))
    assert rc == 0                                            # n_pairs = 0 is a no-op
    with pytest.raises(TypeError):
        solver.sim3_options(max_depth=1.0)
    with pytest.raises(ValueError):
        solver.sim3(K, X1, X2[:-1])
    assert solver.sim3(K, X1, X2, n_hyp=16)["status"][0] == ST["ok"]          # the handle is still usable


# ---------------------------------------------------------------------------------------------------- 8: reproducibility, independence
def test_bits_and_independence(solver):
    counts = (0, 3, 4, 5, 0, 255, 256, 0, 257, 0, 300)
    sets = [S.noisy_scene(430 + i, n)[:2] if n else (np.zeros((0, 3)), np.zeros((0, 3))) for i, n in enumerate(counts)]
    c = S.outlier_case(0.3, True, seed=SCENE_SEED)
    sets[10] = (c["X1"], c["X2"])
    X1, X2 = np.concatenate([s[0] for s in sets]), np.concatenate([s[1] for s in sets])
    off = _offsets(counts)
    a = solver.sim3(K, X1, X2, off, n_hyp=300)
    b = solver.sim3(K, X1, X2, off, n_hyp=300)
    assert same_result(a, b) and np.array_equal(a["match_inlier"], b["match_inlier"])
    for p in (3, 6, 10):
        alone = [0] * 11
        alone[p] = counts[p]
        r = solver.sim3(K, sets[p][0], sets[p][1], _offsets(alone), n_hyp=300)
        assert same_result(r, a, (slice(p, p + 1), slice(p, p + 1))), p
        assert np.array_equal(r["match_inlier"], a["match_inlier"][off[p]:off[p + 1]])
    print(f"two calls and three pairs alone at their index: bit-equal; statuses {a['status']}")
    # every output may be NULL
    import ctypes as C
    o = solver.sim3_options(n_hyp=300)
    p1, p2 = np.ascontiguousarray(X1), np.ascontiguousarray(X2)
    rc = solver._lib.ba_sim3(solver._h, hip_backend._dp(np.ascontiguousarray(K)), 11, off.ctypes.data_as(C.POINTER(C.c_int64)), hip_backend._dp(p1),
                             hip_backend._dp(p2), C.byref(o), *([None] * 8))
    assert rc == 0


def test_resident_problem_is_untouched(solver):
    prob = make_problem(8, 200, 4, seed=4)
    kw = dict(loss="huber", max_iters=8, small_solver=1)
    c = S.outlier_case(0.3, True, seed=SCENE_SEED)
    with hip_backend.Solver(0) as s:
        s.set_problem(prob)
        base = s.solve(**kw)
        base_params = s.get_params()
        base_trace = s.trace()
        s.set_params(prob.cams, prob.pts)
        before = s.get_params()
        assert s.sim3(K, c["X1"], c["X2"])["status"][0] == ST["ok"]
        after = s.get_params()
        assert np.array_equal(bits(before[0]), bits(after[0])) and np.array_equal(bits(before[1]), bits(after[1]))
        assert repr(s.trace()) == repr(base_trace)            # (repr round-trips a float and compares NaN as text)
        again = s.solve(**kw)
        params = s.get_params()
    assert again["final_cost"] == base["final_cost"] and again["iterations"] == base["iterations"]
    assert np.array_equal(bits(params[0]), bits(base_params[0])) and np.array_equal(bits(params[1]), bits(base_params[1]))


# ---------------------------------------------------------------------------------------------------- 9: end to end
def test_loop_measurement_closes_the_loop(solver):
    """12 cameras / 300 points on make_problem's arc; camera k moved by its own similarity D_k (the accumulated drift with a scale
    of 1 + 0.01 k, D_0 = identity), each point by the D of its first observer; odometry edges from the drifted cameras themselves
    (what covisibility_edges would measure), the loop edge (11 -> 0) from loop_measurement on the points as camera 11's map and
    camera 0's map hold them (3D noise of 0.002, 20 % of the matches wrong)."""
    prob, cams_true, pts_true = make_problem(12, 300, 4, seed=6, return_truth=True, pixel_sigma=0.0)
    n = 12
    truth = posegraph.from_cameras(cams_true)
    k = np.arange(n)[:, None]
    D = np.concatenate([k * np.array([[0.002, 0.004, -0.001]]), k * np.array([[0.03, -0.01, 0.02]]), 1.0 + 0.01 * k], axis=1)
    drifted_nodes = PG.compose(truth, PG.inverse(D))                     # S_k o D_k^-1: sees D_k X as S_k sees X
    Dp = D[posegraph.first_observers(prob.cam_idx, prob.pt_idx, 300)]
    pts = Dp[:, 6:7] * np.einsum("nij,nj->ni", PG.rodrigues(Dp[:, :3]), pts_true) + Dp[:, 3:6]
    drifted = BAProblem(posegraph.to_cameras(drifted_nodes), pts, prob.cam_idx, prob.pt_idx, prob.uv, prob.K4, 0)
    start = posegraph.from_cameras(drifted.cams)
    rng = np.random.default_rng(12)
    new_map = D[11, 6] * pts_true @ PG.rodrigues(D[11, :3]).T + D[11, 3:6] + rng.normal(scale=0.002, size=(300, 3))
    old_map = pts_true + rng.normal(scale=0.002, size=(300, 3))
    wrong = rng.choice(300, 60, replace=False)
    old_map[wrong] = old_map[np.roll(wrong, 1)]
    planted = np.zeros(300, dtype=bool)
    planted[wrong] = True
    li = np.concatenate([np.arange(n - 1), [n - 1]]).astype(np.int32)
    lj = np.concatenate([np.arange(1, n), [0]]).astype(np.int32)
    odo = PG.relative(start[li[:-1]], start[lj[:-1]])
    odo_info = np.broadcast_to(np.eye(7), (n - 1, 7, 7))
    opts = dict(loss="huber", ftol=1e-14, xtol=1e-14, gtol=1e-14, max_iters=200, pcg_tol=1e-13, pcg_max_iters=7 * n)

    def close(meas, info):
        out, fixed = posegraph.close_loop(drifted, li, lj, np.concatenate([odo, meas[None]]), loop_info=np.concatenate([odo_info, info[None]]),
                                          held=(0,), solver=solver, min_shared=10 ** 9, **opts)
        return out, PG.pose_distance(posegraph.from_cameras(fixed.cams), truth)

    meas, info, inlier, raw = posegraph.loop_measurement(drifted, 11, 0, new_map, old_map, solver=solver)
    out, d = close(meas, info)
    Xi, Xj = posegraph._camera_frame(drifted, 11, new_map), posegraph._camera_frame(drifted, 0, old_map)
    Kp = np.array([[prob.K4[0], 0.0, prob.K4[2]], [0.0, prob.K4[1], prob.K4[3]], [0.0, 0.0, 1.0]])
    ref = S.sim3(Kp, Xi, Xj)
    out_ref, d_ref = close(ref["sim"], posegraph.edge_information(ref["sim"], ref["hessian"]))
    m6, i6, _, raw6 = posegraph.loop_measurement(drifted, 11, 0, new_map, old_map, solver=solver, with_scale=False, min_inliers=0)
    out6, d6 = close(m6, i6)
    d0 = PG.pose_distance(start, truth)
    print(f"loop edge: s = {meas[6]:.6f} (drift 1 / {D[11, 6]:.2f} = {1.0 / D[11, 6]:.6f}), {inlier.sum()} inliers of 300 ({(~planted).sum()} planted), rms "
          f"{raw['rms_px'][0]:.3f} px; cameras off the truth by {d0:.3e} before, {d:.3e} after (reference's measurement {d_ref:.3e}, bound "
          f"{10.0 * d_ref:.3e}), {d6:.3e} with the SE(3) measurement ({raw6['n_inliers'][0]} inliers); loop edge weight {out['edge_weight'][-1]:.3f} "
          f"(SE(3): {out6['edge_weight'][-1]:.3f}); status {out['status_name']}")
    assert np.array_equal(inlier, ~planted) and ref["status"] == S.OK and np.array_equal(ref["match_inlier"], ~planted)
    assert abs(meas[6] * D[11, 6] - 1.0) <= 1e-3
    assert out["status"] != 0 and out_ref["status"] != 0
    assert d <= 10.0 * d_ref and d < d0
    assert not d6 <= 10.0 * d_ref
    assert out["edge_weight"][-1] > 0.5
