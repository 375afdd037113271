"""GPU: ba_fundamental (Hartley normalisation, seven-point RANSAC and refinement on the device) against the numpy yardstick of
tests/fundamental_reference.py.

Tolerances, on the pixel F at unit Frobenius norm with the sign taken out (F_distance).  The solver alone and its coherence with
the reference: 100 x the reference's own worst error against the true F on the same samples + 1e-12 (two fp64 routes to one null
space and one cubic differ by conditioning, not by algorithm).  After the local optimisation: 10 x d_ref + 1e-12 of the yardstick
(the refinement of step 4 from the truth on the true inliers), d_ref the numpy reference's own distance to it.  Under a shift
of the images: 100 x the reference's own discrepancy under the same shift + 1e-12.  The measured figures are in DESIGN.md 4u."""
import ctypes as C
import itertools

import numpy as np
import pytest

from bundle_adjustment_amd.hip_backend import FUNDAMENTAL_STATUS
from tests import fundamental_reference as FR
from tests import homography_reference as HG
from tests import relpose_reference as RP

pytestmark = pytest.mark.gpu

ST = FUNDAMENTAL_STATUS
OUTS = ("F", "status", "n_inliers", "rms_px", "best_hyp", "match_inlier", "epipole1", "epipole2")      # the order of the C arguments
COUNTS = FR.COUNTS


@pytest.fixture(scope="module")
def solver():
    import __graft_entry__ as g
    g.build()
    from bundle_adjustment_amd import hip_backend
    with hip_backend.Solver(0) as s:
        yield s


def _offsets(counts):
    return np.r_[0, np.cumsum(counts)].astype(np.int64)


def _void_row(r, i, status):
    return (r["status"][i] == ST[status] and not r["F"][i].any() and r["n_inliers"][i] == 0 and np.isnan(r["rms_px"][i]) and r["best_hyp"][i] == -1
            and not r["epipole1"][i].any() and not r["epipole2"][i].any())


def _signed_unit(F):
    return abs(np.linalg.norm(F) - 1.0) <= 1e-15 and F.ravel()[np.argmax(np.abs(F))] > 0.0


# ---------------------------------------------------------------------------------------------------- the solver alone
@pytest.fixture(scope="module")
def minimal(solver):
    """8 pairs of 12 exact matches in one call, 16 seeds, n_hyp = 1, lo_rounds = 0, min_inliers = 8; per (seed, pair) the
    reference's solution on the sample its generator drew (None: void)."""
    scenes = FR.exact_scenes()
    p1, p2 = np.concatenate([s[0] for s in scenes]), np.concatenate([s[1] for s in scenes])
    runs = [solver.fundamental(p1, p2, _offsets([12] * 8), n_hyp=1, lo_rounds=0, seed=seed, min_inliers=8) for seed in range(16)]
    refs = {}
    for seed in range(16):
        for p, s in enumerate(scenes):
            ref = FR.fundamental(s[0], s[1], pair=p, n_hyp=1, lo_rounds=0, seed=seed, min_inliers=8)
            refs[seed, p] = ref["F"] if ref["best_hyp"] == 0 else None
    worst_ref = max(FR.F_distance(Fr, scenes[p][2]) for (_, p), Fr in refs.items() if Fr is not None)
    return scenes, runs, refs, worst_ref


def test_solver_alone_finds_the_true_F(minimal):
    scenes, runs, refs, worst_ref = minimal
    bound = 100.0 * worst_ref + 1e-12
    worst, void = 0.0, 0
    for seed, r in enumerate(runs):
        for p, s in enumerate(scenes):
            assert r["best_hyp"][p] == (-1 if refs[seed, p] is None else 0), (seed, p)
            if refs[seed, p] is None:
                void += 1
                assert _void_row(r, p, "degenerate") and not r["match_inlier"][12 * p:12 * p + 12].any()
                continue
            assert r["status"][p] == ST["ok"] and r["n_inliers"][p] == 12
            worst = max(worst, FR.F_distance(r["F"][p], s[2]))
    print(f"worst distance of the device's F to the true F {worst:.2e}; the numpy reference's worst on the same samples {worst_ref:.2e}; "
          f"bound {bound:.2e}; {void} void of 128")
    assert worst <= bound
    assert void <= 2


def test_generator_and_solver_are_coherent_with_the_reference(minimal):
    scenes, runs, refs, worst_ref = minimal
    bound = 100.0 * worst_ref + 1e-12
    worst = 0.0
    for seed, r in enumerate(runs):
        for p in range(len(scenes)):
            if refs[seed, p] is not None:
                worst = max(worst, FR.F_distance(r["F"][p], refs[seed, p]))
    print(f"worst distance of the device's F to the reference's seven-point solution on the sample the reference's generator drew {worst:.2e}; "
          f"bound {bound:.2e}")
    assert worst <= bound


# ---------------------------------------------------------------------------------------------------- outliers
@pytest.mark.parametrize("share,n_hyp,seed", FR.OUTLIER_CASES)
def test_outcome_under_outliers(solver, share, n_hyp, seed):
    c = FR.outlier_case(share, n_hyp, seed)
    ref = c["ref"]
    r = solver.fundamental(c["p1"], c["p2"], n_hyp=n_hyp, seed=seed)
    F, e1, e2 = r["F"][0], r["epipole1"][0], r["epipole2"][0]
    d = FR.F_distance(F, c["yard"])
    bound = 10.0 * c["d_ref"] + 1e-12
    res = np.linalg.norm(F @ e1), np.linalg.norm(F.T @ e2)
    print(f"share={share} n_hyp={n_hyp}: status {r['status'][0]}, {r['n_inliers'][0]} inliers ({(~c['planted']).sum()} planted), rms {r['rms_px'][0]:.6f} px "
          f"(reference {ref['rms_px']:.6f}), best_hyp {r['best_hyp'][0]} (reference {ref['best_hyp']}); F to the yardstick {d:.2e}, d_ref {c['d_ref']:.2e}, "
          f"bound {bound:.2e}; |F e1| {res[0]:.1e}, |F^T e2| {res[1]:.1e}")
    assert r["status"][0] == ref["status"] == ST["ok"]
    assert np.array_equal(r["match_inlier"], ~c["planted"]) and r["n_inliers"][0] == (~c["planted"]).sum()
    assert d <= bound
    assert _signed_unit(F)
    assert abs(np.linalg.norm(e1) - 1.0) <= 1e-15 and abs(np.linalg.norm(e2) - 1.0) <= 1e-15 and max(res) <= 1e-12
    assert e1[np.argmax(np.abs(e1))] > 0.0 and e2[np.argmax(np.abs(e2))] > 0.0
    assert abs(r["rms_px"][0] - ref["rms_px"]) <= 1e-6
    assert r["best_hyp"][0] == ref["best_hyp"]


# ---------------------------------------------------------------------------------------------------- edges of the mappings
def _raw_call(solver, p1, p2, off, opts, want):
    """ba_fundamental with NULL for every output that `want` does not name -> the dict of the outputs asked for."""
    from bundle_adjustment_amd import hip_backend as hb
    P, n = off.size - 1, len(p1)
    bufs = dict(F=np.empty((P, 3, 3)), status=np.empty(P, dtype=np.uint8), n_inliers=np.empty(P, dtype=np.int32), rms_px=np.empty(P),
                best_hyp=np.empty(P, dtype=np.int32), match_inlier=np.zeros(n, dtype=np.uint8), epipole1=np.empty((P, 3)), epipole2=np.empty((P, 3)))
    ptr = dict(F=hb._DP, status=C.POINTER(C.c_uint8), n_inliers=hb._IP, rms_px=hb._DP, best_hyp=hb._IP, match_inlier=C.POINTER(C.c_uint8),
               epipole1=hb._DP, epipole2=hb._DP)
    args = [bufs[k].ctypes.data_as(ptr[k]) if k in want else None for k in OUTS]
    hb._check(solver._lib.ba_fundamental(solver._h, P, off.ctypes.data_as(C.POINTER(C.c_int64)), hb._dp(p1), hb._dp(p2), C.byref(opts), *args))
    return {k: bufs[k] for k in want}


@pytest.mark.parametrize("n_hyp", FR.EDGE_N_HYP)
def test_edges_of_the_mappings(solver, n_hyp):
    """Eleven pairs of one call, empty ones between; 85 and 86: candidate 3 h + slot crosses the 256-lane score block inside
    hypothesis 85.  A pair of 8 or 9 matches draws the same seven matches again in another order from n_hyp = 85 on (8 and 36
    distinct samples): the two lowest costs then tie to rounding, and the winner is asked to lie inside the reference's tie set
    (test_fundamental_host.py counts these and holds every other near-tie to one in ten)."""
    pairs, yard, d_ref, cost = FR.edge_pairs()
    p1, p2 = np.concatenate([p[0] for p in pairs]), np.concatenate([p[1] for p in pairs])
    off = _offsets(COUNTS)
    r = solver.fundamental(p1, p2, off, n_hyp=n_hyp, min_inliers=8)
    again = solver.fundamental(p1, p2, off, n_hyp=n_hyp, min_inliers=8)
    for k in OUTS:
        assert np.array_equal(r[k], again[k], equal_nan=True), k
    left_out = 0
    for i, n in enumerate(COUNTS):
        sl = slice(off[i], off[i + 1])
        assert r["n_inliers"][i] == r["match_inlier"][sl].sum()
        if n < 8:
            assert _void_row(r, i, "few_matches")
            continue
        d = FR.F_distance(r["F"][i], yard[i])
        ties = FR.tie_set(cost[i], n_hyp)
        print(f"n_hyp={n_hyp} n={n}: status {r['status'][i]}, {r['n_inliers'][i]} inliers, best_hyp {r['best_hyp'][i]} (reference {FR.winner(cost[i], n_hyp)}, "
              f"{len(ties)} within 1e-9), F to the yardstick {d:.2e} (d_ref {d_ref[i]:.2e})")
        assert r["status"][i] == ST["ok"] and r["n_inliers"][i] == n
        assert d <= 10.0 * d_ref[i] + 1e-12, (n, d, d_ref[i])
        assert _signed_unit(r["F"][i])
        if len(ties) == 1:
            assert r["best_hyp"][i] == FR.winner(cost[i], n_hyp), n
        else:
            assert r["best_hyp"][i] in ties, n
            left_out += not FR.same_sample(ties, i, n)
    assert 10 * left_out <= sum(n >= 8 for n in COUNTS)
    # a pair's row does not depend on the other pairs: the odd (then the even) pairs filled with other data, the rest as they were
    for keep in (0, 1):
        q1, q2 = p1.copy(), p2.copy()
        for i in range(len(COUNTS)):
            if i % 2 != keep:
                q1[off[i]:off[i + 1]], q2[off[i]:off[i + 1]] = p2[off[i]:off[i + 1]] + 5.0, p1[off[i]:off[i + 1]] - 3.0
        b = solver.fundamental(q1, q2, off, n_hyp=n_hyp, min_inliers=8)
        for i in range(keep, len(COUNTS), 2):
            for k in OUTS:
                sl = slice(off[i], off[i + 1]) if k == "match_inlier" else i
                assert np.array_equal(b[k][sl], r[k][sl], equal_nan=True), (i, k)
    # every combination of NULL outputs: what is asked for comes back bit-equal
    opts = solver.fundamental_options(n_hyp=n_hyp, min_inliers=8)
    for m in range(len(OUTS) + 1):
        for want in itertools.combinations(OUTS, m):
            got = _raw_call(solver, p1, p2, off, opts, want)
            for k in want:
                assert np.array_equal(got[k].astype(r[k].dtype), r[k], equal_nan=True), (want, k)


# ---------------------------------------------------------------------------------------------------- degenerate input
def test_degenerate_inputs(solver):
    r = solver.fundamental(*FR.line_case())       # every 7 x 9 system has rank at most 6
    assert _void_row(r, 0, "degenerate") and not r["match_inlier"].any()
    r = solver.fundamental(*FR.point_case())      # step 1: a zero mean distance in image 2
    assert _void_row(r, 0, "degenerate") and not r["match_inlier"].any()
    c = FR.outlier_case(0.3, 256)
    r = solver.fundamental(c["p1"][:7], c["p2"][:7])
    assert _void_row(r, 0, "few_matches")
    r = solver.fundamental(c["p1"], c["p2"], n_hyp=256, min_inliers=250)
    assert r["status"][0] == ST["few_inliers"] and r["n_inliers"][0] == (~c["planted"]).sum() and r["best_hyp"][0] >= 0 and r["F"][0].any()


# ---------------------------------------------------------------------------------------------------- conditioning
def test_a_shift_of_both_images_changes_nothing(solver):
    """The Hartley step doing its job: pixels of the order of 5e4 never meet a quantity of the order of 1."""
    c = FR.outlier_case(0.3, 256)
    sh = np.array([5e4, -3e4])
    T = np.array([[1.0, 0.0, sh[0]], [0.0, 1.0, sh[1]], [0.0, 0.0, 1.0]])
    ref = FR.fundamental(c["p1"] + sh, c["p2"] + sh, n_hyp=256)
    d_ref = FR.F_distance(T.T @ ref["F"] @ T, c["ref"]["F"])
    base = solver.fundamental(c["p1"], c["p2"], n_hyp=256)
    r = solver.fundamental(c["p1"] + sh, c["p2"] + sh, n_hyp=256)
    d = FR.F_distance(T.T @ r["F"][0] @ T, base["F"][0])
    bound = 100.0 * d_ref + 1e-12
    print(f"shift (5e4, -3e4) px: T^T F T to the unshifted call's F {d:.2e}; the reference's own discrepancy {d_ref:.2e}; bound {bound:.2e}")
    assert r["status"][0] == ST["ok"] and np.array_equal(r["match_inlier"], base["match_inlier"]) and np.array_equal(r["match_inlier"], ~c["planted"])
    assert d <= bound


# ---------------------------------------------------------------------------------------------------- refusals
def test_invalid_arguments_name_their_field(solver):
    from bundle_adjustment_amd import hip_backend as hb
    c = FR.outlier_case(0.3, 256)
    p1, p2, n = c["p1"], c["p2"], len(c["p1"])

    def refused(word, off=None, **opts):
        with pytest.raises(hb.BAHipError) as e:
            solver.fundamental(p1, p2, off, **opts)
        assert "ba_fundamental" in str(e.value) and word in str(e.value) and word.encode() in hb.load_library().ba_last_error(), (word, str(e.value))

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
    with pytest.raises(TypeError):
        solver.fundamental(p1, p2, max_px=3.0)
    r = solver.fundamental(np.zeros((0, 2)), np.zeros((0, 2)), np.zeros(1, dtype=np.int64))     # n_pairs = 0: a no-op
    assert r["F"].shape == (0, 3, 3) and r["epipole1"].shape == (0, 3) and r["match_inlier"].shape == (0,)
    o = solver.fundamental_options()
    assert (o.n_hyp, o.lo_rounds, o.seed, o.max_epi_px, o.refine_iters, o.min_inliers) == (1024, 2, 0, 3.0, 20, 16)
    r = solver.fundamental(p1, p2)                # a valid call afterwards still works, with the defaults
    assert r["status"][0] == ST["ok"] and np.array_equal(r["match_inlier"], ~c["planted"])


def test_leaves_a_resident_problem_alone(solver):
    from bundle_adjustment_amd.synthetic import make_problem
    c = FR.outlier_case(0.3, 256)
    solver.set_problem(make_problem(6, 200, 4, seed=3))
    cost0 = solver.residuals("huber", want_vector=False)[2]
    a = solver.fundamental(c["p1"], c["p2"], n_hyp=256)
    other = solver.fundamental(c["p1"], c["p2"], n_hyp=256, seed=1)
    assert other["best_hyp"][0] != a["best_hyp"][0] or not np.array_equal(other["F"], a["F"])
    assert np.array_equal(other["match_inlier"], a["match_inlier"])
    assert solver.residuals("huber", want_vector=False)[2] == cost0


# ---------------------------------------------------------------------------------------------------- the surface
class _Match:
    def __init__(self, q, t):
        self.queryIdx, self.trainIdx = q, t


class _KeyPoint:
    def __init__(self, pt):
        self.pt = (float(pt[0]), float(pt[1]))


def _as_matches(p1, p2):
    n = len(p1)
    return [_Match(i, n - 1 - i) for i in range(n)], [_KeyPoint(p) for p in p1], [_KeyPoint(p) for p in p2[::-1]]


def test_match_by_fundamental_equals_the_guided_call(solver):
    from bundle_adjustment_amd import match_by_fundamental
    rng = np.random.default_rng(4)
    n = 150
    c = FR.outlier_case(0.3, 256)
    F = solver.fundamental(c["p1"], c["p2"], n_hyp=256)["F"][0]
    keep = np.nonzero(~c["planted"])[0][:n]
    des1 = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    perm = rng.permutation(n)
    des2 = des1[perm].copy()
    des2[rng.random(des2.shape) < 0.02] ^= 0x10                    # a few flipped bits
    kp1, kp2 = c["p1"][keep], c["p2"][keep][perm].copy()           # des2[j] = des1[perm[j]]: keypoint j is the match of perm[j]
    kp2[::7] += 40.0                                               # every seventh off its epipolar line
    got = match_by_fundamental(des1, kp1, des2, kp2, F, solver=solver)
    out = solver.match_guided([des1, des2], [kp1, kp2], fundamental=F[None], max_epi_px=3.0)
    good = np.nonzero(out["good"])[0]
    assert np.array_equal(got[0], good) and np.array_equal(got[1], out["best"][good]) and np.array_equal(got[2], out["dist1"][good])
    # a query gets its own keypoint, unless that one was moved off the line: then the gate leaves it another candidate or none
    moved = np.zeros(n, dtype=bool)
    moved[::7] = True
    own = np.argsort(perm)                                         # own[i]: the train row of query i
    wrong = perm[got[1]] != got[0]
    assert len(got[0]) > n // 2 and moved[own[got[0][wrong]]].all() and (~wrong).sum() >= (~moved).sum() - 5
    wide = match_by_fundamental(des1, kp1, des2, kp2, F, max_epi_px=500.0, solver=solver)
    assert len(wide[0]) > len(got[0])


def test_estimate_uncalibrated_tells_a_box_from_a_plane(solver):
    from bundle_adjustment_amd import estimate_uncalibrated
    p1, p2, _, _ = RP.noisy_scene(300, seed=3)
    F, i1, i2, idx, info = estimate_uncalibrated(*_as_matches(p1, p2), solver=solver, quiet=True)
    f, h = info["fundamental"], info["homography"]
    print(f"box: model {info['model']}, {f['n_inliers']} fundamental inliers (rms {f['rms_px']:.3f} px), {h['n_inliers']} homography inliers")
    assert info["model"] == "fundamental" and info["unique"] and f["status"] == ST["ok"] and len(idx) == 300 and i1.dtype == np.float32
    assert np.array_equal(F, f["F"]) and h["n_inliers"] < 0.8 * f["n_inliers"]
    p1, p2 = HG.noisy_plane(0)[:2]
    F, i1, i2, idx, info = estimate_uncalibrated(*_as_matches(p1, p2), solver=solver, quiet=True)
    f, h = info["fundamental"], info["homography"]
    print(f"plane: model {info['model']}, {f['n_inliers']} fundamental inliers (rms {f['rms_px']:.3f} px), {h['n_inliers']} homography inliers")
    assert info["model"] == "planar" and not info["unique"] and h["n_inliers"] == 300
    assert F is not None and _signed_unit(F) and f["n_inliers"] > 0 and f["rms_px"] < 3.0 and len(idx) == f["n_inliers"]
