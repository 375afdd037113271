"""GPU: ba_triangulate_tracks -- N-view triangulation, refinement, measures and status of whole tracks -- against the numpy
yardstick of tests/track_reference.py: parity for both camera models and both launch forms, the measured tolerance on
the points, a stationarity certificate that does not trust the yardstick's optimiser, what the call leaves on the handle,
both layout builds, the refusals, and the loop solve -> triangulate -> filter -> solve."""
import ctypes as C
import functools

import numpy as np
import pytest

from bundle_adjustment_amd import bal, hip_backend
from bundle_adjustment_amd.bal import BALProblem
from bundle_adjustment_amd.problem import BAProblem
from bundle_adjustment_amd.rotations import rvecs_to_matrices
from bundle_adjustment_amd.synthetic import _project, bal_project, make_problem, make_shared_bal_problem
from bundle_adjustment_amd.triangulation import filter_tracks, triangulate_tracks
from bundle_adjustment_amd.hip_backend import TRACK_STAGE
from tests import track_cases as tc
from tests import track_reference as tr

pytestmark = pytest.mark.gpu
K4 = np.array([900.0, 900.0, 640.0, 360.0])
NP = 257
OPTS = dict(min_angle_deg=0.3, max_reproj_px=8.0)
FIELDS = ("angle_deg", "rms_px", "max_px")


# ------------------------------------------------------------------------------------------------ the parity problem
@functools.lru_cache(maxsize=None)
def parity_problem(model):
    """257 points, 70 cameras.  Points 0-239 and 252-256: ordinary tracks of 2-6 views among 12 of the cameras (median 4:
    with 2 lanes per point the library's long-track threshold is 8).  240-244: tracks of 8 (= the threshold), 9, 65, 70
    views among all 70 cameras and one of 130 views (every camera, 60 of them twice).  245 one view, 246 two views by one
    camera, 247 no view, 248 behind the cameras, 249 1e4 m away, 250 with a 40-px outlier, 251 two parallel rays.
    Cameras are the true ones; pixels carry N(0, 0.5) noise -- N(0, 0.01) for 249, whose parallax is 0.013 degrees, none for 251
    (a track without noise has residuals of round-off size, which no relative tolerance describes).  -> (problem, true points)."""
    rng = np.random.default_rng(11)
    _, cams, pts = make_problem(70, NP, 4, seed=7, K4=K4, return_truth=True)
    pts = pts.copy()
    short_cams = np.arange(0, 72, 6)[:12]
    ci, pi = [], []
    lengths = {p: 2 + p % 5 for p in list(range(240)) + list(range(252, NP))}
    for p, n in lengths.items():
        ci += list(rng.choice(short_cams, size=n, replace=False)); pi += [p] * n
    for p, n in ((240, 8), (241, 9), (242, 65), (243, 70)):
        ci += list(rng.choice(70, size=n, replace=False)); pi += [p] * n
    ci += list(range(70)) + list(rng.choice(70, size=60, replace=False)); pi += [244] * 130
    ci += [5]; pi += [245]
    ci += [9, 9]; pi += [246, 246]
    pts[248] = (1.0, 0.3, -12.0)
    pts[249] = (40.0, -25.0, 1e4)
    for p in (248, 249, 250):
        ci += [0, 18, 36, 54]; pi += [p] * 4
    pts[251] = 1e25 * np.array([0.05, -0.02, 1.0])          # a direction: the two rays are parallel
    ci += [6, 60]; pi += [251, 251]
    ci, pi = np.array(ci, dtype=np.int32), np.array(pi, dtype=np.int32)
    if model == "bal":
        from bundle_adjustment_amd.bal import from_pinhole
        b = from_pinhole(BAProblem(cams, pts, ci, pi, np.zeros((len(ci), 2)), K4, 0))
        cams = b.cams.copy()
        cams[:, 6] = 900.0 * (1.0 + 0.02 * rng.normal(size=70))
        cams[:, 7] = -0.03 + 0.01 * rng.normal(size=70)
        cams[:, 8] = 0.003 * rng.choice([-1.0, 1.0], size=70)
        uv = bal_project(cams, pts, ci, pi)
    else:
        uv = _project(cams, pts, ci, pi, K4)[0]
    noisy = ~np.isin(pi, (249, 251))
    uv[noisy] += rng.normal(0.0, 0.5, size=(int(noisy.sum()), 2))
    uv[pi == 249] += rng.normal(0.0, 0.01, size=(4, 2))
    uv[np.nonzero(pi == 250)[0][2]] += (40.0, 0.0)
    order = rng.permutation(len(ci))
    ci, pi, uv = ci[order], pi[order], uv[order]
    start = pts + rng.normal(0.0, 0.05, size=pts.shape)
    if model == "bal":
        return BALProblem(cams, start, ci, pi, uv).validate(), pts
    return BAProblem(cams, start, ci, pi, uv, K4.copy(), 0).validate(), pts


@functools.lru_cache(maxsize=None)
def parity_reference(model, loss, iters):
    prob, _ = parity_problem(model)
    return tr.triangulate_tracks(prob, loss=loss, refine_iters=iters, **OPTS)


def run_device(prob, lanes2=False, monkeypatch=None, **opts):
    """-> (outputs, layout scalars) of ba_triangulate_tracks on prob (either model)."""
    if lanes2:
        monkeypatch.setenv("BA_PT_LANES", "2")        # 2 lanes per point: the library then splits off the long tracks
    with hip_backend.Solver(0) as s:
        intr = s._set_bal(prob) if isinstance(prob, BALProblem) else s.set_problem(prob)
        out = s.triangulate_tracks(intr=intr, **opts)
        return out, s.debug_layout("scalars")


def decided_far_from_threshold(ref, opts):
    """Points whose deciding quantity is not within 1e-6 relative of its threshold (on the yardstick's numbers)."""
    far = np.ones(len(ref["status"]), dtype=bool)
    for key, thr in (("angle_deg", opts.get("min_angle_deg", 0.0)), ("max_px", opts.get("max_reproj_px", 0.0))):
        if thr > 0.0:
            far &= ~(np.abs(ref[key] - thr) <= 1e-6 * thr)
    return far


def measures_at_device_points(prob, out, points):
    """The yardstick's angle / rms / max evaluated at the device's own xyz."""
    R = rvecs_to_matrices(prob.cams[:, :3])
    by_pt = tr.observations_by_point(prob)
    return {p: tr.measures_at(tr.views_of(prob, p, R, by_pt), out["xyz"][p])[:3] for p in points}


def check_measures(prob, out, points):
    worst = (0.0, None, None)
    for p, m in measures_at_device_points(prob, out, points).items():
        for key, want in zip(FIELDS, m):
            worst = max(worst, (abs(out[key][p] - want) / max(abs(want), 1e-300), key, int(p)), key=lambda t: t[0])
    print(f"measures at the device's xyz: largest relative difference {worst[0]:.3e} ({worst[1]} of point {worst[2]}) over {len(points)} points")
    assert worst[0] <= 1e-9, worst


# ------------------------------------------------------------------------------------------------ 1 parity
@pytest.mark.parametrize("lanes2", [True, False], ids=["long-tracks-split-off", "one-launch-form"])
@pytest.mark.parametrize("model", ["pinhole", "bal"])
def test_status_and_measures_match_the_reference(model, lanes2, monkeypatch):
    prob, _ = parity_problem(model)
    ref = parity_reference(model, "linear", 20)
    out, lay = run_device(prob, lanes2, monkeypatch, **OPTS)
    if lanes2:
        assert lay["lanes"] == 2 and lay["long_thr"] == 8 and lay["n_long"] == 4     # tracks of 9, 65, 70 and 130 views
    else:
        assert lay["n_long"] == 0
    assert set(ref["status"]) == set(range(6)), np.bincount(ref["status"])
    want = {245: tr.FEW_VIEWS, 246: tr.FEW_VIEWS, 247: tr.FEW_VIEWS, 248: tr.BEHIND, 249: tr.LOW_ANGLE, 250: tr.HIGH_ERROR,
            251: tr.DEGENERATE}
    for p, st in want.items():
        assert ref["status"][p] == st, (p, ref["status"][p])
    assert (np.delete(ref["status"], list(want)) == tr.OK).all()
    far = decided_far_from_threshold(ref, OPTS)
    assert far.all()                                   # wide margins by construction: the yardstick excludes nothing
    assert (~far).sum() <= 0.01 * NP
    assert np.array_equal(out["status"][far], ref["status"][far]), np.nonzero(out["status"] != ref["status"])[0]
    nanp = np.isin(ref["status"], (tr.FEW_VIEWS,)) | (np.arange(NP) == 251)
    assert np.isnan(out["xyz"][nanp]).all() and np.isnan(out["angle_deg"][nanp]).all() and np.isnan(out["max_px"][nanp]).all()
    assert np.isfinite(out["xyz"][~nanp]).all()
    check_measures(prob, out, np.nonzero(~nanp)[0])


@functools.lru_cache(maxsize=None)
def long_reference(model):
    return tr.triangulate_tracks(tc.long_track_problem(model)[0], **OPTS)


@pytest.mark.parametrize("lanes2", [True, False], ids=["long-tracks-split-off", "one-launch-form"])
@pytest.mark.parametrize("model", ["pinhole", "bal"])
def test_tracks_longer_than_a_stage(model, lanes2, monkeypatch):
    """Tracks of TRACK_STAGE - 1, TRACK_STAGE, TRACK_STAGE + 1, 2 TRACK_STAGE, 2 TRACK_STAGE + 1 views and three of
    2 TRACK_STAGE + 76 whose widest pair of cameras sits in stages (0, 0), (0, 1) -- last position of stage 0, first of stage 1
    -- and (1, 2) of the track's list as the device holds it (tests/track_cases.py): the second and third trip of the long-track
    kernel's staging loop, its `j <= c0` skip and its shortened last stage.  test_tracks_host.py shows that an angle over
    same-stage pairs alone is off by 2e-3 on the last two, against the 1e-9 asserted here.  The same tracks under the
    default lane count go through the 8-lane form, which stages nothing."""
    prob, _, pairs = tc.long_track_problem(model)
    ref = long_reference(model)
    if lanes2:
        monkeypatch.setenv("BA_PT_LANES", "2")
    with hip_backend.Solver(0) as s:
        intr = s._set_bal(prob) if isinstance(prob, BALProblem) else s.set_problem(prob)
        out = s.triangulate_tracks(intr=intr, **OPTS)
        lay = s.debug_layout("scalars")
        pt_off, p_cam, slot = s.debug_layout("pt_off"), s.debug_layout("p_cam"), s.debug_layout("slot")
    lengths = np.bincount(prob.pt_idx, minlength=prob.n_pts)
    if lanes2:
        assert lay["lanes"] == 2 and lay["long_thr"] == 8
        assert lay["n_long"] == int((lengths > lay["long_thr"]).sum()) == len(tc.LONG_POINTS)
    else:
        assert lay["n_long"] == 0
    # the borders, from the layout the kernel reads: the lengths of the tracks, and the stages the widest pairs fall in
    seg = {p: p_cam[pt_off[slot[p]]:pt_off[slot[p] + 1]] for p in tc.LONG_POINTS}
    assert tuple(len(seg[p]) for p in tc.LONG_POINTS) == tc.BORDER_LENGTHS + (tc.N_WIDE,) * 3
    for p, stages, positions in zip(tc.WIDE_POINTS, tc.WIDE_STAGES, tc.WIDE_POSITIONS):
        at = tuple(int(np.nonzero(seg[p] == c)[0][0]) for c in pairs[p])
        assert tuple(q // TRACK_STAGE for q in at) == stages, (p, at)
        if stages == (0, 1):
            assert at == (TRACK_STAGE - 1, TRACK_STAGE)
    far = decided_far_from_threshold(ref, OPTS)
    assert far.all()                                   # the yardstick excludes nothing
    assert (ref["status"] == tr.OK).all()
    assert np.array_equal(out["status"], ref["status"]), np.nonzero(out["status"] != ref["status"])[0]
    assert np.isfinite(out["xyz"]).all()
    check_measures(prob, out, np.arange(prob.n_pts))


def test_both_sides_of_the_angle_test_on_the_stock_generator():
    prob = make_problem(12, 300, 4)
    ref = tr.triangulate_tracks(prob, min_angle_deg=6.0)
    out, _ = run_device(prob, min_angle_deg=6.0)
    assert 5 <= (ref["status"] == tr.LOW_ANGLE).sum() <= 100 and (ref["status"] == tr.OK).sum() >= 200
    assert decided_far_from_threshold(ref, dict(min_angle_deg=6.0)).all()
    assert np.array_equal(out["status"], ref["status"])


# ------------------------------------------------------------------------------------------------ 2 tolerance on xyz
def _rel(a, b):
    return np.abs(a - b).max(axis=1) / np.abs(b).max(axis=1)


@functools.lru_cache(maxsize=None)
def stock(model):
    prob, cams_true, pts_true = make_problem(12, 300, 4, K4=K4, return_truth=True)
    if model == "bal":
        b = bal.from_pinhole(prob)
        rng = np.random.default_rng(3)
        b.cams[:, 7] = -0.03 + 0.01 * rng.normal(size=12)
        b.cams[:, 8] = 0.003 * rng.choice([-1.0, 1.0], size=12)
        t = bal.from_pinhole(BAProblem(cams_true, pts_true, prob.cam_idx, prob.pt_idx, prob.uv, K4, 0))
        t.cams[:, 6:] = b.cams[:, 6:]
        uv = bal_project(t.cams, pts_true, prob.cam_idx, prob.pt_idx) + np.random.default_rng(4).normal(0.0, 0.5, prob.uv.shape)
        return BALProblem(b.cams, b.pts, b.cam_idx, b.pt_idx, uv), pts_true
    return prob, pts_true


@functools.lru_cache(maxsize=None)
def spread(case, iters):
    """-> (problem, options, reference, rows with a finite reference point, d_ref) of one input: d_ref is the reference
    refined from its own DLT against the reference refined from the true point (refine_iters = 20), or the reference through
    the A^T A eigenvector against the reference through LAPACK's SVD of A (refine_iters = 0)."""
    kind, model = case.split("-")
    prob, truth = stock(model) if kind == "stock" else parity_problem(model)
    opts = dict(OPTS) if kind == "parity" else {}
    ref = parity_reference(model, "linear", iters) if kind == "parity" else tr.triangulate_tracks(prob, refine_iters=iters)
    ok = np.isfinite(ref["xyz"]).all(axis=1)
    if iters:
        other = tr.triangulate_tracks(prob, points=np.nonzero(ok)[0], refine_iters=iters, x0=truth, **opts)
    else:
        other = tr.triangulate_tracks(prob, points=np.nonzero(ok)[0], refine_iters=0, dlt_method="svd", **opts)
    return prob, opts, ref, ok, float(_rel(other["xyz"], ref["xyz"][ok]).max())


# (every track of the stock problem has 4 views: one launch form)
@pytest.mark.parametrize("case,lanes2", [("stock-pinhole", False), ("stock-bal", False), ("parity-pinhole", False),
                                         ("parity-pinhole", True), ("parity-bal", False), ("parity-bal", True)])
def test_points_within_the_measured_spread_of_the_reference(case, lanes2, monkeypatch):
    """The device may differ from the reference by 10 d_ref + 1e-12, relative, per input (d_ref: see spread)."""
    for iters in (20, 0):
        prob, opts, ref, ok, d_ref = spread(case, iters)
        out, _ = run_device(prob, lanes2, monkeypatch, refine_iters=iters, **opts)
        dev = float(_rel(out["xyz"][ok], ref["xyz"][ok]).max())
        print(f"{case} refine_iters {iters}: d_ref {d_ref:.3e}, device against the reference {dev:.3e}")
        assert dev <= 10.0 * d_ref + 1e-12
        assert np.array_equal(np.isfinite(out["xyz"]).all(axis=1), ok)


# ------------------------------------------------------------------------------------------------ 3 certificate
@pytest.mark.parametrize("loss,outliers", [("linear", 0.0), ("huber", 0.05)])
def test_gradient_certificate_at_the_device_points(loss, outliers):
    """|Jp^T w r| per point from ba_linearize's bp after write_points = 1: at most ten times the yardstick's own gradient at
    the yardstick's point plus 1e-9 |Jp| |r|."""
    prob = make_problem(12, 300, 4, seed=2, outlier_frac=outliers)
    ref = tr.triangulate_tracks(prob, loss=loss)
    R = rvecs_to_matrices(prob.cams[:, :3])
    by_pt = tr.observations_by_point(prob)
    with hip_backend.Solver(0) as s:
        s.set_problem(prob)
        out = s.triangulate_tracks(loss=loss, write_points=1)
        bp = s.linearize(loss)[3]
    okp = np.nonzero(out["status"] == tr.OK)[0]
    assert okp.size >= 250
    worst = 0.0
    for p in okp:
        v = tr.views_of(prob, p, R, by_pt)
        at_ref = tr.sums_at(v, ref["xyz"][p], loss, 1.0, 0.0)
        lin = tr.sums_at(v, ref["xyz"][p], "linear", 1.0, 0.0)
        bound = 10.0 * np.sqrt((at_ref["g"] ** 2).sum()) + 1e-9 * np.sqrt(np.trace(lin["H"]) * lin["sse"])
        worst = max(worst, np.sqrt((bp[p] ** 2).sum()) / bound)
    print(f"{loss}: largest |bp| / bound over {okp.size} points {worst:.3e}")
    assert worst <= 1.0


# ------------------------------------------------------------------------------------------------ 4 handle hygiene
SOLVE = dict(loss="huber", max_iters=6, small_solver=1)


def test_write_points_0_leaves_the_handle_as_found():
    prob = make_problem(12, 300, 4, seed=5)
    with hip_backend.Solver(0) as s:
        s.set_problem(prob)
        a = s.solve(**SOLVE)
        pa = s.get_params()
    with hip_backend.Solver(0) as s:
        s.set_problem(prob)
        before = s.get_params()
        s.triangulate_tracks(loss="huber", min_angle_deg=2.0)
        after = s.get_params()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        b = s.solve(**SOLVE)
        pb = s.get_params()
    assert np.array_equal(pa[0], pb[0]) and np.array_equal(pa[1], pb[1])
    assert all(a[k] == b[k] for k in ("final_cost", "final_sse", "iterations", "pcg_iterations", "final_lambda"))


def test_write_points_1_is_set_params_with_the_merged_points():
    prob = make_problem(12, 300, 4, seed=5)
    held = np.arange(300) % 9 == 0
    with hip_backend.Solver(0) as s:
        s.set_problem(prob)
        s.set_held(points=held)
        s.solve(**SOLVE)                                   # (the current parameter set is then whichever the solve ended on)
        cams, old = s.get_params()
        out = s.triangulate_tracks(min_angle_deg=6.0, write_points=1)
        c1, p1 = s.get_params()
        take = (out["status"] == tr.OK) & ~held
        assert take.sum() > 100 and (~take).sum() > held.sum() and ((out["status"] == tr.OK) & held).sum() > 10
        assert np.array_equal(c1, cams)
        assert np.array_equal(p1[take], out["xyz"][take]) and np.array_equal(p1[~take], old[~take])
        a = s.solve(**SOLVE)
        pa = s.get_params()
    with hip_backend.Solver(0) as s:
        s.set_problem(prob)
        s.set_held(points=held)
        s.solve(**SOLVE)
        s.set_params(cams, p1)
        b = s.solve(**SOLVE)
        pb = s.get_params()
    assert np.array_equal(pa[0], pb[0]) and np.array_equal(pa[1], pb[1])
    assert all(a[k] == b[k] for k in ("final_cost", "final_sse", "iterations", "pcg_iterations", "final_lambda"))


# ------------------------------------------------------------------------------------------------ 5 layout paths
def _shuffled(prob, seed):
    """The same problem with the points renumbered at random and the observations in random order: -> (problem, new_of_old)."""
    rng = np.random.default_rng(seed)
    new_of_old = rng.permutation(prob.n_pts).astype(np.int32)
    order = rng.permutation(prob.n_obs)
    pts = np.empty_like(prob.pts)
    pts[new_of_old] = prob.pts
    return BAProblem(prob.cams, pts, prob.cam_idx[order], new_of_old[prob.pt_idx[order]], prob.uv[order], prob.K4, 0), new_of_old


def _rms_at(prob, xyz):
    uv = _project(prob.cams, xyz, prob.cam_idx, prob.pt_idx, prob.K4)[0]
    e2 = ((prob.uv - uv) ** 2).sum(axis=1)
    return np.sqrt(np.bincount(prob.pt_idx, weights=e2, minlength=prob.n_pts) / np.bincount(prob.pt_idx, minlength=prob.n_pts))


@pytest.mark.parametrize("size,path", [((40, 6000, 10), 1), ((5, 200, 4), 0)], ids=["device-built", "packed-upload"])
def test_caller_point_order_on_both_layout_builds(size, path):
    prob, new_of_old = _shuffled(make_problem(*size, seed=1), 8)
    assert prob.n_obs >= 50000 or path == 0
    out, lay = run_device(prob, max_reproj_px=50.0)
    assert lay["build_path"] == path
    assert (out["status"] == tr.OK).all()
    # every point: the rms of the device's xyz under the CALLER's numbering is the rms the device reports
    assert np.allclose(_rms_at(prob, out["xyz"]), out["rms_px"], rtol=1e-9, atol=0.0)
    sample = np.random.default_rng(0).choice(prob.n_pts, size=150, replace=False)
    ref = tr.triangulate_tracks(prob, points=sample, max_reproj_px=50.0)
    unshuffled = tr.triangulate_tracks(make_problem(*size, seed=1), points=np.argsort(new_of_old)[sample][:20], max_reproj_px=50.0)
    assert float(_rel(unshuffled["xyz"], ref["xyz"][:20]).max()) <= 1e-7          # (the yardstick itself does not care)
    dev = float(_rel(out["xyz"][sample], ref["xyz"]).max())
    print(f"{size}: device against the reference on 150 points {dev:.3e}")
    assert dev <= 1e-10                                  # order check; the tolerance proper is test 2's
    check_measures(prob, out, sample[:40])


# ------------------------------------------------------------------------------------------------ 6 refusals
def _raw(s, o, intr=None):
    lib = hip_backend.load_library()
    rc = lib.ba_triangulate_tracks(s._h, intr, C.byref(o), None, None, None, None, None)
    return rc, lib.ba_last_error().decode()


def test_refusals():
    prob = make_problem(5, 50, 3)
    with hip_backend.Solver(0) as s:
        o = s.track_options()
        rc, msg = _raw(s, o)
        assert rc == -3 and msg                          # BA_ERR_STATE: no problem
        s.set_problem(prob, with_params=False)
        rc, msg = _raw(s, o)
        assert rc == -3 and msg                          # ... no parameters
        s.set_params(prob.cams, prob.pts)
        assert _raw(s, o)[0] == 0
        for field, value in (("loss", 5), ("loss", -1), ("f_scale", 0.0), ("f_scale", -1.0), ("refine_iters", -1), ("reserved0", 1)):
            o = s.track_options()
            setattr(o, field, value)
            rc, msg = _raw(s, o)
            assert rc == -1 and msg, field                # BA_ERR_INVALID
        lib = hip_backend.load_library()
        assert lib.ba_triangulate_tracks(s._h, None, None, None, None, None, None, None) == -1
        with pytest.raises(TypeError):
            s.triangulate_tracks(no_such_option=1)
        with pytest.raises(ValueError):
            s.triangulate_tracks(loss="nope")


# ------------------------------------------------------------------------------------------------ 7 end to end
def test_solve_triangulate_filter_solve_on_a_bal_problem():
    prob, _ = make_shared_bal_problem(None, 20, 2000, 9000, seed=3, outlier_frac=0.05)
    kw = dict(fixed_cam=0, loss="huber", max_iters=15)
    first, s1 = bal.solve(prob, **kw)
    out, merged = bal.triangulate(first, write=True, loss="huber", max_reproj_px=4.0, min_angle_deg=0.2)
    keep = out["status"] == tr.OK
    assert 0.3 * prob.n_pts < keep.sum() < prob.n_pts
    assert np.array_equal(merged.pts[keep], out["xyz"][keep]) and np.array_equal(merged.pts[~keep], first.pts[~keep])
    kept, old = filter_tracks(merged, keep)
    assert np.array_equal(old, np.nonzero(keep)[0]) and np.array_equal(kept.pts, merged.pts[old])
    second, s2 = bal.solve(kept, **kw)
    rmse1 = np.sqrt(s1["final_sse"] / first.n_obs)
    rmse2 = np.sqrt(s2["final_sse"] / kept.n_obs)
    print(f"rmse {rmse1:.4f} px on {first.n_pts} points -> {rmse2:.4f} px on {kept.n_pts} points")
    assert kept.n_pts < first.n_pts and rmse2 < rmse1
    back = first.pts.copy()
    back[old] = second.pts                                 # the adjusted points, back under their old numbers
    assert np.array_equal(back[~keep], first.pts[~keep]) and not np.array_equal(back[keep], first.pts[keep])


def test_pinhole_wrapper_returns_the_merged_problem():
    prob = make_problem(6, 120, 4, seed=9)
    out, merged = triangulate_tracks(prob, write=True, min_angle_deg=10.0)
    take = out["status"] == tr.OK
    assert take.any() and (~take).any()
    assert np.array_equal(merged.pts[take], out["xyz"][take]) and np.array_equal(merged.pts[~take], prob.pts[~take])
    assert merged.cams is prob.cams and np.array_equal(triangulate_tracks(prob, min_angle_deg=10.0)["status"], out["status"])
