"""CPU: the numpy yardstick of ba_triangulate_tracks (tests/track_reference.py) on problems with a known answer, every
status on a hand-built track, the bookkeeping of triangulation.filter_tracks, and the new ABI symbols in the header."""
import os
import re

import numpy as np
import pytest

from bundle_adjustment_amd.bal import BALProblem
from bundle_adjustment_amd.problem import BAProblem
from bundle_adjustment_amd.rotations import rvecs_to_matrices
from bundle_adjustment_amd.synthetic import _project, bal_project, make_problem
from bundle_adjustment_amd.triangulation import filter_tracks
from tests import track_reference as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K4 = np.array([700.0, 700.0, 640.0, 360.0])


def test_reference_recovers_the_true_points_from_noiseless_pixels():
    prob, cams_true, pts_true = make_problem(12, 300, 4, return_truth=True)
    uv, z = _project(cams_true, pts_true, prob.cam_idx, prob.pt_idx, prob.K4)
    assert (z > 0).all()
    exact = BAProblem(cams_true, prob.pts, prob.cam_idx, prob.pt_idx, uv, prob.K4, 0)
    for iters in (0, 20):
        out = tr.triangulate_tracks(exact, refine_iters=iters)
        assert (out["status"] == tr.OK).all()
        rel = np.abs(out["xyz"] - pts_true).max(axis=1) / np.abs(pts_true).max(axis=1)
        # noiseless pixels: the error is round-off times the conditioning of the flattest track (parallax 3.5 degrees: ~1e3
        # in the depth; squared by A^T A for the linear solution)
        assert rel.max() < (1e-8 if iters == 0 else 1e-10), rel.max()
        assert out["max_px"].max() < 1e-6


@pytest.mark.parametrize("k1", [-0.04, -0.03, -0.02])
@pytest.mark.parametrize("k2", [-0.003, 0.003])
def test_bal_undistortion_round_trips_the_projection(k1, k2):
    rng = np.random.default_rng(5)
    cams = np.zeros((1, 9))
    cams[0, 6:] = (900.0, k1, k2)
    pts = np.concatenate([rng.uniform(-6.0, 6.0, (200, 2)), rng.uniform(-14.0, -8.0, (200, 1))], axis=1)   # the camera looks down -z
    pts[0, :2] = 0.0                                                                                          # the image centre itself
    uv = bal_project(cams, pts, np.zeros(200, dtype=int), np.arange(200))
    p_true = -pts[:, :2] / pts[:, 2:3]
    for i in range(200):
        p0, p1, ok = tr.bal_undistort(uv[i], 900.0, k1, k2)
        assert ok
        assert abs(p0 - p_true[i, 0]) <= 1e-14 and abs(p1 - p_true[i, 1]) <= 1e-14


def test_bal_undistortion_refuses_the_non_monotone_branch():
    # k1 = -0.5: r (1 - 0.5 r^2) has its maximum 0.544 at r = 0.816; r_d = 2 has no solution on the monotone branch
    assert not tr.bal_undistort(np.array([1800.0, 0.0]), 900.0, -0.5, 0.0)[2]


def _views(cams, X, cam_ids, K4=K4, uv=None):
    cams = np.asarray(cams, dtype=np.float64)
    ids = np.asarray(cam_ids, dtype=np.int64)
    R = rvecs_to_matrices(cams[:, :3])
    if uv is None:
        uv = _project(cams, X[None, :], ids, np.zeros(len(ids), dtype=int), K4)[0]
    return tr.Views(R[ids], cams[ids, 3:6], uv, ids, K4=K4)


def _rig(n=4):
    cams = np.zeros((n, 6))
    cams[:, 3] = -np.arange(n) * 0.5          # centres at x = 0, 0.5, 1.0, ...
    return cams


def test_every_status_on_a_hand_built_track():
    cams, X = _rig(), np.array([0.3, -0.2, 10.0])
    opts = dict(min_angle_deg=1.0, max_reproj_px=4.0)
    assert tr.track(_views(cams, X, [0, 1, 2, 3]), **opts)["status"] == tr.OK
    one = tr.track(_views(cams, X, [2]), **opts)
    assert one["status"] == tr.FEW_VIEWS and np.isnan(one["xyz"]).all() and np.isnan(one["angle_deg"])
    assert tr.track(_views(cams, X, [1, 1]), **opts)["status"] == tr.FEW_VIEWS
    assert tr.track(_views(cams, X, []), **opts)["status"] == tr.FEW_VIEWS
    # behind: the point sits 10 m behind every camera; its pixels are those of the line through the centre
    behind = tr.track(_views(cams, np.array([0.3, -0.2, -10.0]), [0, 1, 2, 3]), **opts)
    assert behind["status"] == tr.BEHIND and np.allclose(behind["xyz"], [0.3, -0.2, -10.0], atol=1e-8)
    far = tr.track(_views(cams, np.array([30.0, -20.0, 1e4]), [0, 1, 2, 3]), **opts)
    assert far["status"] == tr.LOW_ANGLE and far["angle_deg"] < 0.01 and np.isfinite(far["xyz"]).all()
    v = _views(cams, X, [0, 1, 2, 3])
    v.uv[2] += (40.0, 0.0)
    out = tr.track(v, **opts)
    assert out["status"] == tr.HIGH_ERROR and out["max_px"] > 20.0
    # parallel rays: two cameras of the same orientation see the same normalised pixel
    par = _views(cams, X, [0, 3], uv=np.array([[700.0, 400.0], [700.0, 400.0]]))
    assert tr.track(par, **opts)["status"] == tr.DEGENERATE
    # the first failing test in enum order: behind AND low angle AND high error -> BEHIND
    v = _views(cams, np.array([30.0, -20.0, -1e4]), [0, 1, 2, 3])
    assert tr.track(v, min_angle_deg=1.0, max_reproj_px=1e-12)["status"] == tr.BEHIND


def test_jacobi_matches_lapack():
    rng = np.random.default_rng(2)
    for _ in range(20):
        A = rng.normal(size=(9, 4)) * np.array([1.0, 1.0, 1.0, 30.0])
        M = A.T @ A
        lam, V = tr.jacobi_eig(M)
        ref = np.linalg.eigvalsh(M)
        assert np.allclose(np.sort(lam), ref, rtol=1e-12, atol=1e-12 * ref.max())
        assert np.allclose(V.T @ V, np.eye(4), atol=1e-14) and np.allclose(M @ V, V * lam, atol=1e-11 * ref.max())


def test_robust_refinement_lands_on_a_stationary_point_of_its_cost():
    cams, X = _rig(6), np.array([0.8, 0.1, 9.0])
    v = _views(cams, X, np.arange(6))
    v.uv += np.random.default_rng(4).normal(0.0, 0.5, v.uv.shape)
    v.uv[4] += (15.0, -9.0)
    for loss in ("linear", "huber", "soft_l1", "cauchy", "arctan"):
        out = tr.track(v, loss=loss, f_scale=1.0)
        s = tr.sums_at(v, out["xyz"], loss, 1.0, 0.0)
        assert np.abs(s["g"]).max() <= 1e-6 * np.sqrt(np.trace(s["H"]) * s["sse"]), loss
    lin, hub = tr.track(v, loss="linear")["xyz"], tr.track(v, loss="huber")["xyz"]
    assert np.abs(hub - X).max() < np.abs(lin - X).max()


@pytest.mark.parametrize("model", ["pinhole", "bal"])
def test_long_track_cases_tell_a_same_stage_angle_from_the_true_one(model):
    """The three tracks of tests/track_cases.py with a placed widest pair: an angle over the pairs of one stage only (the
    mutant of track_reference) is the true one when both cameras sit in stage 0, and is off by more than 1e-6 relative --
    the device tests assert 1e-9 -- when they sit in stages (0, 1) and (1, 2)."""
    from bundle_adjustment_amd.hip_backend import TRACK_STAGE
    from tests import track_cases as tc
    prob, truth, pairs = tc.long_track_problem(model)
    R = rvecs_to_matrices(prob.cams[:, :3])
    by_pt = tr.observations_by_point(prob)
    lengths = np.bincount(prob.pt_idx, minlength=prob.n_pts)
    assert tuple(lengths[list(tc.LONG_POINTS)]) == tc.BORDER_LENGTHS + (tc.N_WIDE,) * 3
    assert np.sort(lengths)[prob.n_pts // 2] == 4 and lengths[:tc.N_SHORT].max() <= 6      # the library's median: long_thr = 8
    for p, stages, positions in zip(tc.WIDE_POINTS, tc.WIDE_STAGES, tc.WIDE_POSITIONS):
        v = tr.views_of(prob, p, R, by_pt)
        assert len(set(v.cam.tolist())) == tc.N_WIDE                      # distinct cameras
        assert tuple(int(np.nonzero(v.cam == c)[0][0]) for c in pairs[p]) == positions
        assert tuple(q // TRACK_STAGE for q in positions) == stages
        stage = np.arange(tc.N_WIDE) // TRACK_STAGE
        true, mutant = tr.max_angle_deg(v.centres, truth[p]), tr.max_angle_deg_same_stage(v.centres, truth[p], stage)
        rel = abs(true - mutant) / true
        print(f"{model} point {p}, widest pair in stages {stages}: true angle {true:.6f} deg, same-stage pairs only {mutant:.6f} ({rel:.2e})")
        assert mutant <= true
        if stages[0] == stages[1]:
            assert rel <= 1e-12
        else:
            assert rel > 1e-6
    # one stage for every view: the mutant is the yardstick
    v = tr.views_of(prob, tc.WIDE_POINTS[1], R, by_pt)
    assert tr.max_angle_deg_same_stage(v.centres, truth[tc.WIDE_POINTS[1]], np.zeros(tc.N_WIDE, int)) == \
        pytest.approx(tr.max_angle_deg(v.centres, truth[tc.WIDE_POINTS[1]]), rel=1e-14)


def test_filter_tracks_bookkeeping():
    prob = make_problem(5, 40, 3, seed=3)
    rng = np.random.default_rng(0)
    perm = rng.permutation(prob.n_obs)
    prob = BAProblem(prob.cams, prob.pts, prob.cam_idx[perm], prob.pt_idx[perm], prob.uv[perm], prob.K4, 0,
                     pt_held=np.arange(40) % 7 == 0)
    keep = rng.random(40) < 0.6
    new, old = filter_tracks(prob, keep)
    assert (old == np.nonzero(keep)[0]).all() and new.n_pts == int(keep.sum())
    assert (new.pts == prob.pts[old]).all() and (new.pt_held == prob.pt_held[old]).all()
    sel = keep[prob.pt_idx]
    assert new.n_obs == int(sel.sum())
    assert (old[new.pt_idx] == prob.pt_idx[sel]).all()                    # same points, observation order preserved
    assert (new.cam_idx == prob.cam_idx[sel]).all() and (new.uv == prob.uv[sel]).all()
    assert new.pt_idx.dtype == np.int32 and new.cams is prob.cams
    new.validate()
    empty, old0 = filter_tracks(prob, np.zeros(40, dtype=bool))
    assert empty.n_pts == 0 and empty.n_obs == 0 and old0.size == 0 and empty.pts.shape == (0, 3)
    everything, old1 = filter_tracks(prob, np.ones(40, dtype=bool))
    assert (everything.pt_idx == prob.pt_idx).all() and (old1 == np.arange(40)).all()
    for bad in (np.ones(39, dtype=bool), np.ones(40, dtype=np.int32), np.ones((40, 1), dtype=bool)):
        with pytest.raises(ValueError):
            filter_tracks(prob, bad)
    bal = BALProblem(np.zeros((5, 9)), prob.pts, prob.cam_idx, prob.pt_idx, prob.uv)
    nb, ob = filter_tracks(bal, keep)
    assert isinstance(nb, BALProblem) and (ob == old).all() and (nb.pt_idx == new.pt_idx).all()


def test_header_declares_both_symbols_and_the_structs_match():
    import ctypes as C
    from bundle_adjustment_amd import hip_backend as hb
    hdr = open(os.path.join(ROOT, "include", "ba_hip.h")).read()
    assert re.search(r"^int ba_default_track_options\(ba_track_options\*", hdr, flags=re.M)
    assert re.search(r"^int ba_triangulate_tracks\(ba_handle\*", hdr, flags=re.M)
    assert {"ba_default_track_options", "ba_triangulate_tracks"} <= set(hb.SYMBOLS)
    body = re.search(r"typedef struct ba_track_options \{(.*?)\} ba_track_options;", hdr, flags=re.S).group(1)
    names = re.findall(r"(?:int32_t|double)\s+([a-z_0-9]+)\s*;", body)
    assert names == [n for n, _ in hb.BATrackOptions._fields_]
    assert C.sizeof(hb.BATrackOptions) == 2 * 4 + 4 * 8 + 2 * 4
    enum = dict(re.findall(r"BA_TRACK_(\w+) = (\d)", hdr))
    assert {k.lower(): int(v) for k, v in enum.items()} == hb.TRACK_STATUS
    assert (tr.OK, tr.FEW_VIEWS, tr.DEGENERATE, tr.BEHIND, tr.LOW_ANGLE, tr.HIGH_ERROR) == tuple(range(6))
    doc = " ".join(re.search(r"/\* N-view triangulation and filtering of whole tracks.*?\*/", hdr, flags=re.S).group(0).replace("\n *", " ").split())
    assert "no collective" in doc and "write_points = 1 is a rank-local write" in doc and "Pinned on two ranks" in doc


def test_default_track_options_need_no_gpu():
    import __graft_entry__ as g
    g.build()
    from bundle_adjustment_amd import hip_backend as hb
    o = hb.BATrackOptions()
    assert hb.load_library().ba_default_track_options(o) == 0
    assert (o.loss, o.refine_iters, o.f_scale, o.min_angle_deg, o.max_reproj_px, o.min_depth, o.write_points, o.reserved0) == \
        (0, 20, 1.0, 0.0, 0.0, 0.0, 0, 0)
