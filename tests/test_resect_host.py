"""CPU: the numpy yardstick of ba_resect (tests/resect_reference.py) on problems with a known answer, the reduced 4 x 4 DLT
against the SVD of the full matrix, every status on a hand-built camera, and the new ABI symbols in the header and library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from bundle_adjustment_amd.bal import from_pinhole
from bundle_adjustment_amd.problem import BAProblem
from bundle_adjustment_amd.rotations import rvecs_to_matrices
from bundle_adjustment_amd.synthetic import _project, bal_project, make_problem
from tests import resect_reference as rr
from tests.resect_reference import pose_diff

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def exact_problem(bal=False):
    prob, cams_true, pts_true = make_problem(6, 60, 3, return_truth=True, K4=(700.0, 700.0, 640.0, 360.0))
    if bal:
        b = from_pinhole(BAProblem(cams_true, pts_true, prob.cam_idx, prob.pt_idx, prob.uv, prob.K4, 0))
        b.cams[:, 6:] = (900.0, -0.03, 0.002)
        b.uv = bal_project(b.cams, b.pts, b.cam_idx, b.pt_idx)
        return b, b.cams[:, :6].copy()
    uv, z = _project(cams_true, pts_true, prob.cam_idx, prob.pt_idx, prob.K4)
    assert (z > 0).all()
    return BAProblem(cams_true.copy(), pts_true, prob.cam_idx, prob.pt_idx, uv, prob.K4, 0), cams_true


@pytest.mark.parametrize("bal", [False, True])
def test_reference_recovers_noise_free_poses(bal):
    exact, cams_true = exact_problem(bal)
    exact.cams[:, :6] += 0.3                                  # the DLT start does not read the current pose
    for method in ("svd", "reduced"):
        for iters in (0, 20):
            out = rr.resect_cameras(exact, refine_iters=iters, dlt_method=method)
            assert (out["status"] == rr.OK).all()
            d = pose_diff(out["poses"], cams_true).max()
            # noise-free pixels: round-off times the conditioning of the DLT (squared by the normal matrix of the reduced form)
            assert d < (1e-8 if iters == 0 else 1e-11), (method, iters, d)
            assert out["max_px"].max() < 1e-5 and (out["n_inliers"] == np.bincount(exact.cam_idx, minlength=6)).all()


def test_reduced_form_agrees_with_the_svd_form():
    for seed, kw in ((0, {}), (1, dict(outlier_frac=0.05))):
        prob, cams_true, pts_true = make_problem(12, 300, 4, seed=seed, return_truth=True, **kw)
        prob = BAProblem(prob.cams, pts_true, prob.cam_idx, prob.pt_idx, prob.uv, prob.K4, 0)
        a = rr.resect_cameras(prob, refine_iters=0, dlt_method="svd")
        b = rr.resect_cameras(prob, refine_iters=0, dlt_method="reduced")
        assert (a["status"] == rr.OK).all() and (b["status"] == rr.OK).all()
        # both minimise the same algebraic error over |P| = 1 / |p3| = 1: the minimisers differ by the normalisation only,
        # i.e. by second order in the pixel noise (0.5 px / 700 px)
        assert pose_diff(a["poses"], b["poses"]).max() < 2e-2
        # and both are starts from which the refinement reaches the same pose
        ra = rr.resect_cameras(prob, loss="huber", dlt_method="svd")
        rb = rr.resect_cameras(prob, loss="huber", dlt_method="reduced")
        rt = rr.resect_cameras(prob, loss="huber", x0=cams_true)
        assert pose_diff(ra["poses"], rb["poses"]).max() < 1e-9 and pose_diff(ra["poses"], rt["poses"]).max() < 1e-9


@pytest.mark.parametrize("bal", [False, True])
def test_analytic_jacobian_against_finite_differences(bal):
    exact, _ = exact_problem(bal)
    o = rr.obs_of(exact, 3)
    pose = exact.cams[3, :6] + np.array([0.3, -0.2, 0.25, 0.05, -0.03, 0.04])
    _, J, _ = o.project(pose)
    for k in range(6):
        h = np.zeros(6)
        h[k] = 1e-6
        fd = (o.project(pose + h)[0] - o.project(pose - h)[0]) / 2e-6
        assert np.abs(fd - J[:, :, k]).max() <= 1e-6 * np.abs(J[:, :, k]).max()


def _camera(n=40, seed=3):
    rng = np.random.default_rng(seed)
    pose = np.array([0.05, -0.1, 0.02, 0.3, -0.2, 0.5])
    X = np.stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(8, 16, n)], axis=1)
    K4 = np.array([700.0, 700.0, 640.0, 360.0])
    uv = _project(pose[None], X, np.zeros(n, dtype=int), np.arange(n), K4)[0]
    return rr.Obs(X, uv, K4=K4), pose


def test_every_status_on_a_hand_built_camera():
    o, pose = _camera()
    off = pose + 0.01
    assert rr.resect(o, off)["status"] == rr.OK
    assert pose_diff(rr.resect(o, off)["pose"], pose).max() < 1e-11
    few = rr.resect(o.keep(np.arange(40) < 5), off)
    assert few["status"] == rr.FEW_POINTS and (few["pose"] == off).all() and np.isnan(few["rms_px"]) and few["n_inliers"] == 0
    assert rr.resect(o.keep(np.arange(40) < 5), off, init="current", min_inliers=3)["status"] == rr.OK
    assert rr.resect(o.keep(np.arange(40) < 5), off, init="current")["status"] == rr.FEW_INLIERS       # (the default asks for 6)
    assert rr.resect(o.keep(np.arange(40) < 2), off, init="current")["status"] == rr.FEW_POINTS
    flat = rr.Obs(o.X * np.array([1.0, 1.0, 0.0]) + np.array([0.0, 0.0, 10.0]), o.uv, K4=o.K4)
    deg = rr.resect(flat, off)
    assert deg["status"] == rr.DEGENERATE and (deg["pose"] == off).all() and np.isnan(deg["max_px"])
    assert rr.resect(flat, off, init="current", refine_iters=0)["status"] == rr.OK
    # mirrored behind the scene: the camera centre reflected through the points' plane, looking away
    mirrored = np.array([0.0, np.pi, 0.0, 0.0, 0.0, -24.0])
    assert rr.resect(o, mirrored, init="current", refine_iters=0)["status"] == rr.BEHIND
    noisy = rr.Obs(o.X, o.uv.copy(), K4=o.K4)
    noisy.uv[:36] += 40.0 * np.random.default_rng(0).normal(size=(36, 2))
    out = rr.resect(noisy, pose, init="current", refine_iters=0, max_reproj_px=2.0)
    assert out["status"] == rr.FEW_INLIERS and out["n_inliers"] == 4 and out["max_px"] < 1e-9
    out = rr.resect(noisy, pose, init="current", refine_iters=0, max_rms_px=5.0)
    assert out["status"] == rr.HIGH_ERROR and out["n_inliers"] == 40 and out["rms_px"] > 5.0


def test_robust_refinement_lands_on_a_stationary_point_of_its_cost():
    prob, cams_true, pts_true = make_problem(12, 300, 4, outlier_frac=0.05, return_truth=True)
    prob = BAProblem(prob.cams, pts_true, prob.cam_idx, prob.pt_idx, prob.uv, prob.K4, 0)
    for loss in ("linear", "huber", "cauchy"):
        for c in (2, 7):
            o = rr.obs_of(prob, c)
            out = rr.resect(o, prob.cams[c], loss=loss)
            s = rr.sums_at(o, out["pose"], loss, 1.0, 0.0)
            assert out["status"] == rr.OK and np.all(np.abs(s["g"]) <= 1e-9 * s["absgrad"]), (loss, c)


def test_header_declares_both_symbols_and_the_structs_match():
    from bundle_adjustment_amd import hip_backend as hb
    hdr = open(os.path.join(ROOT, "include", "ba_hip.h")).read()
    assert re.search(r"^int ba_default_resect_options\(ba_resect_options\*", hdr, flags=re.M)
    assert re.search(r"^int ba_resect\(ba_handle\*", hdr, flags=re.M)
    assert {"ba_default_resect_options", "ba_resect"} <= set(hb.SYMBOLS)
    body = re.search(r"typedef struct ba_resect_options \{(.*?)\} ba_resect_options;", hdr, flags=re.S).group(1)
    names = re.findall(r"(?:int32_t|double)\s+([a-z_0-9]+)\s*;", body)
    assert names == [n for n, _ in hb.BAResectOptions._fields_]
    assert C.sizeof(hb.BAResectOptions) == 2 * 4 + 8 + 2 * 4 + 3 * 8 + 2 * 4
    enum = dict(re.findall(r"BA_RESECT_(?!INIT)(\w+) = (\d)", hdr))
    assert {k.lower(): int(v) for k, v in enum.items()} == hb.RESECT_STATUS
    init = dict(re.findall(r"BA_RESECT_INIT_(\w+) = (\d)", hdr))
    assert {k.lower(): int(v) for k, v in init.items()} == hb.RESECT_INIT
    assert (rr.OK, rr.FEW_POINTS, rr.DEGENERATE, rr.BEHIND, rr.FEW_INLIERS, rr.HIGH_ERROR) == tuple(range(6))
    assert re.search(r"BA_K_RESECT = (\d+)", hdr).group(1) == str(hb.K_RESECT)
    flat = " ".join(hdr.replace("\n *", " ").split())
    # what is pinned on two ranks: ba_triangulate_tracks, ba_resect, ba_resect_ransac, ba_transform, ba_align -- and the
    # camera writes that are refused there: both resections' write_cams, ba_align's apply with pt_ref
    assert flat.count("Pinned on two ranks (tests/test_gpu_multirank_local.py)") >= 5
    assert flat.count("refused when world > 1") >= 2 and "with apply = 1 and world > 1 it is refused" in flat
    assert "every rank must pass the same similarity" in flat and "untested on" not in hdr


def test_library_exports_ba_resect_and_its_defaults_need_no_gpu():
    import __graft_entry__ as g
    g.build()
    from bundle_adjustment_amd import hip_backend as hb
    lib = hb.load_library()
    assert hasattr(lib, "ba_resect")
    o = hb.BAResectOptions()
    assert lib.ba_default_resect_options(o) == 0
    assert (o.loss, o.refine_iters, o.f_scale, o.init, o.min_inliers, o.max_reproj_px, o.max_rms_px, o.min_depth, o.write_cams,
            o.reserved0) == (0, 20, 1.0, 0, 6, 0.0, 0.0, 0.0, 0, 0)
    assert lib.ba_kernel_name(hb.K_RESECT) == b"resect"
