"""Relative pose of two views from raw matches -- the geometry step that runs on every frame, upstream of triangulation and
bundle adjustment.

Mirrors ``estimate_pose`` of ``src/pose_estimator.py`` (``cv2.findEssentialMat(..., RANSAC, prob=0.999, threshold=3.0)`` then
``cv2.recoverPose``: same arguments, same five-tuple, same log lines) on the GPU (``ba_relative_pose``: five-point hypotheses
scored on all matches, decomposition with cheirality votes, local optimisation on the consensus set).  A fixed number of
hypotheses instead of cv2's adaptive stopping, so the result is not bit-comparable with cv2's; what comes back goes straight
into ``triangulation.triangulate_points``.  ``estimate_two_view`` runs the planar model (``ba_homography``) next to the essential
one and picks between them by COLMAP's inlier-ratio rule: exactly coplanar matches admit two essential matrices of zero cost,
so the first pair of a sequence over a desk or a wall is the homography's to decide.  No cv2 is needed: matches and keypoints
are duck-typed.  No CPU fallback: without the library / a GPU the call raises.
"""
from __future__ import annotations

import numpy as np

from . import hip_backend


def relative_pose(K, pts1, pts2, solver=None, **opts):
    """One pair on arrays: ``hip_backend.Solver.relative_pose`` with the leading pair axis removed -- dict(R (3, 3), t (3,),
    status (int, ``hip_backend.RELPOSE_STATUS``), n_inliers, rms_px, parallax_deg, best_hyp, match_inlier (n,) bool).
    ``solver``: a ``hip_backend.Solver`` to run on (its resident problem is not touched); default: one on device 0 for the call."""
    own = solver is None
    s = hip_backend.Solver(0) if own else solver
    try:
        out = s.relative_pose(K, pts1, pts2, **opts)
    finally:
        if own:
            s.close()
    return dict(R=out["R"][0], t=out["t"][0], status=int(out["status"][0]), n_inliers=int(out["n_inliers"][0]),
                rms_px=float(out["rms_px"][0]), parallax_deg=float(out["parallax_deg"][0]), best_hyp=int(out["best_hyp"][0]),
                match_inlier=out["match_inlier"])


def estimate_pose(matches, kp1, kp2, camera_matrix, solver=None, quiet=False, **opts):
    """-> (R_rel 3 x 3, t_rel 3 x 1, inlier pts1, inlier pts2, inlier indices), ``src/pose_estimator.py:7-43``; five ``None``
    when there is no pose (status few_matches, or degenerate with no hypothesis).  ``matches``: objects with ``queryIdx`` /
    ``trainIdx``; ``kp1`` / ``kp2``: objects with ``pt``.  Points are float32 as there.  opts as ``relative_pose``."""
    pts1 = np.float32([kp1[m.queryIdx].pt for m in matches]).reshape(-1, 2)
    pts2 = np.float32([kp2[m.trainIdx].pt for m in matches]).reshape(-1, 2)
    out = relative_pose(camera_matrix, pts1, pts2, solver=solver, **opts)
    st = hip_backend.RELPOSE_STATUS
    if out["status"] == st["few_matches"] or (out["status"] == st["degenerate"] and out["best_hyp"] < 0):
        return None, None, None, None, None
    num_matches = len(matches)
    num_inliers = int(out["match_inlier"].sum())
    inlier_ratio = num_inliers / num_matches if num_matches > 0 else 0
    if not quiet:
        print(f"    -> Pose Estimation: {num_inliers} inliers out of {num_matches} matches (Ratio: {inlier_ratio:.2f})")
        if inlier_ratio < 0.4:
            print("    -> WARNING: Low inlier ratio. Pose estimate may be unreliable.")
    mask = out["match_inlier"]
    return (np.array(out["R"], dtype=np.float64).reshape(3, 3), np.array(out["t"], dtype=np.float64).reshape(3, 1), pts1[mask], pts2[mask],
            np.where(mask)[0])


def homography(K, pts1, pts2, solver=None, **opts):
    """One pair on arrays: ``hip_backend.Solver.homography`` with the leading pair axis removed -- dict(H (3, 3) in pixels, status
    (int, ``hip_backend.HOMOGRAPHY_STATUS``), n_inliers, rms_px, best_hyp, n_pose, match_inlier (n,) bool, and the two poses, the
    better first: R (2, 3, 3), t, normal (2, 3), t_over_d, votes, pose_cost (2,)).  ``solver`` as ``relative_pose``."""
    own = solver is None
    s = hip_backend.Solver(0) if own else solver
    try:
        out = s.homography(K, pts1, pts2, **opts)
    finally:
        if own:
            s.close()
    return dict(H=out["H"][0], status=int(out["status"][0]), n_inliers=int(out["n_inliers"][0]), rms_px=float(out["rms_px"][0]),
                best_hyp=int(out["best_hyp"][0]), n_pose=int(out["n_pose"][0]), match_inlier=out["match_inlier"], R=out["R"][0],
                t=out["t"][0], normal=out["normal"][0], t_over_d=out["t_over_d"][0], votes=out["votes"][0], pose_cost=out["pose_cost"][0])


def fundamental(pts1, pts2, solver=None, **opts):
    """One pair on arrays: ``hip_backend.Solver.fundamental`` with the leading pair axis removed -- dict(F (3, 3) in pixels
    (p2^T F p1 = 0), status (int, ``hip_backend.FUNDAMENTAL_STATUS``), n_inliers, rms_px, best_hyp, match_inlier (n,) bool,
    epipole1, epipole2 (3,)).  No camera matrix is needed.  ``solver`` as ``relative_pose``."""
    own = solver is None
    s = hip_backend.Solver(0) if own else solver
    try:
        out = s.fundamental(pts1, pts2, **opts)
    finally:
        if own:
            s.close()
    return dict(F=out["F"][0], status=int(out["status"][0]), n_inliers=int(out["n_inliers"][0]), rms_px=float(out["rms_px"][0]),
                best_hyp=int(out["best_hyp"][0]), match_inlier=out["match_inlier"], epipole1=out["epipole1"][0], epipole2=out["epipole2"][0])


def _skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def focal_from_fundamental(F, pp1, pp2):
    """(f1, f2): the focal lengths of the two views from a fundamental matrix (pixels, p2^T F p1 = 0), for square pixels, no skew
    and known principal points ``pp1`` / ``pp2`` -- Bougnoux's closed form (1998), numpy on the host: a first focal length for a
    BAL solve of an uncalibrated pair.  With I~ = diag(1, 1, 0), p_k = (pp_k, 1) and e2 the null vector of F^T,
    f1^2 = -(p2^T [e2]x I~ F p1)(p1^T F^T p2) / (p2^T [e2]x I~ F I~ F^T p2), and f2^2 is the same expression for F^T with e1 and
    the roles of p1 and p2 swapped.  NaN where the squared focal length is not positive (noise, or a wrong principal point) or
    not finite.  Degenerate motions, for which the denominator vanishes and no F determines the focal lengths: optical axes that
    intersect (a camera turning about a point it looks at, which includes parallel axes under a sideways translation), and a pure
    translation along the optical axes."""
    F = np.asarray(F, dtype=np.float64).reshape(3, 3)
    p1 = np.r_[np.asarray(pp1, dtype=np.float64).reshape(2), 1.0]
    p2 = np.r_[np.asarray(pp2, dtype=np.float64).reshape(2), 1.0]
    It = np.diag([1.0, 1.0, 0.0])

    def one(Fm, pa, pb):
        e = np.linalg.svd(Fm.T)[2][2]                # Fm^T e = 0
        ex = _skew(e)
        with np.errstate(divide="ignore", invalid="ignore"):
            f2 = -(pb @ ex @ It @ Fm @ pa) * (pa @ Fm.T @ pb) / (pb @ ex @ It @ Fm @ It @ Fm.T @ pb)
        return float(np.sqrt(f2)) if np.isfinite(f2) and f2 > 0.0 else float("nan")

    return one(F, p1, p2), one(F.T, p2, p1)


_FUNDAMENTAL_OPTS = ("n_hyp", "lo_rounds", "seed", "refine_iters", "min_inliers", "max_epi_px")
_PLANE_OPTS = ("n_hyp", "lo_rounds", "seed", "refine_iters", "min_inliers", "max_px")


def estimate_uncalibrated(matches, kp1, kp2, solver=None, planar_ratio=0.8, quiet=False, **opts):
    """Two-view geometry of an UNCALIBRATED pair: ``fundamental`` (``ba_fundamental``) on the matches, and ``homography`` beside it
    for the degeneracy no fundamental matrix can see -- a plane (or a pure rotation) admits a family of them.
    -> (F 3 x 3 in pixels, inlier pts1, inlier pts2, inlier indices, info); four ``None`` in front of ``info`` when there is no
    F (status few_matches, or degenerate with no hypothesis).  ``info``: ``model`` -- "planar" when ``n_inliers_H >= planar_ratio *
    n_inliers_F`` (COLMAP's planar-or-panoramic rule: F is still returned, it explains the matches, but it is NOT unique and its
    epipoles mean nothing), else "fundamental" --, ``unique`` (model == "fundamental"), ``fundamental`` and ``homography`` (the two
    calls' outputs).  The homography runs with K = [f0 0 cx; 0 f0 cy; 0 0 1], f0 = 1000 and (cx, cy) the centroid of both images'
    matches: its H, n_inliers and match_inlier do not depend on that K beyond rounding; its poses do, and are not returned.
    ``matches`` / ``kp*`` as ``estimate_pose`` (points are float32 as there).  opts: n_hyp, lo_rounds, seed, refine_iters,
    min_inliers go to both calls; max_epi_px to the fundamental matrix, max_px to the homography."""
    for k in opts:
        if k not in _FUNDAMENTAL_OPTS + _PLANE_OPTS:
            raise TypeError(f"unknown option {k}")
    pts1 = np.float32([kp1[m.queryIdx].pt for m in matches]).reshape(-1, 2)
    pts2 = np.float32([kp2[m.trainIdx].pt for m in matches]).reshape(-1, 2)
    own = solver is None
    s = hip_backend.Solver(0) if own else solver
    try:
        f = fundamental(pts1, pts2, solver=s, **{k: v for k, v in opts.items() if k in _FUNDAMENTAL_OPTS})
        centre = np.concatenate([pts1, pts2]).astype(np.float64).mean(axis=0) if len(pts1) else np.zeros(2)
        K0 = np.array([[1000.0, 0.0, centre[0]], [0.0, 1000.0, centre[1]], [0.0, 0.0, 1.0]])
        h = homography(K0, pts1, pts2, solver=s, **{k: v for k, v in opts.items() if k in _PLANE_OPTS})
    finally:
        if own:
            s.close()
    info = dict(model="fundamental", unique=True, fundamental=f, homography=h)
    st = hip_backend.FUNDAMENTAL_STATUS
    if f["status"] == st["few_matches"] or (f["status"] == st["degenerate"] and f["best_hyp"] < 0):
        return None, None, None, None, info
    if h["best_hyp"] >= 0 and h["n_inliers"] >= planar_ratio * f["n_inliers"]:
        info.update(model="planar", unique=False)
    mask = f["match_inlier"]
    if not quiet:
        num_matches = len(matches)
        num_inliers = int(mask.sum())
        inlier_ratio = num_inliers / num_matches if num_matches > 0 else 0
        print(f"    -> Two-view model: {info['model']} ({h['n_inliers']} homography inliers, {f['n_inliers']} fundamental)")
        print(f"    -> Fundamental matrix: {num_inliers} inliers out of {num_matches} matches (Ratio: {inlier_ratio:.2f})")
        if info["model"] == "planar":
            print("    -> WARNING: Planar or panoramic pair. The fundamental matrix is not unique.")
    return np.array(f["F"], dtype=np.float64).reshape(3, 3), pts1[mask], pts2[mask], np.where(mask)[0], info


_BOTH = ("n_hyp", "lo_rounds", "seed", "refine_iters", "min_inliers", "max_depth")
_ESSENTIAL_ONLY = ("max_epi_px", "min_parallax_deg")
_HOMOGRAPHY_ONLY = ("max_px", "ambiguity_ratio", "min_translation")


def estimate_two_view(matches, kp1, kp2, camera_matrix, solver=None, planar_ratio=0.8, quiet=False, **opts):
    """``estimate_pose`` with planar model selection: both ``relative_pose`` (essential matrix) and ``homography`` run on the same
    matches, and the homography's first pose is taken when ``n_inliers_H >= planar_ratio * n_inliers_E`` (COLMAP's
    ``max_H_inlier_ratio``), its status is ok and that pose carries the most votes; otherwise the essential pose.
    -> ``estimate_pose``'s five values and a dict: ``model`` ("essential", "homography", "rotation", "ambiguous"), ``essential`` and
    ``homography`` (the two calls' outputs), ``normal`` (the plane's, or None) and ``second_pose`` ((R, t 3 x 1, normal) of the
    homography's other pose, or None).  "rotation" (no translation to triangulate with: R alone, t = 0) and "ambiguous" (two poses
    explain the plane equally well; the first is returned, the other is ``second_pose``) come with the pose but with empty inlier
    arrays: nothing to triangulate, the reference would discard such a frame.  With model "essential" the five values are
    ``estimate_pose``'s, bit for bit.  opts: n_hyp, lo_rounds, seed, refine_iters, min_inliers, max_depth go to both calls;
    max_epi_px, min_parallax_deg to the essential one; max_px, ambiguity_ratio, min_translation to the homography."""
    for k in opts:
        if k not in _BOTH + _ESSENTIAL_ONLY + _HOMOGRAPHY_ONLY:
            raise TypeError(f"unknown option {k}")
    pts1 = np.float32([kp1[m.queryIdx].pt for m in matches]).reshape(-1, 2)
    pts2 = np.float32([kp2[m.trainIdx].pt for m in matches]).reshape(-1, 2)
    own = solver is None
    s = hip_backend.Solver(0) if own else solver
    try:
        e = relative_pose(camera_matrix, pts1, pts2, solver=s, **{k: v for k, v in opts.items() if k in _BOTH + _ESSENTIAL_ONLY})
        h = homography(camera_matrix, pts1, pts2, solver=s, **{k: v for k, v in opts.items() if k in _BOTH + _HOMOGRAPHY_ONLY})
    finally:
        if own:
            s.close()
    hs = hip_backend.HOMOGRAPHY_STATUS
    info = dict(model="essential", essential=e, homography=h, normal=None, second_pose=None)
    planar = h["best_hyp"] >= 0 and h["n_inliers"] >= planar_ratio * e["n_inliers"]
    if planar and h["status"] == hs["ok"] and h["n_pose"] >= 1 and h["votes"][0] > h["votes"][1]:
        info["model"] = "homography"
    elif planar and h["status"] == hs["rotation"]:
        info["model"] = "rotation"
    elif planar and h["status"] == hs["ambiguous"] and h["n_pose"] >= 1:
        info["model"] = "ambiguous"
    num_matches = len(matches)
    if info["model"] == "essential":
        st = hip_backend.RELPOSE_STATUS
        if e["status"] == st["few_matches"] or (e["status"] == st["degenerate"] and e["best_hyp"] < 0):
            return None, None, None, None, None, info
        R, t, mask = e["R"], e["t"], e["match_inlier"]
    else:
        R, t = h["R"][0], h["t"][0]
        mask = h["match_inlier"] if info["model"] == "homography" else np.zeros(num_matches, dtype=bool)
        if info["model"] != "rotation":
            info["normal"] = np.array(h["normal"][0], dtype=np.float64)
            info["second_pose"] = (np.array(h["R"][1], dtype=np.float64), np.array(h["t"][1], dtype=np.float64).reshape(3, 1),
                                   np.array(h["normal"][1], dtype=np.float64))
    if not quiet:
        num_inliers = int(mask.sum())
        inlier_ratio = num_inliers / num_matches if num_matches > 0 else 0
        if info["model"] != "essential":
            print(f"    -> Two-view model: {info['model']} ({h['n_inliers']} homography inliers, {e['n_inliers']} essential)")
        print(f"    -> Pose Estimation: {num_inliers} inliers out of {num_matches} matches (Ratio: {inlier_ratio:.2f})")
        if inlier_ratio < 0.4 and info["model"] in ("essential", "homography"):
            print("    -> WARNING: Low inlier ratio. Pose estimate may be unreliable.")
    return (np.array(R, dtype=np.float64).reshape(3, 3), np.array(t, dtype=np.float64).reshape(3, 1), pts1[mask], pts2[mask],
            np.where(mask)[0], info)
