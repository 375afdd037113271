"""Relative pose of two views from raw matches -- the geometry step that runs on every frame, upstream of triangulation and
bundle adjustment.

Mirrors ``estimate_pose`` of ``src/pose_estimator.py`` (``cv2.findEssentialMat(..., RANSAC, prob=0.999, threshold=3.0)`` then
``cv2.recoverPose``: same arguments, same five-tuple, same log lines) on the GPU (``ba_relative_pose``: five-point hypotheses
scored on all matches, decomposition with cheirality votes, local optimisation on the consensus set).  A fixed number of
hypotheses instead of cv2's adaptive stopping, so the result is not bit-comparable with cv2's; what comes back goes straight
into ``triangulation.triangulate_points``.  No cv2 is needed: matches and keypoints are duck-typed.  No CPU fallback: without
the library / a GPU the call raises.
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
