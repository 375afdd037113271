"""Two-view triangulation + cheirality and the re-observation bookkeeping of a new keyframe -- the step right upstream of
bundle adjustment that creates the landmarks it refines.

Mirrors ``VisualOdometryPipeline._triangulate_points`` (``src/pipeline.py:315-336``: same arguments, same return value
``(points_3d[:3, valid], valid_indices)`` or ``(None, None)``, same log line) on the GPU (``ba_triangulate``), and the
split of a keyframe's inlier matches into re-observations and new points (``src/pipeline.py:248-282``) as array code.
``cv2.triangulatePoints`` is restated from OpenCV's published DLT; the sign of its singular vector is fixed as
``w >= 0`` (parity unpinned at the cv2 boundary).  No CPU fallback: without the library / a GPU the call raises.

``triangulate_tracks`` is the N-view step between two adjustments (``ba_triangulate_tracks``: every point from all of its
observations and the problem's cameras, refined, with triangulation angle, reprojection errors and a status), and
``filter_tracks`` the host-side bookkeeping that drops the rejected points: together the loop
*solve -> triangulate -> filter_tracks -> solve* of an SfM / SLAM pipeline.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import hip_backend


def triangulate_points(camera_matrix, R_rel, t_rel, pts1, pts2, solver=None, quiet=False):
    """-> (3 x n_kept points in the first camera's frame, indices kept), ``src/pipeline.py:315-336``."""
    pts1 = np.ascontiguousarray(pts1, dtype=np.float64).reshape(-1, 2)
    pts2 = np.ascontiguousarray(pts2, dtype=np.float64).reshape(-1, 2)
    if pts1.shape[0] == 0:
        return None, None
    if pts2.shape[0] != pts1.shape[0]:
        raise ValueError("pts1 and pts2 must list the same number of points")
    own = solver is None
    s = hip_backend.Solver(0) if own else solver
    try:
        xyz, valid = s.triangulate(camera_matrix, R_rel, t_rel, pts1, pts2)
    finally:
        if own:
            s.close()
    if not quiet:
        print(f"    -> Triangulation: Kept {int(valid.sum())} of {pts1.shape[0]} points.")
    return xyz[valid].T.copy(), np.where(valid)[0]


def split_reobservations(last_kf_observations, query_idx, train_idx):
    """The bookkeeping loop of ``src/pipeline.py:251-282`` over the inlier matches of a new keyframe, as arrays.
    ``last_kf_observations``: the last keyframe's ``[(mp_id, kp_idx)]``; ``query_idx`` / ``train_idx``: keypoint index
    in the last / new keyframe per inlier match.  Returns ``(is_reobs, mp_id)``: for match i, ``is_reobs[i]`` says the
    last keyframe's keypoint already has a landmark (``mp_id[i]``; the LAST one listed for that keypoint, as the dict
    comprehension of :251 keeps), else it is a new point to triangulate (``mp_id[i] = -1``)."""
    q = np.asarray(query_idx, dtype=np.int64).ravel()
    if len(last_kf_observations) == 0 or q.size == 0:
        return np.zeros(q.size, dtype=bool), -np.ones(q.size, dtype=np.int64)
    ob = np.asarray(last_kf_observations, dtype=np.int64).reshape(-1, 2)
    # later entries overwrite earlier ones for the same keypoint index
    order = np.argsort(ob[:, 1], kind="stable")
    kp_sorted, mp_sorted = ob[order, 1], ob[order, 0]
    last_of_run = np.r_[kp_sorted[1:] != kp_sorted[:-1], True]
    kp_u, mp_u = kp_sorted[last_of_run], mp_sorted[last_of_run]
    pos = np.searchsorted(kp_u, q)
    pos_c = np.minimum(pos, kp_u.size - 1)
    hit = kp_u[pos_c] == q
    return hit, np.where(hit, mp_u[pos_c], -1)


def triangulate_tracks(prob, solver=None, write=False, **opts):
    """Triangulate every point of a ``BAProblem`` from all of its observations and ``prob.cams`` (``ba_triangulate_tracks``;
    opts as ``hip_backend.Solver.triangulate_tracks``: loss, refine_iters, f_scale, min_angle_deg, max_reproj_px, min_depth).
    Returns dict(xyz, status, angle_deg, rms_px, max_px) in ``prob``'s point order; with ``write=True`` also a copy of
    ``prob`` whose OK points that are not held carry the triangulated positions.  ``solver``: a ``hip_backend.Solver`` to
    upload into (its resident problem is replaced); default: one on device 0 for the call."""
    import dataclasses
    own = solver is None
    s = hip_backend.Solver(0) if own else solver
    try:
        s.set_problem(prob)
        out = s.triangulate_tracks(write_points=int(bool(write)), **opts)
        pts = s.get_params()[1] if write else None
    finally:
        if own:
            s.close()
    if not write:
        return out
    return out, dataclasses.replace(prob, pts=pts)


def resect_cameras(prob, solver=None, write=True, cams=None, known_points=None, **opts):
    """Resect the cameras of a pinhole ``BAProblem`` from ``prob.pts``, taken as known (``ba_resect``; cams, known_points
    and opts as ``hip_backend.Solver.resect``: loss, refine_iters, f_scale, init, min_inliers, max_reproj_px, max_rms_px,
    min_depth).  Returns ``(out, problem)``: dict(poses, status, n_inliers, rms_px, max_px) in ``prob``'s camera order and a
    copy of ``prob`` with the merged cameras -- with ``write=True`` the selected cameras that are OK, not the fixed camera and
    have no pose parameter held carry their resected poses; with ``write=False`` the cameras are ``prob``'s.  ``solver``: a
    ``hip_backend.Solver`` to upload into (its resident problem is replaced); default: one on device 0 for the call."""
    import dataclasses
    own = solver is None
    s = hip_backend.Solver(0) if own else solver
    try:
        s.set_problem(prob)
        out = s.resect(cams=cams, known_points=known_points, write_cams=int(bool(write)), **opts)
        merged = s.get_params()[0]
    finally:
        if own:
            s.close()
    return out, dataclasses.replace(prob, cams=merged)


def resect_cameras_ransac(prob, solver=None, write=True, cams=None, known_points=None, **opts):
    """Resect the cameras of a pinhole ``BAProblem`` from raw matches (``ba_resect_ransac``; cams, known_points and opts as
    ``hip_backend.Solver.resect_ransac``: n_hyp, lo_rounds, seed, max_reproj_px, loss, refine_iters, f_scale, min_inliers,
    max_rms_px, min_depth).  Returns ``(out, problem)`` like ``resect_cameras``; ``out["obs_inlier"]`` is the consensus set in
    ``prob``'s observation order, what ``filter_observations`` takes."""
    import dataclasses
    own = solver is None
    s = hip_backend.Solver(0) if own else solver
    try:
        s.set_problem(prob)
        out = s.resect_ransac(cams=cams, known_points=known_points, write_cams=int(bool(write)), **opts)
        merged = s.get_params()[0]
    finally:
        if own:
            s.close()
    return out, dataclasses.replace(prob, cams=merged)


def filter_observations(prob, keep):
    """Drop the observations where ``keep`` (bool (n_obs,)) is false; the others keep their order, and cameras and points keep
    their numbers (a point may be left with fewer than two observations: ``filter_tracks`` is the call for that).  ``prob``: a
    ``BAProblem`` or a ``bal.BALProblem``.  Returns ``(new_problem, old_index_of_new_observation)``.  Pure numpy."""
    import dataclasses
    keep = np.asarray(keep)
    if keep.dtype != np.bool_ or keep.shape != (prob.n_obs,):
        raise ValueError(f"keep must be a bool array of shape ({prob.n_obs},), not {keep.dtype} {keep.shape}")
    old = np.nonzero(keep)[0]
    return dataclasses.replace(prob, cam_idx=prob.cam_idx[old].copy(), pt_idx=prob.pt_idx[old].copy(), uv=prob.uv[old].copy()), old


def filter_tracks(prob, keep):
    """Drop the points where ``keep`` (bool (Np,)) is false together with their observations and renumber ``pt_idx``; the
    remaining observations keep their order.  ``prob``: a ``BAProblem`` or a ``bal.BALProblem``.  Returns
    ``(new_problem, old_index_of_new_point)``.  Held flags and point priors given as arrays follow their points; a dict of
    point priors is re-keyed.  Pure numpy."""
    import dataclasses
    keep = np.asarray(keep)
    if keep.dtype != np.bool_ or keep.shape != (prob.n_pts,):
        raise ValueError(f"keep must be a bool array of shape ({prob.n_pts},), not {keep.dtype} {keep.shape}")
    old = np.nonzero(keep)[0]
    new_of_old = np.full(prob.n_pts, -1, dtype=np.int64)
    new_of_old[old] = np.arange(old.size)
    sel = keep[prob.pt_idx]
    changes = dict(pts=prob.pts[old].copy(), cam_idx=prob.cam_idx[sel].copy(),
                   pt_idx=new_of_old[prob.pt_idx[sel]].astype(np.int32), uv=prob.uv[sel].copy())
    if getattr(prob, "pt_held", None) is not None:
        changes["pt_held"] = np.asarray(prob.pt_held)[old].copy()
    prior = getattr(prob, "pt_prior", None)
    if isinstance(prior, dict):
        changes["pt_prior"] = {int(new_of_old[i]): v for i, v in prior.items() if keep[i]}
    elif prior is not None:
        changes["pt_prior"] = tuple(np.asarray(a)[old].copy() for a in prior)
    return dataclasses.replace(prob, **changes), old
