"""Pose-graph bookkeeping around ``ba_pose_graph`` (``include/ba_hip.h``): the step that spreads the drift a loop closure
reveals over the keyframes before the global adjustment (ORB-SLAM's ``OptimizeEssentialGraph`` / ``CorrectLoop``).

A node is a world-to-node similarity ``x = s R X + t`` stored as ``rvec | t | s``; an edge ``(i, j)`` carries the measured
``S_j o S_i^-1``.  The node ``(s, R, t)`` is the camera ``R | t / s``: both camera models divide by depth, so a camera frame
scaled by ``s`` sees the same pixels (``ba_transform``'s argument, per keyframe).

Everything here is numpy but two calls of the GPU: ``loop_measurement`` (``hip_backend.Solver.sim3``, the loop edge's
``meas`` and ``info`` from matched map points) and ``close_loop`` (``hip_backend.Solver.pose_graph``).
"""
from __future__ import annotations

import dataclasses

import numpy as np

from .rotations import rvecs_to_matrices
from .similarity import log_map


def from_cameras(cams):
    """(Nc, >= 6) cameras ``rvec | t | ...`` -> (Nc, 7) nodes ``rvec | t | 1``."""
    cams = np.asarray(cams, dtype=np.float64)
    return np.concatenate([cams[:, :6], np.ones((cams.shape[0], 1))], axis=1)


def to_cameras(poses):
    """(n, 7) nodes -> (n, 6) cameras ``rvec | t / s``."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 7)
    return np.concatenate([poses[:, :3], poses[:, 3:6] / poses[:, 6:7]], axis=1)


def compose(outer, inner):
    """``outer o inner`` of similarities ``rvec | t | s`` given as (m, 7) rows (either may be (1, 7))."""
    Ro, Ri = rvecs_to_matrices(outer[:, :3]), rvecs_to_matrices(inner[:, :3])
    out = np.empty((max(outer.shape[0], inner.shape[0]), 7))
    out[:, :3] = log_map(Ro @ Ri)
    out[:, 3:6] = outer[:, 6:7] * np.einsum("nij,nj->ni", Ro, inner[:, 3:6]) + outer[:, 3:6]
    out[:, 6] = outer[:, 6] * inner[:, 6]
    return out


def inverse(sim):
    """The inverse similarities of (m, 7) rows ``rvec | t | s``."""
    R = rvecs_to_matrices(sim[:, :3])
    out = np.empty(sim.shape)
    out[:, :3] = -sim[:, :3]
    out[:, 3:6] = -np.einsum("nji,nj->ni", R, sim[:, 3:6]) / sim[:, 6:7]
    out[:, 6] = 1.0 / sim[:, 6]
    return out


def relative(pose_i, pose_j):
    """The ``meas`` an edge between two nodes would carry: ``S_j o S_i^-1`` as ``rvec | t | s`` ((7,) or (m, 7))."""
    a, b = np.asarray(pose_i, dtype=np.float64), np.asarray(pose_j, dtype=np.float64)
    out = compose(b.reshape(-1, 7), inverse(a.reshape(-1, 7)))
    return out[0] if a.ndim == 1 and b.ndim == 1 else out


def covisibility_edges(cam_idx, pt_idx, n_cams, poses, min_shared=15):
    """An edge for every camera pair that shares at least ``min_shared`` points: ``(edge_i, edge_j, meas, info)`` with
    ``i < j`` in key order, ``meas = relative(poses[i], poses[j])`` of the current poses and ``info = shared count x I``.
    Vectorised: the observations are sorted by point, partners ``d`` places apart inside a track give the pair keys, and the
    keys are counted by a sort (the only Python loop runs over the track length)."""
    cam_idx, pt_idx = np.asarray(cam_idx, dtype=np.int64), np.asarray(pt_idx, dtype=np.int64)
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 7)
    obs = np.unique(pt_idx * n_cams + cam_idx)            # sorted by point, then camera; a (camera, point) pair once
    pt, cam = obs // n_cams, obs % n_cams
    keys = []
    d = 1
    while d < obs.shape[0]:
        same = pt[d:] == pt[:-d]
        if not same.any():
            break
        keys.append(cam[:-d][same] * n_cams + cam[d:][same])      # cam ascending inside a track: lower index first
        d += 1
    if not keys:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 7)), np.zeros((0, 7, 7))
    key, count = np.unique(np.concatenate(keys), return_counts=True)
    keep = count >= min_shared
    key, count = key[keep], count[keep]
    ei, ej = (key // n_cams).astype(np.int32), (key % n_cams).astype(np.int32)
    meas = relative(poses[ei], poses[ej]) if ei.size else np.zeros((0, 7))
    info = count[:, None, None].astype(np.float64) * np.eye(7)
    return ei, ej, meas, info


def correct_points(points, ref_cam, poses_old, poses_new):
    """``X' = S_new^-1 (S_old X)`` with the similarities of each point's reference camera (ORB-SLAM's ``CorrectLoop``): the
    point keeps its coordinates in that keyframe's frame.  ``ref_cam`` (Np,) int, -1 = leave the point where it is."""
    pts = np.array(points, dtype=np.float64).reshape(-1, 3)
    ref = np.asarray(ref_cam, dtype=np.int64).reshape(-1)
    old, new = np.asarray(poses_old, dtype=np.float64).reshape(-1, 7), np.asarray(poses_new, dtype=np.float64).reshape(-1, 7)
    sel = ref >= 0
    o, n = old[ref[sel]], new[ref[sel]]
    x = o[:, 6:7] * np.einsum("nij,nj->ni", rvecs_to_matrices(o[:, :3]), pts[sel]) + o[:, 3:6]
    pts[sel] = np.einsum("nji,nj->ni", rvecs_to_matrices(n[:, :3]), x - n[:, 3:6]) / n[:, 6:7]
    return pts


def first_observers(cam_idx, pt_idx, n_pts):
    """(Np,) the camera of each point's first observation (in observation order), -1 for a point nobody sees."""
    cam_idx, pt_idx = np.asarray(cam_idx, dtype=np.int64), np.asarray(pt_idx, dtype=np.int64)
    ref = np.full(n_pts, -1, dtype=np.int64)
    ref[pt_idx[::-1]] = cam_idx[::-1]          # the earliest observation is written last
    return ref


def edge_information(sim, hessian, sigma_px=1.0):
    """The ``info`` of a pose-graph edge from ``Solver.sim3``'s ``sim`` ((7,) or (m, 7)) and ``hessian`` ((7, 7) or (m, 7, 7)):
    ``T H T^T / sigma_px^2`` with ``T = diag(R_ij^T, I, 1)``.  The call's chart moves the model by ``R <- exp(d omega) R, t <- t +
    d t, s <- s exp(d sigma)``; the edge residual ``e = [log(R_ij^T R_r); t_r - t_ij; ln(s_r / s_ij)]`` of a relative pose that far
    from the measurement is ``[R_ij^T d omega; d t; d sigma]`` to first order, so ``d = T^T e`` and ``0.5 d^T H d = 0.5 e^T (T H T^T)
    e``.  ``sigma_px``: the standard deviation of a reprojection residual in pixels (``hessian`` is in pixels^-2)."""
    sim, H = np.asarray(sim, dtype=np.float64), np.asarray(hessian, dtype=np.float64)
    S, Hm = sim.reshape(-1, 7), H.reshape(-1, 7, 7)
    T = np.zeros((S.shape[0], 7, 7))
    T[:, :3, :3] = np.transpose(rvecs_to_matrices(S[:, :3]), (0, 2, 1))
    T[:, 3, 3] = T[:, 4, 4] = T[:, 5, 5] = T[:, 6, 6] = 1.0
    info = T @ Hm @ np.transpose(T, (0, 2, 1)) / float(sigma_px) ** 2
    info = 0.5 * (info + np.transpose(info, (0, 2, 1)))
    return info[0] if sim.ndim == 1 else info


_FLIP = np.array([1.0, -1.0, -1.0])            # F = diag(1, -1, -1): BAL's camera frame (looks down -z) <-> the pinhole one


def _camera_frame(prob, cam, pt):
    """``pt`` -- (n,) indices into ``prob.pts`` or (n, 3) world coordinates -- in the frame of camera ``cam``."""
    pt = np.asarray(pt)
    X = prob.pts[pt.astype(np.int64)] if pt.ndim == 1 and np.issubdtype(pt.dtype, np.integer) else np.asarray(pt, dtype=np.float64).reshape(-1, 3)
    c = np.asarray(prob.cams[cam], dtype=np.float64)
    return X @ rvecs_to_matrices(c[:3])[0].T + c[3:6]


def loop_measurement(prob, i, j, pt_i, pt_j, K=None, solver=None, sigma_px=1.0, **opts):
    """The measurement of the loop edge ``(i, j)`` of a ``BAProblem`` or ``bal.BALProblem`` from matched map points: ``pt_i[k]``
    (seen by camera ``i``) and ``pt_j[k]`` (seen by camera ``j``) are the same physical point, given as (n,) indices into
    ``prob.pts`` or (n, 3) world coordinates; a share of the matches may be wrong.  The points are moved into the two camera
    frames and ``Solver.sim3`` finds ``S_j o S_i^-1``.  Returns ``(meas (7,), info (7, 7), inlier (n,) bool, out)``, ready for
    ``close_loop(prob, [i], [j], [meas], loop_info=[info])``; ``out`` is ``Solver.sim3``'s dict in the pinhole frames the call
    saw.  A status other than OK raises ValueError naming it.  ``K``: (3, 3), default the problem's (``diag(f_j, f_j, 1)`` for
    a BAL problem, whose frames are conjugated with ``F = diag(1, -1, -1)``: ``R = F R' F, t = F t'``, the Hessian's rotation and
    translation blocks likewise).  ``solver``: a ``hip_backend.Solver`` to run on (its resident problem stays); default: one on
    device 0 for the call.  ``sigma_px``: ``edge_information``'s.  opts: ``ba_sim3_options``."""
    from . import hip_backend
    bal = np.asarray(prob.cams).shape[1] == 9
    Xi, Xj = _camera_frame(prob, i, pt_i), _camera_frame(prob, j, pt_j)
    if Xi.shape[0] != Xj.shape[0]:
        raise ValueError("pt_i and pt_j list different numbers of points")
    if bal:
        Xi, Xj = Xi * _FLIP, Xj * _FLIP
    if K is None:
        if bal:
            f = float(prob.cams[j, 6])
            K = np.diag([f, f, 1.0])
        else:
            fx, fy, cx, cy = (float(v) for v in prob.K4)
            K = np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])
    own = solver is None
    if own:
        solver = hip_backend.Solver(0)
    try:
        out = solver.sim3(K, Xi, Xj, **opts)
    finally:
        if own:
            solver.close()
    status = int(out["status"][0])
    if status != hip_backend.SIM3_STATUS["ok"]:
        name = {v: k for k, v in hip_backend.SIM3_STATUS.items()}.get(status, str(status))
        raise ValueError(f"loop_measurement: ba_sim3 status {name} ({int(out['n_inliers'][0])} inliers of {Xi.shape[0]} matches)")
    R, t, s, H = out["R"][0], out["sim"][0, 3:6], out["sim"][0, 6], out["hessian"][0]
    if bal:
        T = np.r_[_FLIP, _FLIP, 1.0]
        R, t, H = R * np.outer(_FLIP, _FLIP), t * _FLIP, H * np.outer(T, T)
    meas = np.r_[log_map(R[None])[0], t, s]
    return meas, edge_information(meas, H, sigma_px), out["match_inlier"], out


def close_loop(prob, loop_i, loop_j, loop_meas, loop_info=None, held=(0,), solver=None, min_shared=15, **opts):
    """Close a loop on a ``BAProblem`` or ``bal.BALProblem``: covisibility edges of the current cameras plus the loop edges
    ``(loop_i, loop_j)`` with ``loop_meas`` (k, 7) / ``loop_info`` (k, 7, 7) (None: the largest covisibility weight x I) ->
    ``Solver.pose_graph`` with the nodes in ``held`` constant -> cameras ``R | t / s`` and points moved with their first
    observer.  Returns ``(out, corrected problem)``, ``out`` as ``Solver.pose_graph``'s dict plus ``edge_i`` / ``edge_j``
    (the loop edges are the last ``k``).  ``solver``: a ``hip_backend.Solver`` to run on (its resident problem stays);
    default: one on device 0 for the call.  opts: ``ba_posegraph_options``."""
    cams = np.asarray(prob.cams, dtype=np.float64)
    n = cams.shape[0]
    poses = from_cameras(cams)
    ei, ej, meas, info = covisibility_edges(prob.cam_idx, prob.pt_idx, n, poses, min_shared)
    li = np.atleast_1d(np.asarray(loop_i, dtype=np.int32))
    lj = np.atleast_1d(np.asarray(loop_j, dtype=np.int32))
    lm = np.asarray(loop_meas, dtype=np.float64).reshape(-1, 7)
    if not (li.shape[0] == lj.shape[0] == lm.shape[0]):
        raise ValueError("loop_i, loop_j and loop_meas list different numbers of edges")
    if loop_info is None:
        top = float(info[:, 0, 0].max()) if info.shape[0] else 1.0
        linfo = np.broadcast_to(top * np.eye(7), (li.shape[0], 7, 7))
    else:
        linfo = np.asarray(loop_info, dtype=np.float64).reshape(-1, 7, 7)
    ei, ej = np.concatenate([ei, li]), np.concatenate([ej, lj])
    meas, info = np.concatenate([meas, lm]), np.concatenate([info, linfo])
    hm = np.zeros(n, np.uint8)
    hm[list(held)] = 1
    own = solver is None
    if own:
        from . import hip_backend
        solver = hip_backend.Solver(0)
    try:
        out = solver.pose_graph(poses, ei, ej, meas, info=info, held=hm, **opts)
    finally:
        if own:
            solver.close()
    out = dict(out, edge_i=ei, edge_j=ej)
    new_cams = cams.copy()
    new_cams[:, :6] = to_cameras(out["poses"])
    pts = correct_points(prob.pts, first_observers(prob.cam_idx, prob.pt_idx, prob.pts.shape[0]), poses, out["poses"])
    return out, dataclasses.replace(prob, cams=new_cams, pts=pts)
