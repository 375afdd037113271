"""Similarity transforms of a reconstruction: ``X' = s R X + t`` (``include/ba_hip.h``: ``ba_transform``, ``ba_align``).

A bundle adjustment fixes a reconstruction only up to these seven parameters.  A world-to-camera pose ``(R_c, t_c)``
becomes ``R_c' = R_c R^T``, ``t_c' = s t_c - R_c' t``: camera-frame coordinates are ``s`` times the old ones and both camera
models divide by depth, so every residual is unchanged and ``f, k1, k2`` / ``K4`` are not touched.

``compose``, ``inverse`` and ``apply`` are pure numpy (host bookkeeping on problems that are not resident);
``align`` estimates the similarity on the GPU (``ba_align``: weighted, robust Umeyama) and returns the transformed problem
the device wrote.  The rotation vectors come from the quaternion log map, NOT from ``rotations.matrices_to_rvecs``, which
follows ``cv2.Rodrigues`` and is off by up to 2e-5 near pi and 1e-6 near 0: fine for packing a keyframe once, not for a
change of frame that must leave every residual where it was.

fp64 in a far-away frame costs residual precision (``|t| = 5e6`` moves residuals by 3e-7 px): subtract a local origin from
UTM-like references before aligning to them.
"""
from __future__ import annotations

import dataclasses

import numpy as np

from .rotations import rvecs_to_matrices


def _srt(s, R, t):
    return float(s), np.asarray(np.eye(3) if R is None else R, dtype=np.float64).reshape(3, 3), \
        np.asarray(np.zeros(3) if t is None else t, dtype=np.float64).reshape(3)


def compose(outer, inner):
    """(s, R, t) of ``x -> outer(inner(x))``."""
    s2, R2, t2 = _srt(*outer)
    s1, R1, t1 = _srt(*inner)
    return s2 * s1, R2 @ R1, s2 * (R2 @ t1) + t2


def inverse(sim):
    """(s, R, t) of the inverse map: ``X = (1 / s) R^T (X' - t)``."""
    s, R, t = _srt(*sim)
    return 1.0 / s, R.T.copy(), -(R.T @ t) / s


def log_map(Rs):
    """(n, 3, 3) rotation matrices -> (n, 3) rotation vectors, ``|rvec| <= pi``, through the unit quaternion picked by the
    largest of trace and diagonal entries (Shepperd), ``w >= 0``, ``theta = 2 atan2(|v|, w)``; exact to rounding at every
    angle from 0 to pi."""
    R = np.asarray(Rs, dtype=np.float64).reshape(-1, 3, 3)
    tr = R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2]
    which = np.argmax(np.stack([tr, R[:, 0, 0], R[:, 1, 1], R[:, 2, 2]], axis=1), axis=1)
    q = np.empty((R.shape[0], 4))                   # 4 q_k (w, x, y, z), q_k the largest component
    forms = (
        (1.0 + tr, R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]),
        (R[:, 2, 1] - R[:, 1, 2], 1.0 + R[:, 0, 0] - R[:, 1, 1] - R[:, 2, 2], R[:, 0, 1] + R[:, 1, 0], R[:, 0, 2] + R[:, 2, 0]),
        (R[:, 0, 2] - R[:, 2, 0], R[:, 0, 1] + R[:, 1, 0], 1.0 + R[:, 1, 1] - R[:, 0, 0] - R[:, 2, 2], R[:, 1, 2] + R[:, 2, 1]),
        (R[:, 1, 0] - R[:, 0, 1], R[:, 0, 2] + R[:, 2, 0], R[:, 1, 2] + R[:, 2, 1], 1.0 + R[:, 2, 2] - R[:, 0, 0] - R[:, 1, 1]),
    )
    for k, form in enumerate(forms):
        m = which == k
        for j in range(4):
            q[m, j] = form[j][m]
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q[q[:, 0] < 0] *= -1.0
    vn = np.linalg.norm(q[:, 1:], axis=1)
    small = vn < 1e-10
    k = np.where(small, 2.0 / np.where(small, q[:, 0], 1.0), 2.0 * np.arctan2(vn, q[:, 0]) / np.where(small, 1.0, vn))
    return q[:, 1:] * k[:, None]


_log_map = log_map


def _transform_arrays(cams, pts, s=1.0, R=None, t=None):
    """The similarity applied to (Nc, >= 6) cameras ``rvec | t | ...`` (further columns are kept) and (Np, 3) points."""
    s, R, t = _srt(s, R, t)
    if not (np.isfinite(s) and s > 0):
        raise ValueError("the scale s must be finite and positive")
    if np.abs(R @ R.T - np.eye(3)).max() > 1e-9 or np.linalg.det(R) < 0:
        raise ValueError("R must be a rotation matrix")
    cams = np.array(cams, dtype=np.float64)
    Rn = rvecs_to_matrices(cams[:, :3]) @ R.T
    tn = s * cams[:, 3:6] - Rn @ t
    cams[:, :3] = log_map(Rn)
    cams[:, 3:6] = tn
    return cams, s * (np.asarray(pts, dtype=np.float64) @ R.T) + t


def apply(prob, s=1.0, R=None, t=None):
    """A copy of ``prob`` (``BAProblem`` or ``bal.BALProblem``) in the frame ``X' = s R X + t``; residuals, intrinsics,
    masks and groups unchanged.  Priors are not transformed: a problem that carries them is refused (ValueError)."""
    if getattr(prob, "cam_prior", None) is not None or getattr(prob, "pt_prior", None) is not None:
        raise ValueError("similarity.apply: the problem carries priors, whose means live in the old frame")
    cams, pts = _transform_arrays(prob.cams, prob.pts, s, R, t)
    return dataclasses.replace(prob, cams=cams, pts=pts)


def _centres(cams):
    """(Nc, 3) camera centres ``-R_c^T t_c`` of (Nc, >= 6) cameras."""
    cams = np.asarray(cams, dtype=np.float64)
    return -np.einsum("nji,nj->ni", rvecs_to_matrices(cams[:, :3]), cams[:, 3:6])


def align(prob, cam_ref=None, pt_ref=None, cam_w=None, pt_w=None, loss="linear", f_scale=1.0, iters=10, with_scale=True,
          solver=None):
    """Align a ``BAProblem`` to reference positions on the GPU (``ba_align`` with apply = 1; arguments as
    ``hip_backend.Solver.align``).  Returns ``(result dict, transformed problem)``; when the status is not OK the problem
    comes back unchanged.  ``solver``: a ``hip_backend.Solver`` to upload into (its resident problem is replaced);
    default: one on device 0 for the call.  A problem with priors is refused: align first, set priors afterwards."""
    from . import hip_backend
    if getattr(prob, "cam_prior", None) is not None or getattr(prob, "pt_prior", None) is not None:
        raise ValueError("similarity.align: the problem carries priors, whose means live in the old frame")
    own = solver is None
    s = hip_backend.Solver(0) if own else solver
    try:
        s.set_problem(prob)
        res = s.align(cam_ref=cam_ref, pt_ref=pt_ref, cam_w=cam_w, pt_w=pt_w, loss=loss, f_scale=f_scale, iters=iters,
                      with_scale=with_scale, apply=True)
        cams, pts = s.get_params()
    finally:
        if own:
            s.close()
    return res, dataclasses.replace(prob, cams=cams, pts=pts)
