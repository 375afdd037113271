"""BAL ("Bundle Adjustment in the Large") problems: text reader / writer and the 9-parameter BAL camera
(SURVEY.md section 8f row 2).  The reference itself only has the shared-intrinsics pinhole of
``cv2.projectPoints(..., distCoeffs=None)`` (``src/bundle_adjuster.py:67``); BAL is the public format BASELINE config 5
("BAL-style Ladybug 1723-cam / 156k-point problem") is stated in.

File format (Agarwal et al., grail.cs.washington.edu/projects/bal)::

    <num_cameras> <num_points> <num_observations>
    <camera_index> <point_index> <x> <y>            one line per observation
    <camera parameter>                              9 lines per camera: rvec(3) t(3) f k1 k2
    <point coordinate>                              3 lines per point

Camera model: ``P = R(rvec) X + t;  p = -P[:2] / P[2]`` (the camera looks down -z);
``r = 1 + k1 |p|^2 + k2 |p|^4``; projection ``f r p`` (origin at the image centre).  Residual = observed - projected, x
then y, the reference's sign (``src/bundle_adjuster.py:68-69``).

What runs where: ``read_bal`` / ``write_bal`` are host code; ``Solver.residuals_bal`` evaluates the BAL residual on the
GPU (``ba_residuals_bal``: K1 with per-camera ``f, k1, k2``); ``to_pinhole`` converts a BAL problem whose cameras share
one focal length and have no distortion into the reference's model (z flipped, shared K), which the LM / Schur / PCG
solver then adjusts as it stands; ``solve`` / ``Solver.solve_bal`` adjust the full 9-parameter cameras (``ba_solve_bal``:
the same kernels and host loop as ``ba_solve``, instantiated for the ``BalCam`` model of ``csrc/ba_models.hpp`` -- LM + Schur
+ PCG with 2x9 camera blocks, ``jacobian_precision`` and multi-rank jobs included; checked step by step against
``oracle.lm_solve(model='bal')``, which is test infrastructure and never imported here), ``Solver.linearize_bal`` returns
the block normal equations (``ba_linearize_bal``).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from .problem import BAProblem


@dataclass
class BALProblem:
    cams: np.ndarray        # (Nc,9) float64  [rvec | tvec | f k1 k2]
    pts: np.ndarray         # (Np,3) float64
    cam_idx: np.ndarray     # (Nobs,) int32
    pt_idx: np.ndarray      # (Nobs,) int32
    uv: np.ndarray          # (Nobs,2) float64, origin at the image centre

    @property
    def n_cams(self):
        return int(self.cams.shape[0])

    @property
    def n_pts(self):
        return int(self.pts.shape[0])

    @property
    def n_obs(self):
        return int(self.cam_idx.shape[0])

    def validate(self):
        if self.cams.ndim != 2 or self.cams.shape[1] != 9 or self.pts.ndim != 2 or self.pts.shape[1] != 3:
            raise ValueError("cams must be (Nc,9) and pts (Np,3)")
        if self.pt_idx.shape != (self.n_obs,) or self.uv.shape != (self.n_obs, 2):
            raise ValueError("observation arrays disagree in length")
        if self.n_obs and (self.cam_idx.min() < 0 or self.cam_idx.max() >= self.n_cams or
                           self.pt_idx.min() < 0 or self.pt_idx.max() >= self.n_pts):
            raise ValueError("observation index out of range")
        return self


def read_bal(path) -> BALProblem:
    """Parse a BAL text file (plain or .bz2 / .gz).  Whitespace-separated numbers; line structure is not required."""
    import bz2
    import gzip
    opener = bz2.open if str(path).endswith(".bz2") else gzip.open if str(path).endswith(".gz") else open
    with opener(path, "rt") as f:
        head = f.readline().split()
        while len(head) < 3:                                   # header split over lines
            more = f.readline()
            if not more:
                raise ValueError("truncated BAL header")
            head += more.split()
        nc, npt, nobs = int(head[0]), int(head[1]), int(head[2])
        rest = np.array(head[3:] + f.read().split(), dtype=np.float64)
    need = 4 * nobs + 9 * nc + 3 * npt
    if rest.size != need:
        raise ValueError(f"BAL file holds {rest.size} numbers after the header, {need} expected for "
                         f"{nc} cameras / {npt} points / {nobs} observations")
    obs = rest[:4 * nobs].reshape(nobs, 4)
    if nobs and (np.any(obs[:, :2] != np.floor(obs[:, :2]))):
        raise ValueError("non-integer camera / point index in the observation block")
    cams = rest[4 * nobs:4 * nobs + 9 * nc].reshape(nc, 9).copy()
    pts = rest[4 * nobs + 9 * nc:].reshape(npt, 3).copy()
    return BALProblem(cams, pts, obs[:, 0].astype(np.int32), obs[:, 1].astype(np.int32), obs[:, 2:].copy()).validate()


def write_bal(path, prob: BALProblem):
    """Write the BAL text format; numbers with 17 significant digits (``read_bal(write_bal(p))`` is exact)."""
    prob.validate()
    with open(path, "w") as f:
        f.write(f"{prob.n_cams} {prob.n_pts} {prob.n_obs}\n")
        for c, p, (x, y) in zip(prob.cam_idx.tolist(), prob.pt_idx.tolist(), prob.uv.tolist()):
            f.write(f"{c} {p}     {x!r} {y!r}\n")
        for v in prob.cams.ravel().tolist():
            f.write(f"{v!r}\n")
        for v in prob.pts.ravel().tolist():
            f.write(f"{v!r}\n")


def to_pinhole(prob: BALProblem, tol=0.0) -> BAProblem:
    """The same problem in the reference's camera model, possible when every BAL camera has the same focal length
    and no distortion (|k1|, |k2| <= tol): BAL projects ``-f P / P.z``; with ``S = diag(1, -1, -1)`` the camera
    ``(S R, S t)`` looking down +z with ``K4 = (f, -f, 0, 0)`` (a negative fy stands for BAL's y axis) gives
    ``u = f X'/Z' ... `` identical pixels.  Raises when the cameras do not allow it."""
    from .rotations import matrices_to_rvecs, rvecs_to_matrices
    f = prob.cams[:, 6]
    if np.ptp(f) > tol * max(1.0, abs(f[0])) or np.abs(prob.cams[:, 7:]).max() > tol:
        raise ValueError("to_pinhole needs one shared focal length and zero distortion")
    S = np.diag([1.0, -1.0, -1.0])
    R = S @ rvecs_to_matrices(prob.cams[:, :3])
    t = prob.cams[:, 3:6] @ S.T
    cams = np.concatenate([matrices_to_rvecs(R), t], axis=1)
    # BAL: u = -f Px/Pz, v = -f Py/Pz.  With P' = S P: Px' = Px, Py' = -Py, Pz' = -Pz  ->  u = f Px'/Pz', v = -f Py'/Pz'
    K4 = np.array([f[0], -f[0], 0.0, 0.0])
    return BAProblem(cams, prob.pts.copy(), prob.cam_idx.copy(), prob.pt_idx.copy(), prob.uv.copy(), K4, 0).validate()


def from_pinhole(prob: BAProblem) -> BALProblem:
    """A problem in the reference's camera model written as a BAL problem: needs |fy| = fx (BAL has one focal length);
    the principal point is taken out of the pixels (BAL's origin is the image centre) and, for fy = +fx, the y axis is
    turned over (BAL's camera looks down -z: v_bal = -(v - cy)).  Inverse of ``to_pinhole`` when K4 = (f, -f, 0, 0)."""
    from .rotations import matrices_to_rvecs, rvecs_to_matrices
    fx, fy, cx, cy = (float(v) for v in prob.K4)
    if abs(fy) != fx:
        raise ValueError("only |fy| = fx maps onto the BAL camera (one focal length)")
    S = np.diag([1.0, -1.0, -1.0])
    R = S @ rvecs_to_matrices(prob.cams[:, :3])
    t = prob.cams[:, 3:6] @ S.T
    cams = np.concatenate([matrices_to_rvecs(R), t, np.tile([fx, 0.0, 0.0], (prob.n_cams, 1))], axis=1)
    uv = prob.uv - np.array([cx, cy])
    if fy > 0:
        uv = uv * np.array([1.0, -1.0])
    return BALProblem(cams, prob.pts.copy(), prob.cam_idx.copy(), prob.pt_idx.copy(), uv).validate()


def _shared_start(prob, labels, shared_init):
    """prob with every group's (f, k1, k2) set to ONE value: the members' median (shared_init 'median'), or the members'
    own when they already agree ('given': raises ValueError when they do not)."""
    if shared_init not in ("median", "given"):
        raise ValueError(f"shared_init must be 'median' or 'given', not {shared_init!r}")
    cams = prob.cams.copy()
    for g in np.unique(labels[labels >= 0]):
        m = np.nonzero(labels == g)[0]
        if shared_init == "given":
            if (cams[m, 6:9] != cams[m[0], 6:9]).any():
                bad = m[(cams[m, 6:9] != cams[m[0], 6:9]).any(axis=1)][0]
                raise ValueError(f"shared_init='given': camera {int(bad)} of group {int(g)} does not start with the f, k1, k2 of camera {int(m[0])}")
        else:
            cams[m, 6:9] = np.median(cams[m, 6:9], axis=0)
    return BALProblem(cams, prob.pts, prob.cam_idx, prob.pt_idx, prob.uv)


def _bal_priors(prob, camera_priors, intrinsics_sigma, labels=None):
    """camera_priors plus the calibration regulariser: a prior on f, k1, k2 of every camera at their input values with
    standard deviations intrinsics_sigma = (s_f, s_k1, s_k2), added to the 9 x 9 blocks of camera_priors.  labels (shared
    intrinsics): a group carries the regulariser once, on its leader (the member with the lowest index)."""
    if intrinsics_sigma is None:
        return camera_priors
    from .priors import camera_prior_nb, info_from_sigma, pack_priors
    nc = prob.n_cams
    mean = np.zeros((nc, 9))
    info = np.zeros((nc, 9, 9))
    if camera_priors is not None:
        nb = camera_prior_nb(camera_priors) or 6
        m, packed = pack_priors(camera_priors, nc, nb, "camera")
        iu = np.triu_indices(nb)
        full = np.zeros((nc, nb, nb))
        full[:, iu[0], iu[1]] = packed
        full[:, iu[1], iu[0]] = packed
        if nb == 9 and full[:, 6:, :].any():
            raise ValueError("intrinsics_sigma and camera_priors both set information on f, k1, k2")
        mean[:, :nb] = m
        info[:, :nb, :nb] = full
    mean[:, 6:] = prob.cams[:, 6:9]
    info[:, 6:, 6:] = info_from_sigma(np.asarray(intrinsics_sigma, dtype=np.float64).reshape(3))
    if labels is not None:
        for g in np.unique(labels[labels >= 0]):
            m = np.nonzero(labels == g)[0]
            info[m[1:], 6:, 6:] = 0.0
    return mean, info


def solve(prob: BALProblem, device=0, fixed_cam=-1, hold_intrinsics=False, held_cameras=None, held_points=None,
          camera_priors=None, point_priors=None, intrinsics_sigma=None, shared_intrinsics=None, shared_init="median",
          **options):
    """Adjust a BAL problem on the GPU (``ba_solve_bal``: poses, points AND f / k1 / k2 per camera).  Returns
    ``(BALProblem with the adjusted parameters, summary dict)``; options as ``hip_backend.Solver.solve``.
    hold_intrinsics: keep every camera's f, k1, k2 (calibrated cameras); held_cameras / held_points: parameters kept
    constant, in the forms of ``hip_backend.Solver.set_held`` (a (Nc, 9) bool array names single BAL parameters).
    camera_priors / point_priors: Gaussian priors in the forms of ``hip_backend.Solver.set_priors`` (camera blocks of 6 or
    9 coordinates); intrinsics_sigma = (s_f, s_k1, s_k2): the calibration regulariser, a prior on f, k1, k2 of every
    camera at their input values -- the soft form of hold_intrinsics.  With priors ``final_cost`` is the total objective.
    shared_intrinsics: cameras that share ONE f, k1, k2 (``hip_backend.camera_groups`` forms: True = all cameras, a label
    array, a list of index lists) -- self-calibration of a few physical cameras.  shared_init: 'median' starts every group
    from its members' median, 'given' requires equal members.  A grouped ``fixed_cam`` has its POSE held (the group's
    intrinsics stay free); intrinsics_sigma then acts once per group.  The members come back bit-equal."""
    from . import hip_backend
    labels = hip_backend.camera_groups(shared_intrinsics, prob.n_cams)
    if labels is not None:
        prob = _shared_start(prob, labels, shared_init)
        if fixed_cam >= 0 and labels[fixed_cam] >= 0 and np.count_nonzero(labels == labels[fixed_cam]) > 1:
            cm = hip_backend.held_camera_mask(held_cameras, prob.n_cams, 9)
            cm = np.zeros(prob.n_cams, np.uint16) if cm is None else cm.copy()
            cm[fixed_cam] |= np.uint16(0x3F)
            held_cameras, fixed_cam = cm, -1
    with hip_backend.Solver(device) as s:
        summary, cams, pts = s.solve_bal(prob, fixed_cam=fixed_cam, hold_intrinsics=hold_intrinsics,
                                         held_cameras=held_cameras, held_points=held_points,
                                         camera_priors=_bal_priors(prob, camera_priors, intrinsics_sigma, labels),
                                         point_priors=point_priors, shared_intrinsics=labels, **options)
    return BALProblem(cams, pts, prob.cam_idx.copy(), prob.pt_idx.copy(), prob.uv.copy()), summary


def covariance(prob: BALProblem, device=0, fixed_cam=-1, hold_intrinsics=False, held_cameras=None, held_points=None,
               loss="linear", f_scale=1.0, full=False, rcond=0.0, camera_priors=None, point_priors=None, intrinsics_sigma=None,
               shared_intrinsics=None):
    """Marginal covariances of a BAL problem at ``prob``'s parameters (``ba_covariance``; normally the problem ``solve``
    returned).  The held-parameter forms are those of ``solve``; a BAL problem with nothing held has a free 7-dof gauge
    and is refused (hold e.g. ``fixed_cam`` and one translation coordinate of another camera) unless priors
    (camera_priors / point_priors / intrinsics_sigma, as in ``solve``) fix it: Sigma = (H + L)^-1.  Returns
    ``dict(cams (Nc, 9, 9), points (Np, 3, 3), full (9 Nc, 9 Nc) or None)``, see ``hip_backend.Solver.covariance``.
    Covariances of shared intrinsics are not offered: shared_intrinsics that name a group raise ValueError."""
    from . import hip_backend
    labels = hip_backend.camera_groups(shared_intrinsics, prob.n_cams)
    if labels is not None and (np.bincount(labels[labels >= 0]) > 1).any():
        raise ValueError("bal.covariance: covariances of shared intrinsics are not offered")
    with hip_backend.Solver(device) as s:
        intr = s._set_bal(prob, fixed_cam)
        cm = hip_backend.held_camera_mask(held_cameras, s.n_cams, 9)
        if hold_intrinsics:
            cm = (np.zeros(s.n_cams, np.uint16) if cm is None else cm) | np.uint16(0x1C0)
        if cm is not None or held_points is not None:
            s.set_held(cm, held_points)
        cp = _bal_priors(prob, camera_priors, intrinsics_sigma)
        if cp is not None or point_priors is not None:
            s.set_priors(cp, point_priors)
        return s.covariance(loss=loss, f_scale=f_scale, intr=intr, full=full, rcond=rcond)


def triangulate(prob: BALProblem, device=0, write=False, **opts):
    """Triangulate every point of a BAL problem from all of its observations and ``prob``'s cameras, f / k1 / k2 included
    (``ba_triangulate_tracks``; opts as ``hip_backend.Solver.triangulate_tracks``: loss, refine_iters, f_scale,
    min_angle_deg, max_reproj_px, min_depth).  Returns dict(xyz, status, angle_deg, rms_px, max_px) in ``prob``'s point order;
    with ``write=True`` also a copy of ``prob`` whose OK points carry the triangulated positions -- what
    ``triangulation.filter_tracks`` and the next ``solve`` take."""
    from . import hip_backend
    with hip_backend.Solver(device) as s:
        intr = s._set_bal(prob)
        out = s.triangulate_tracks(intr=intr, write_points=int(bool(write)), **opts)
        pts = s.get_params()[1] if write else None
    if not write:
        return out
    return out, BALProblem(prob.cams.copy(), pts, prob.cam_idx.copy(), prob.pt_idx.copy(), prob.uv.copy())


def resect(prob: BALProblem, device=0, write=True, cams=None, known_points=None, **opts):
    """Resect the cameras of a BAL problem from ``prob.pts``, taken as known, with each camera's own f / k1 / k2
    (``ba_resect``; cams, known_points and opts as ``hip_backend.Solver.resect``).  Returns ``(out, problem)``:
    dict(poses, status, n_inliers, rms_px, max_px) and a copy of ``prob`` with the merged cameras (``write=True``: the
    selected cameras that are OK carry their resected poses; f, k1, k2 are left alone)."""
    from . import hip_backend
    with hip_backend.Solver(device) as s:
        intr = s._set_bal(prob)
        out = s.resect(intr=intr, cams=cams, known_points=known_points, write_cams=int(bool(write)), **opts)
        cams6 = s.get_params()[0]
    return out, BALProblem(np.concatenate([cams6, intr], axis=1), prob.pts.copy(), prob.cam_idx.copy(), prob.pt_idx.copy(), prob.uv.copy())


def resect_ransac(prob: BALProblem, device=0, write=True, cams=None, known_points=None, **opts):
    """Resect the cameras of a BAL problem from raw matches (``ba_resect_ransac``; cams, known_points and opts as
    ``hip_backend.Solver.resect_ransac``).  Returns ``(out, problem)`` like ``resect``; ``out["obs_inlier"]`` is the consensus
    set in ``prob``'s observation order, what ``triangulation.filter_observations`` takes."""
    from . import hip_backend
    with hip_backend.Solver(device) as s:
        intr = s._set_bal(prob)
        out = s.resect_ransac(intr=intr, cams=cams, known_points=known_points, write_cams=int(bool(write)), **opts)
        cams6 = s.get_params()[0]
    return out, BALProblem(np.concatenate([cams6, intr], axis=1), prob.pts.copy(), prob.cam_idx.copy(), prob.pt_idx.copy(), prob.uv.copy())


def align(prob: BALProblem, cam_ref=None, pt_ref=None, cam_w=None, pt_w=None, loss="linear", f_scale=1.0, iters=10,
          with_scale=True, device=0):
    """Align a BAL problem to reference positions: the similarity ``X' = s R X + t`` that brings its camera centres
    (cam_ref (Nc, 3)) and / or points (pt_ref (Np, 3)) onto them, weighted and robust (``ba_align`` with apply = 1;
    arguments as ``hip_backend.Solver.align``).  Returns ``(result dict, transformed BALProblem)``; f, k1, k2 are left
    alone and every residual stays where it was.  When the status is not OK the problem comes back unchanged."""
    from . import hip_backend
    with hip_backend.Solver(device) as s:
        intr = s._set_bal(prob)
        res = s.align(cam_ref=cam_ref, pt_ref=pt_ref, cam_w=cam_w, pt_w=pt_w, loss=loss, f_scale=f_scale, iters=iters,
                      with_scale=with_scale, apply=True)
        cams6, pts = s.get_params()
    return res, BALProblem(np.concatenate([cams6, intr], axis=1), pts, prob.cam_idx.copy(), prob.pt_idx.copy(), prob.uv.copy())
