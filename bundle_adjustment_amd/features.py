"""Feature extraction and descriptor matching -- the steps that produce the keypoints and matches everything downstream starts
from.

``ORBExtractor.extract`` stands where ``ORBExtractor.extract`` of ``src/features.py`` does (``cv2.ORB_create(nfeatures=3000)
.detectAndCompute(gray, None)``) and runs on the GPU (``ba_orb_extract``): ORB by the published algorithm -- multi-scale FAST-9,
Harris ranking, intensity-centroid orientation, steered BRIEF on a blurred pyramid.  It is NOT cv2's output: neither the
keypoints nor the descriptors are claimed equal to cv2's, and the default test pattern is not OpenCV's learned one (pass that
table as ``pattern`` if you have it); descriptors match only descriptors made with the same pattern.

The matcher mirrors ``BruteForceMatcher.match`` of ``src/features.py`` (``cv2.BFMatcher(NORM_HAMMING, crossCheck=False).knnMatch(des1, des2,
k=2)`` then Lowe's ``m.distance < 0.75 * n.distance``) on the GPU (``ba_match_descriptors``: brute-force Hamming 2-nearest
neighbours, ties to the lower train index, the ratio test in fp64).  The match objects are duck-typed for
``pose_estimator.estimate_pose``, which reads ``queryIdx`` / ``trainIdx``.  No cv2 is needed.
``match_l2`` and ``BruteForceMatcher(norm="l2")`` match uint8 descriptors under the Euclidean distance (``ba_match_l2``: SIFT /
RootSIFT as COLMAP stores them, 128 uint8 per keypoint; ``quantize_descriptors`` takes float descriptors there).
Once geometry is known, ``match_epipolar`` and ``match_by_projection`` match a second time under it (``ba_match_guided``: the
same 2-NN over the keypoints an epipolar line or a search window admits; no counterpart in the reference).
``track``, ``calc_optical_flow_pyr_lk`` (the shapes of ``cv2.calcOpticalFlowPyrLK``) and ``refine_matches`` follow known points
from one image into another by pyramidal Lucas-Kanade (``ba_track_klt``): the per-frame step between keyframes, and the
sub-pixel refinement of an ORB match.  Lucas-Kanade by the library's definition, not cv2's numbers.
No CPU fallback: without the library / a GPU the call raises.
"""
from __future__ import annotations

import numpy as np

from . import hip_backend


class Match:
    """What ``estimate_pose`` and the reference's pipeline read of a ``cv2.DMatch``."""
    __slots__ = ("queryIdx", "trainIdx", "imgIdx", "distance")

    def __init__(self, queryIdx, trainIdx, distance):
        self.queryIdx, self.trainIdx, self.imgIdx, self.distance = int(queryIdx), int(trainIdx), 0, float(distance)

    def __repr__(self):
        return f"Match(queryIdx={self.queryIdx}, trainIdx={self.trainIdx}, distance={self.distance})"


def _descriptors(des):
    a = np.asarray(des)
    if a.dtype != np.uint8 or a.ndim != 2:
        raise ValueError(f"descriptors must be a 2-D uint8 array, not {a.dtype} with shape {a.shape}")
    return a


def _good_of_pair(out, p):
    """(query_idx, train_idx, distance) of the good rows of pair p, in query order."""
    lo, hi = int(out["row_off"][p]), int(out["row_off"][p + 1])
    q = np.nonzero(out["good"][lo:hi])[0]
    return q, out["best"][lo:hi][q].astype(np.int64), out["dist1"][lo:hi][q].astype(np.int64)


def _match_list(q, t, d):
    return [Match(a, b, c) for a, b, c in zip(q.tolist(), t.tolist(), d.tolist())]


def match(des1, des2, solver=None, **opts):
    """-> (query_idx, train_idx, distance) int64 arrays of the good matches of des1 (queries) against des2, in query order.
    opts: ratio (default 0.75), max_distance, mutual (``hip_backend.Solver.match_descriptors``).  ``solver``: a
    ``hip_backend.Solver`` to run on (its resident problem is not touched); default: one on device 0 for the call."""
    own = solver is None
    s = hip_backend.Solver(0) if own else solver
    try:
        out = s.match_descriptors([_descriptors(des1), _descriptors(des2)], **opts)
    finally:
        if own:
            s.close()
    return _good_of_pair(out, 0)


def match_l2(des1, des2, solver=None, **opts):
    """``match`` for uint8 descriptors under the Euclidean distance (``hip_backend.Solver.match_l2``; width a multiple of 32 in
    32 .. 256) -> (query_idx, train_idx, sqdist) int64 arrays of the good matches in query order; sqdist is the SQUARED
    distance, and so is the unit of ``max_distance``.  opts: ratio (default 0.75, Lowe's test on the distances), max_distance,
    mutual."""
    own = solver is None
    s = hip_backend.Solver(0) if own else solver
    try:
        out = s.match_l2([_descriptors(des1), _descriptors(des2)], **opts)
    finally:
        if own:
            s.close()
    return _good_of_pair(out, 0)


def quantize_descriptors(x, root=False):
    """Float descriptors (n, D) -> uint8 the way COLMAP stores SIFT: with ``root`` (RootSIFT) every row is L1-normalised and
    its square root taken; then every row is L2-normalised and stored as min(255, floor(512 x + 0.5)).  All-zero rows stay
    zero.  Computed in float64 on the host.  This follows COLMAP's published steps; equality with COLMAP's bytes (float32
    arithmetic there) is NOT verified."""
    a = np.asarray(x, dtype=np.float64)
    if a.ndim != 2:
        raise ValueError(f"descriptors must be a 2-D array, not shape {a.shape}")
    if root:
        l1 = np.abs(a).sum(axis=1, keepdims=True)
        a = np.sqrt(np.abs(a) / np.where(l1 > 0, l1, 1.0))
    l2 = np.sqrt((a * a).sum(axis=1, keepdims=True))
    a = a / np.where(l2 > 0, l2, 1.0)
    return np.minimum(255.0, np.floor(512.0 * a + 0.5)).clip(0.0, 255.0).astype(np.uint8)


def match_to_keyframes(des_new, keyframe_descriptors, solver=None, norm="hamming", **opts):
    """The exhaustive loop of ``pipeline.py:133-134`` in ONE call: every keyframe's descriptors are a query set against the new
    frame's (the argument order ``match(kf.descriptors, des_new)`` there), the new frame's set is uploaded once.  Returns one
    list of ``Match`` per keyframe, in query order; a keyframe without descriptors (``None``) gets ``[]``, and so does
    every keyframe when ``des_new`` is ``None``.  ``norm``: "hamming" (binary descriptors, the default) or "l2" (uint8 descriptors
    through ``ba_match_l2``; ``Match.distance`` is then the Euclidean distance, the square root of ``dist1``)."""
    if norm not in ("hamming", "l2"):
        raise ValueError(f"norm must be 'hamming' or 'l2', not {norm!r}")
    kfs = list(keyframe_descriptors)
    if des_new is None or not kfs:
        return [[] for _ in kfs]
    have = [k for k, d in enumerate(kfs) if d is not None]
    if not have:
        return [[] for _ in kfs]
    sets = [_descriptors(des_new)] + [_descriptors(kfs[k]) for k in have]
    pairs = np.array([(1 + n, 0) for n in range(len(have))], dtype=np.int32)
    own = solver is None
    s = hip_backend.Solver(0) if own else solver
    try:
        out = (s.match_l2 if norm == "l2" else s.match_descriptors)(sets, pairs, **opts)
    finally:
        if own:
            s.close()
    lists = [[] for _ in kfs]
    for n, k in enumerate(have):
        q, t, d = _good_of_pair(out, n)
        lists[k] = _match_list(q, t, np.sqrt(d.astype(np.float64)) if norm == "l2" else d)
    return lists


def fundamental(K, R, t):
    """F = K^-T [t]x R K^-1 of x2 ~ K (R x1 + t), the convention of ``ba_relative_pose``: x2^T F x1 = 0 in pixels."""
    K, R, t = np.asarray(K, dtype=np.float64).reshape(3, 3), np.asarray(R, dtype=np.float64).reshape(3, 3), np.asarray(t, dtype=np.float64).reshape(3)
    tx = np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])
    Ki = np.linalg.inv(K)
    return Ki.T @ tx @ R @ Ki


def _positions(kp):
    """(n, 2) float64 pixel positions of an (n, 2) array or of a sequence of objects with ``.pt``; None -> None."""
    if kp is None:
        return None
    if isinstance(kp, np.ndarray):
        return np.asarray(kp, dtype=np.float64).reshape(-1, 2)
    kp = list(kp)
    if kp and hasattr(kp[0], "pt"):
        return np.array([k.pt for k in kp], dtype=np.float64).reshape(-1, 2)
    return np.asarray(kp, dtype=np.float64).reshape(-1, 2)


def _empty_matches():
    z = np.zeros(0, dtype=np.int64)
    return z, z.copy(), z.copy()


def _guided(solver, sets, kps, **kw):
    own = solver is None
    s = hip_backend.Solver(0) if own else solver
    try:
        return s.match_guided(sets, kps, **kw)
    finally:
        if own:
            s.close()


def match_epipolar(des1, kp1, des2, kp2, K, R, t, max_epi_px=3.0, solver=None, **opts):
    """The matches of des1 (queries, keypoints kp1) against des2 (kp2) that the pose explains: a train keypoint is a candidate
    of a query only within ``max_epi_px`` of the query's epipolar line under x2 ~ K (R x1 + t) (``ba_match_guided``, epipolar
    gate).  -> (query_idx, train_idx, distance) int64 arrays in query order.  ``kp*``: (n, 2) arrays or sequences of objects
    with ``.pt``.  opts: ratio, max_distance, mutual, single.  ``None`` or empty descriptors on either side return no match."""
    if des1 is None or des2 is None or len(des1) == 0 or len(des2) == 0:
        return _empty_matches()
    out = _guided(solver, [_descriptors(des1), _descriptors(des2)], [_positions(kp1), _positions(kp2)],
                  fundamental=fundamental(K, R, t)[None], max_epi_px=max_epi_px, **opts)
    return _good_of_pair(out, 0)


def match_by_fundamental(des1, kp1, des2, kp2, F, max_epi_px=3.0, solver=None, **opts):
    """``match_epipolar`` with a given fundamental matrix (pixels, p2^T F p1 = 0: ``ba_fundamental``'s ``F``) in place of K, R, t:
    the guided second pass of an uncalibrated pair.  -> (query_idx, train_idx, distance) int64 arrays in query order.  opts:
    ratio, max_distance, mutual, single.  ``None`` or empty descriptors on either side return no match."""
    if des1 is None or des2 is None or len(des1) == 0 or len(des2) == 0:
        return _empty_matches()
    out = _guided(solver, [_descriptors(des1), _descriptors(des2)], [_positions(kp1), _positions(kp2)],
                  fundamental=np.asarray(F, dtype=np.float64).reshape(1, 3, 3), max_epi_px=max_epi_px, **opts)
    return _good_of_pair(out, 0)


def match_by_projection(K, R, t, points, point_desc, kp, des, radius_px, image_size=None, solver=None, **opts):
    """Map points matched into an image by projection under a predicted pose (ORB-SLAM's ``SearchByProjection``): point n with
    descriptor ``point_desc[n]`` is projected on the host, x ~ K (R X + t), and only the keypoints within ``radius_px`` (a scalar or
    one per point) of the projection are its candidates (``ba_match_guided``, window gate).  A point with z <= 0, with a
    projection that is not finite or, given ``image_size = (width, height)``, outside 0 <= x < width, 0 <= y < height gets radius
    -1: no candidate.  -> (point_idx, kp_idx, distance) int64 arrays in point order: the 3D-2D observations ``ba_resect_ransac``
    takes.  opts: ratio, max_distance, mutual, single.  ``None`` or empty inputs on either side return no match."""
    if points is None or point_desc is None or des is None or len(point_desc) == 0 or len(des) == 0:
        return _empty_matches()
    X = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    pd = _descriptors(point_desc)
    if len(X) != len(pd):
        raise ValueError(f"{len(X)} points for {len(pd)} point descriptors")
    Xc = X @ np.asarray(R, dtype=np.float64).reshape(3, 3).T + np.asarray(t, dtype=np.float64).reshape(3)
    x = Xc @ np.asarray(K, dtype=np.float64).reshape(3, 3).T
    front = Xc[:, 2] > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        uv = x[:, :2] / x[:, 2:3]
    ok = front & np.isfinite(uv).all(axis=1)
    if image_size is not None:
        ok &= (uv[:, 0] >= 0) & (uv[:, 0] < image_size[0]) & (uv[:, 1] >= 0) & (uv[:, 1] < image_size[1])
    window = np.zeros((len(X), 3), dtype=np.float32)
    window[:, :2] = np.where(ok[:, None], uv, 0.0)
    window[:, 2] = np.where(ok, np.broadcast_to(np.asarray(radius_px, dtype=np.float64), (len(X),)), -1.0)
    kps = _positions(kp)
    out = _guided(solver, [pd, _descriptors(des)], [np.zeros((len(X), 2), dtype=np.float32), kps], window=window, **opts)
    return _good_of_pair(out, 0)


def match_by_homography(des1, kp1, des2, kp2, H, radius_px, solver=None, **opts):
    """Matches of a planar scene under a known homography (pixels, p2 ~ H p1: ``ba_homography``'s ``H``): keypoint i of the
    first image is predicted at pi(H kp1[i]) on the host, and only the keypoints of the second image within ``radius_px`` (a
    scalar or one per keypoint) of the prediction are its candidates (``ba_match_guided``, window gate).  A keypoint whose
    prediction has a non-positive third component or is not finite gets radius -1: no candidate.  -> (idx1, idx2, distance) int64
    arrays in the order of the first image.  opts: ratio, max_distance, mutual, single.  ``None`` or empty inputs on either side
    return no match."""
    if des1 is None or des2 is None or len(des1) == 0 or len(des2) == 0:
        return _empty_matches()
    k1 = _positions(kp1)
    y = np.c_[np.asarray(k1, dtype=np.float64), np.ones(len(k1))] @ np.asarray(H, dtype=np.float64).reshape(3, 3).T
    with np.errstate(divide="ignore", invalid="ignore"):
        uv = y[:, :2] / y[:, 2:3]
    ok = (y[:, 2] > 0) & np.isfinite(uv).all(axis=1)
    window = np.zeros((len(k1), 3), dtype=np.float32)
    window[:, :2] = np.where(ok[:, None], uv, 0.0)
    window[:, 2] = np.where(ok, np.broadcast_to(np.asarray(radius_px, dtype=np.float64), (len(k1),)), -1.0)
    out = _guided(solver, [_descriptors(des1), _descriptors(des2)], [k1, _positions(kp2)], window=window, **opts)
    return _good_of_pair(out, 0)


class BruteForceMatcher:
    """Drop-in for the reference's ``BruteForceMatcher`` (Hamming norm): ``match(des1, des2)`` -> the good matches, a list in
    query order of objects with ``queryIdx``, ``trainIdx``, ``imgIdx = 0`` and ``distance`` (float).  ``None`` for either
    argument returns ``[]`` as there, and so does a train set of fewer than two descriptors (there ``for m, n in matches``
    raises and the ``except`` returns the empty list).  ``norm="l2"``: uint8 descriptors under the Euclidean distance
    (``match_l2``), ``distance`` the square root of the squared distance as a float, cv2's ``NORM_L2`` convention."""

    def __init__(self, ratio=0.75, solver=None, norm="hamming"):
        if norm not in ("hamming", "l2"):
            raise ValueError(f"norm must be 'hamming' or 'l2', not {norm!r}")
        self.ratio, self.solver, self.norm = ratio, solver, norm

    def match(self, des1, des2):
        if des1 is None or des2 is None:
            return []
        if self.norm == "l2":
            q, t, d = match_l2(des1, des2, solver=self.solver, ratio=self.ratio)
            return _match_list(q, t, np.sqrt(d.astype(np.float64)))
        return _match_list(*match(des1, des2, solver=self.solver, ratio=self.ratio))


class KeyPoint:
    """What the pipeline reads of a ``cv2.KeyPoint``: ``pt`` (x, y) in pixels of the full image, ``size`` (patch diameter),
    ``angle`` (degrees in [0, 360)), ``response`` (Harris), ``octave`` (pyramid level), ``class_id`` (-1)."""
    __slots__ = ("pt", "size", "angle", "response", "octave", "class_id")

    def __init__(self, x, y, size, angle=-1.0, response=0.0, octave=0, class_id=-1):
        self.pt, self.size, self.angle = (float(x), float(y)), float(size), float(angle)
        self.response, self.octave, self.class_id = float(response), int(octave), int(class_id)

    def __repr__(self):
        return f"KeyPoint(pt={self.pt}, size={self.size}, angle={self.angle}, response={self.response}, octave={self.octave})"


def to_gray(bgr):
    """(H, W, 3) uint8 BGR -> (H, W) uint8 grey, the 14-bit fixed-point weights of ``cv2.cvtColor(..., COLOR_BGR2GRAY)``:
    (1868 B + 9617 G + 4899 R + 8192) >> 14.  Numpy on the host; a 2-D array is returned as it is."""
    a = np.asarray(bgr)
    if a.dtype != np.uint8:
        raise ValueError(f"the image must be uint8, not {a.dtype}")
    if a.ndim == 2:
        return a
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"the image must be (H, W) or (H, W, 3), not {a.shape}")
    c = a.astype(np.uint32)
    return ((1868 * c[..., 0] + 9617 * c[..., 1] + 4899 * c[..., 2] + 8192) >> 14).astype(np.uint8)


def extract(images, solver=None, pattern=None, **opts):
    """``hip_backend.Solver.extract_orb`` of one grey image (H, W) or a batch (n, H, W) of one size -> its dict of arrays
    (kp_off, n_kp, xy, size, angle, response, octave, level_xy, cs, desc).  opts: n_features, scale_factor, n_levels,
    edge_threshold, fast_threshold.  ``solver``: a ``hip_backend.Solver`` to run on (its resident problem is not touched);
    default: one on device 0 for the call."""
    own = solver is None
    s = hip_backend.Solver(0) if own else solver
    try:
        return s.extract_orb(images, pattern=pattern, **opts)
    finally:
        if own:
            s.close()


def _track_pair(img1, img2, pts, guess, solver, opts):
    """``hip_backend.Solver.track_klt`` of one image pair (colour images through ``to_gray``) -> its dict."""
    a, b = to_gray(img1), to_gray(img2)
    if a.shape != b.shape:
        raise ValueError(f"the two images must have one size, not {a.shape} and {b.shape}")
    p = np.asarray(pts, dtype=np.float32).reshape(-1, 2)
    g = None if guess is None else [np.asarray(guess, dtype=np.float32).reshape(-1, 2)]
    own = solver is None
    s = hip_backend.Solver(0) if own else solver
    try:
        return s.track_klt(np.stack([a, b]), [(0, 1)], [p], guess=g, **opts)
    finally:
        if own:
            s.close()


def track(img1, img2, pts, guess=None, solver=None, **opts):
    """Follows the points ``pts`` (n, 2), pixels of ``img1``, into ``img2`` by pyramidal Lucas-Kanade (``ba_track_klt``) ->
    (next (n, 2) float32, ok (n,) bool, err (n,) float32): ok where the status is OK, err the mean absolute intensity difference
    of the window there (NaN elsewhere).  ``guess``: the starts in ``img2`` (default: ``pts``).  opts: half_window, max_level,
    max_iters, eps, min_eig, fb_max_px (> 0: forward-backward check).  Lucas-Kanade by the library's definition, not cv2's
    output.  ``solver``: a ``hip_backend.Solver`` to run on (its resident problem is not touched); default: one on device 0."""
    out = _track_pair(img1, img2, pts, guess, solver, opts)
    return out["next"], out["status"] == hip_backend.KLT_STATUS["ok"], out["err"]


def calc_optical_flow_pyr_lk(prev_img, next_img, prev_pts, next_pts=None, win_size=(21, 21), max_level=3, criteria=(30, 0.01),
                             min_eig_threshold=1e-4, solver=None):
    """Drop-in with the shapes of ``cv2.calcOpticalFlowPyrLK``: ``prev_pts`` (n, 1, 2) (or (n, 2)) float32, ``next_pts`` the
    initial guesses or None -> (next_pts (n, 1, 2) float32, status (n, 1) uint8 with 1 = found, err (n, 1) float32).
    ``criteria`` = (max iterations, epsilon).  A square window of odd size only; any other raises ValueError.  Not cv2's numbers
    (``track``)."""
    if len(win_size) != 2 or win_size[0] != win_size[1] or int(win_size[0]) != win_size[0] or int(win_size[0]) % 2 != 1:
        raise ValueError(f"win_size must be square and odd, not {tuple(win_size)}")
    out = _track_pair(prev_img, next_img, prev_pts, next_pts, solver,
                      dict(half_window=(int(win_size[0]) - 1) // 2, max_level=int(max_level), max_iters=int(criteria[0]), eps=float(criteria[1]),
                           min_eig=float(min_eig_threshold)))
    n = len(out["status"])
    found = (out["status"] == hip_backend.KLT_STATUS["ok"]).astype(np.uint8)
    return out["next"].reshape(n, 1, 2), found.reshape(n, 1), out["err"].reshape(n, 1)


def refine_matches(img1, kp1, img2, kp2, q, t, max_shift_px=2.0, solver=None, **opts):
    """Subpixel positions for the matches (q[k], t[k]) of keypoints ``kp1`` of ``img1`` and ``kp2`` of ``img2``: ``kp1[q]`` is tracked
    into ``img2`` from ``kp2[t]`` (``ba_track_klt`` with ``guess``) -> (xy2 (m, 2) float32, keep (m,) bool).  A match is kept when the
    status is OK and the refined point lies within ``max_shift_px`` of ``kp2[t]``; xy2 of a match that is not kept is ``kp2[t]``.
    ``kp*``: (n, 2) arrays or sequences of objects with ``.pt``.  xy2[keep] is the ``uv`` of the second image for ``to_problem`` /
    ``ba_set_problem``."""
    k1, k2 = _positions(kp1), _positions(kp2)
    q, t = np.asarray(q, dtype=np.int64).reshape(-1), np.asarray(t, dtype=np.int64).reshape(-1)
    if len(q) != len(t):
        raise ValueError("q and t must list the same number of matches")
    start = k2[t].astype(np.float32)
    out = _track_pair(img1, img2, k1[q], start, solver, opts)
    moved = np.hypot(*(out["next"].astype(np.float64) - start.astype(np.float64)).T)
    with np.errstate(invalid="ignore"):
        keep = (out["status"] == hip_backend.KLT_STATUS["ok"]) & (moved <= max_shift_px)
    return np.where(keep[:, None], out["next"], start), keep


class ORBExtractor:
    """Drop-in for the reference's ``ORBExtractor``: ``extract(image)`` -> (list of ``KeyPoint``, uint8 (n, 32) descriptors), or
    ``([], None)`` when the image has no keypoint.  A colour image (H, W, 3) is taken as BGR (``to_gray``).  ORB by the published
    algorithm on the GPU, not cv2's keypoints or pattern (the module docstring)."""

    def __init__(self, n_features=3000, solver=None, pattern=None, **opts):
        self.n_features, self.solver, self.pattern, self.opts = n_features, solver, pattern, opts

    def extract(self, image):
        out = extract(to_gray(image), solver=self.solver, pattern=self.pattern, n_features=self.n_features, **self.opts)
        n = int(out["n_kp"][0])
        if n == 0:
            return [], None
        kps = [KeyPoint(x, y, sz, an, rs, oc) for (x, y), sz, an, rs, oc in zip(out["xy"].tolist(), out["size"].tolist(), out["angle"].tolist(),
                                                                                 out["response"].tolist(), out["octave"].tolist())]
        return kps, out["desc"]
