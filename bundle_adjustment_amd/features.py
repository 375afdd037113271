"""Descriptor matching -- the step that produces the matches everything downstream starts from.

Mirrors ``BruteForceMatcher.match`` of ``src/features.py`` (``cv2.BFMatcher(NORM_HAMMING, crossCheck=False).knnMatch(des1, des2,
k=2)`` then Lowe's ``m.distance < 0.75 * n.distance``) on the GPU (``ba_match_descriptors``: brute-force Hamming 2-nearest
neighbours, ties to the lower train index, the ratio test in fp64).  The match objects are duck-typed for
``pose_estimator.estimate_pose``, which reads ``queryIdx`` / ``trainIdx``.  No cv2 is needed; ORB extraction is not offered.
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


def match_to_keyframes(des_new, keyframe_descriptors, solver=None, **opts):
    """The exhaustive loop of ``pipeline.py:133-134`` in ONE call: every keyframe's descriptors are a query set against the new
    frame's (the argument order ``match(kf.descriptors, des_new)`` there), the new frame's set is uploaded once.  Returns one
    list of ``Match`` per keyframe, in query order; a keyframe without descriptors (``None``) gets ``[]``, and so does
    every keyframe when ``des_new`` is ``None``."""
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
        out = s.match_descriptors(sets, pairs, **opts)
    finally:
        if own:
            s.close()
    lists = [[] for _ in kfs]
    for n, k in enumerate(have):
        lists[k] = _match_list(*_good_of_pair(out, n))
    return lists


class BruteForceMatcher:
    """Drop-in for the reference's ``BruteForceMatcher`` (Hamming norm): ``match(des1, des2)`` -> the good matches, a list in
    query order of objects with ``queryIdx``, ``trainIdx``, ``imgIdx = 0`` and ``distance`` (float).  ``None`` for either
    argument returns ``[]`` as there, and so does a train set of fewer than two descriptors (there ``for m, n in matches``
    raises and the ``except`` returns the empty list)."""

    def __init__(self, ratio=0.75, solver=None):
        self.ratio, self.solver = ratio, solver

    def match(self, des1, des2):
        if des1 is None or des2 is None:
            return []
        return _match_list(*match(des1, des2, solver=self.solver, ratio=self.ratio))
