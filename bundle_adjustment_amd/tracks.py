"""Feature tracks from pairwise matches (hip_backend.Solver.build_tracks, ba_build_tracks): which keypoints of which images
are one 3D point -- the step between the verified matches of the image pairs and a problem to triangulate and adjust.

    pairs = place.pair_list(solver, vectors, top_k=20)
    matches = [(i, j, *features.match(desc[i], desc[j], solver=solver)[:2]) for i, j in pairs]       # verified: add a keep array
    tr = build_tracks([len(k) for k in keypoints], matches, solver=solver)
    prob = to_problem(tr, keypoints, cams, K4)                                                       # every point at 0
    out, prob = triangulation.triangulate_tracks(prob, solver=solver, write=True)
    prob, _ = triangulation.filter_tracks(prob, out["status"] == 0)

The reference does this pair by pair with a dict per keyframe (src/pipeline.py, _add_new_keyframe /
_add_new_keyframe_exhaustive: last_kf_obs_lookup / kf_obs_lookup).  Everything here is bookkeeping on the host; the
components, the ordering and the conflict policy are the library's.
"""
from __future__ import annotations

import numpy as np


def build_tracks(n_keypoints, pair_matches, solver=None, **opts):
    """Tracks over the keypoints of ``len(n_keypoints)`` images.  ``n_keypoints``: keypoints per image.  ``pair_matches``: an
    iterable of ``(i, j, idx_i, idx_j)`` or ``(i, j, idx_i, idx_j, keep)`` -- images i and j, the keypoint index arrays
    ``features.match`` and the guided matchers return, and optionally a ``match_inlier`` array (0 removes the match).  opts as
    ``hip_backend.Solver.build_tracks``: min_length, conflict ("drop" / "first"), max_rounds.  Returns that call's dict plus
    ``track_image`` and ``track_kp`` (members,): the image and the keypoint index of every member.  ``solver``: a
    ``hip_backend.Solver`` (no resident problem is read or touched); default: one on device 0 for the call.

    The call is stateless.  The incremental use: a map that already has tracks passes them as ``chain_edges`` next to the new
    image's matches and reads ``node_track`` of each old track's first member to carry its point number over."""
    n_keypoints = np.asarray(n_keypoints, dtype=np.int64).reshape(-1)
    kp_off = np.concatenate([[0], np.cumsum(n_keypoints)]).astype(np.int64)
    ea, eb, ek, masked = [], [], [], False
    for item in pair_matches:
        if len(item) not in (4, 5):
            raise ValueError(f"a pair_matches entry has {len(item)} fields: expected (i, j, idx_i, idx_j) or (i, j, idx_i, idx_j, keep)")
        i, j = int(item[0]), int(item[1])
        if not (0 <= i < n_keypoints.shape[0] and 0 <= j < n_keypoints.shape[0]):
            raise ValueError(f"pair ({i}, {j}) names an image outside 0 .. {n_keypoints.shape[0] - 1}")
        ii = np.asarray(item[2], dtype=np.int64).reshape(-1)
        jj = np.asarray(item[3], dtype=np.int64).reshape(-1)
        if ii.shape != jj.shape:
            raise ValueError(f"pair ({i}, {j}): idx_i and idx_j have {ii.shape[0]} and {jj.shape[0]} entries")
        if ii.size and (ii.min() < 0 or ii.max() >= n_keypoints[i] or jj.min() < 0 or jj.max() >= n_keypoints[j]):
            raise ValueError(f"pair ({i}, {j}): a keypoint index is outside its image's keypoints")
        if len(item) == 5 and item[4] is not None:
            k = np.asarray(item[4]).reshape(-1) != 0
            if k.shape != ii.shape:
                raise ValueError(f"pair ({i}, {j}): keep has {k.shape[0]} entries for {ii.shape[0]} matches")
            masked = True
        else:
            k = np.ones(ii.shape[0], dtype=bool)
        ea.append(kp_off[i] + ii); eb.append(kp_off[j] + jj); ek.append(k)
    cat = (lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dtype=dt))
    edge_a, edge_b = cat(ea, np.int32), cat(eb, np.int32)
    keep = cat(ek, np.uint8) if masked else None
    own = solver is None
    if own:
        from . import hip_backend
        solver = hip_backend.Solver(0)
    try:
        out = dict(solver.build_tracks(n_keypoints, edge_a, edge_b, keep, **opts))
    finally:
        if own:
            solver.close()
    return with_members(out)


def with_members(tracks):
    """``tracks`` (a build_tracks dict) with ``track_image`` and ``track_kp`` derived from ``track_node`` and ``kp_off``."""
    out = dict(tracks)
    kp_off = np.asarray(out["kp_off"], dtype=np.int64)
    node = np.asarray(out["track_node"], dtype=np.int64)
    image = np.searchsorted(kp_off, node, side="right") - 1
    out["track_image"] = image.astype(np.int32)
    out["track_kp"] = (node - kp_off[image]).astype(np.int32)
    return out


def _pixels(keypoints):
    """Per image an (n_i, 2) float32 array from an (n_i, 2) array or a list of KeyPoint-likes (``.pt``)."""
    pix = []
    for kps in keypoints:
        if isinstance(kps, np.ndarray):
            a = kps
        else:
            kps = list(kps)
            a = np.array([k.pt for k in kps]) if kps and hasattr(kps[0], "pt") else np.asarray(kps)
        pix.append(np.asarray(a, dtype=np.float32).reshape(-1, 2))
    return pix


def observations(tracks, keypoints):
    """``(cam_idx int32, pt_idx int32, uv float64 (n, 2))`` of the tracks' members in track order: point t is track t, camera
    i is image i.  ``keypoints``: per image an (n_i, 2) array or a list of ``KeyPoint``.  Pixels are float32 values, as
    cv2's are (so the library keeps its float2 pixel streams)."""
    if "track_image" not in tracks:
        tracks = with_members(tracks)
    pix = _pixels(keypoints)
    kp_off = np.asarray(tracks["kp_off"], dtype=np.int64)
    if len(pix) != kp_off.shape[0] - 1 or any(p.shape[0] != kp_off[i + 1] - kp_off[i] for i, p in enumerate(pix)):
        raise ValueError("keypoints must list every image's keypoints, as many per image as build_tracks was told")
    allpix = np.concatenate(pix) if pix else np.zeros((0, 2), dtype=np.float32)
    track_off = np.asarray(tracks["track_off"], dtype=np.int64)
    pt_idx = np.repeat(np.arange(track_off.shape[0] - 1, dtype=np.int32), np.diff(track_off))
    uv = allpix[np.asarray(tracks["track_node"], dtype=np.int64)].astype(np.float64).reshape(-1, 2)
    return np.asarray(tracks["track_image"], dtype=np.int32).copy(), pt_idx, uv


def to_problem(tracks, keypoints, cams, K4=None):
    """A problem over the tracks with every point at 0: a ``BAProblem`` for ``K4`` and (Nc, 6) cameras, a ``bal.BALProblem``
    for (Nc, 9) cameras.  The caller then runs ``triangulation.triangulate_tracks(prob, write=True)`` (or
    ``bal.triangulate(prob, write=True)``) and ``triangulation.filter_tracks(merged, out["status"] == 0)``: the N-view DLT does
    not read the starting point.  By construction no point has two observations in one camera."""
    cams = np.ascontiguousarray(cams, dtype=np.float64)
    cam_idx, pt_idx, uv = observations(tracks, keypoints)
    n_images = np.asarray(tracks["kp_off"]).shape[0] - 1
    if cams.ndim != 2 or cams.shape[0] != n_images:
        raise ValueError(f"cams must have one row per image ({n_images}), not shape {cams.shape}")
    pts = np.zeros((np.asarray(tracks["track_off"]).shape[0] - 1, 3))
    if cams.shape[1] == 9:
        if K4 is not None:
            raise ValueError("(Nc, 9) cameras carry their own intrinsics: K4 must be None")
        from .bal import BALProblem
        return BALProblem(cams, pts, cam_idx, pt_idx, uv).validate()
    if cams.shape[1] != 6 or K4 is None:
        raise ValueError("expected (Nc, 6) cameras with K4, or (Nc, 9) cameras without")
    from .problem import BAProblem
    return BAProblem(cams, pts, cam_idx, pt_idx, uv, np.asarray(K4, dtype=np.float64).reshape(4), fixed_cam=0).validate()


def chain_edges(tracks):
    """``(edge_a, edge_b)`` int32 joining the consecutive members of every track: the edges that, fed back to build_tracks,
    reproduce the tracks.  The incremental use: pass them next to a new image's matches, then read ``node_track`` of each old
    track's first member (``track_node[track_off[t]]``) to carry point number t over."""
    node = np.asarray(tracks["track_node"], dtype=np.int32)
    track_off = np.asarray(tracks["track_off"], dtype=np.int64)
    first = np.zeros(node.shape[0], dtype=bool)
    first[track_off[:-1]] = True                              # (no track is empty)
    later = np.nonzero(~first)[0]
    return node[later - 1].copy(), node[later].copy()
