"""The long-track problem of the ba_triangulate_tracks tests: tracks around and beyond TRACK_STAGE views, the number of unit
vectors the long-track kernel stages in LDS at a time, with the two cameras that subtend the widest angle placed in chosen
stages of the observation list.  Shared by tests/test_gpu_tracks.py (the device) and tests/test_tracks_host.py (the check
that a kernel which paired views of one stage only would be seen)."""
import functools

import numpy as np

from bundle_adjustment_amd.bal import BALProblem, from_pinhole
from bundle_adjustment_amd.hip_backend import TRACK_STAGE
from bundle_adjustment_amd.problem import BAProblem
from bundle_adjustment_amd.rotations import rvecs_to_matrices
from bundle_adjustment_amd.synthetic import _project, bal_project, make_problem

K4 = np.array([900.0, 900.0, 640.0, 360.0])
N_SHORT = 50
N_WIDE = 2 * TRACK_STAGE + 76                                    # views of the three tracks with a placed widest pair
N_CAMS = N_WIDE
# views of the tracks on either side of one and of two stages
BORDER_LENGTHS = (TRACK_STAGE - 1, TRACK_STAGE, TRACK_STAGE + 1, 2 * TRACK_STAGE, 2 * TRACK_STAGE + 1)
# positions of the widest pair in the observation list of its track -> the stages (position // TRACK_STAGE) they fall in
WIDE_POSITIONS = ((3, TRACK_STAGE - 2), (TRACK_STAGE - 1, TRACK_STAGE), (TRACK_STAGE + 5, 2 * TRACK_STAGE + 70))
WIDE_STAGES = ((0, 0), (0, 1), (1, 2))
LONG_POINTS = tuple(range(N_SHORT, N_SHORT + len(BORDER_LENGTHS) + len(WIDE_POSITIONS)))
WIDE_POINTS = LONG_POINTS[len(BORDER_LENGTHS):]
NP = N_SHORT + len(LONG_POINTS)


def widest_pair(centres, X):
    """-> (i, j, d2, runner-up d2): the two rows of centres that subtend the widest angle at X."""
    u = centres - X
    u = u / np.sqrt((u * u).sum(axis=1))[:, None]
    d2 = ((u[:, None, :] - u[None, :, :]) ** 2).sum(axis=2)
    i, j = np.unravel_index(int(np.argmax(d2)), d2.shape)
    best = float(d2[i, j])
    d2[i, j] = d2[j, i] = 0.0
    return int(min(i, j)), int(max(i, j)), best, float(d2.max())


@functools.lru_cache(maxsize=None)
def long_track_problem(model):
    """N_CAMS cameras (the table of the point passes does not fit in LDS at that count, for either model).  Points
    0 .. N_SHORT - 1: ordinary tracks of 2-6 views among 12 cameras (median 4: with 2 lanes per point the long-track threshold
    is 8).  Then one track per entry of BORDER_LENGTHS on distinct cameras, and three tracks of N_WIDE views -- every
    camera once -- whose widest pair sits at WIDE_POSITIONS of the track's observations.  Observations of different points
    are interleaved at random, those of one point keep their order.  True cameras, pixels with N(0, 0.5) noise.
    -> (problem, true points, {point: (camera a, camera b) of the widest pair})."""
    rng = np.random.default_rng(23)
    _, cams, pts = make_problem(N_CAMS, NP, 4, seed=9, K4=K4, return_truth=True)
    R = rvecs_to_matrices(cams[:, :3])
    centres = -np.einsum("nji,nj->ni", R, cams[:, 3:6])
    short_cams = np.arange(0, N_CAMS, N_CAMS // 12)[:12]
    ci, pi = [], []
    for p in range(N_SHORT):
        n = 2 + p % 5
        ci += list(rng.choice(short_cams, size=n, replace=False)); pi += [p] * n
    for p, n in zip(LONG_POINTS, BORDER_LENGTHS):
        ci += list(rng.choice(N_CAMS, size=n, replace=False)); pi += [p] * n
    pairs = {}
    for p, (pa, pb) in zip(WIDE_POINTS, WIDE_POSITIONS):
        a, b, best, second = widest_pair(centres, pts[p])
        assert best > second * (1.0 + 1e-4)                        # one widest pair, clear of the runner-up
        rest = [c for c in rng.permutation(N_CAMS) if c not in (a, b)]
        order = rest[:pa] + [a] + rest[pa:pb - 1] + [b] + rest[pb - 1:]
        assert len(order) == N_WIDE and order[pa] == a and order[pb] == b
        ci += order; pi += [p] * N_WIDE
        pairs[p] = (a, b)
    ci, pi = np.array(ci, dtype=np.int32), np.array(pi, dtype=np.int32)
    if model == "bal":
        b = from_pinhole(BAProblem(cams, pts, ci, pi, np.zeros((len(ci), 2)), K4, 0))
        cams = b.cams.copy()
        cams[:, 6] = 900.0 * (1.0 + 0.02 * rng.normal(size=N_CAMS))
        cams[:, 7] = -0.03 + 0.01 * rng.normal(size=N_CAMS)
        cams[:, 8] = 0.003 * rng.choice([-1.0, 1.0], size=N_CAMS)
        uv = bal_project(cams, pts, ci, pi)
    else:
        uv = _project(cams, pts, ci, pi, K4)[0]
    uv = uv + rng.normal(0.0, 0.5, size=uv.shape)
    # interleave the points; inside a point the keys ascend, so its observations keep their order
    keys = rng.random(len(ci))
    for p in range(NP):
        sel = np.nonzero(pi == p)[0]
        keys[sel] = np.sort(keys[sel])
    order = np.argsort(keys, kind="stable")
    ci, pi, uv = ci[order], pi[order], uv[order]
    start = pts + rng.normal(0.0, 0.05, size=pts.shape)
    if model == "bal":
        return BALProblem(cams, start, ci, pi, uv).validate(), pts, pairs
    return BAProblem(cams, start, ci, pi, uv, K4.copy(), 0).validate(), pts, pairs
