"""The correspondence sets of the ba_align tests at the borders of its reduction grid: ALIGN_THREADS correspondences per
workgroup and pass, one partial row per workgroup, at most ALIGN_MAX_BLOCKS workgroups.  Shared by
tests/test_gpu_similarity.py (the device) and tests/test_similarity_host.py (the check that a fold which dropped the last
rows would be seen)."""
import functools

import numpy as np

from bundle_adjustment_amd.hip_backend import ALIGN_MAX_BLOCKS, ALIGN_THREADS
from bundle_adjustment_amd.synthetic import make_problem
from tests import similarity_reference as sr

NOISE = 0.05
HEAVY, HEAVY_WEIGHT = 40, 1000.0
TOL = 1e-10         # the tolerance of test_gpu_similarity.py's parity tests on s, R, t / max(1, |t0|) and the errors
# correspondence counts: 64 partial rows and one more; every workgroup of the grid with one correspondence per thread, and
# one more, which the first thread of the first workgroup takes in a second trip of its grid-stride loop
BORDER_COUNTS = (64 * ALIGN_THREADS, 64 * ALIGN_THREADS + 1, ALIGN_MAX_BLOCKS * ALIGN_THREADS, ALIGN_MAX_BLOCKS * ALIGN_THREADS + 1)
SIM = (0.8, np.array([-3.0, 1.0, 2.0]))


def partial_rows(nn):
    """(workgroups = partial rows of a pass, most correspondences a thread takes) for nn correspondences."""
    blocks = min(-(-nn // ALIGN_THREADS), ALIGN_MAX_BLOCKS)
    return blocks, -(-nn // (blocks * ALIGN_THREADS))


@functools.lru_cache(maxsize=None)
def border_scene(nn):
    """3 cameras and nn - 3 points with two observations each (the problem only has to exist on the handle).  a: the camera
    centres, then the points.  b: the similarity SIM (and a rotation drawn from nn) applied to a, plus N(0, NOISE) noise;
    the last HEAVY rows weigh HEAVY_WEIGHT and draw their noise from another stream, so a sum that dropped them, or took
    them twice, moves s, R and t far outside the tolerance.  -> (problem, a, b, w, (s0, R0, t0))."""
    prob = make_problem(3, nn - 3, 2, seed=nn % 1000)
    a = np.concatenate([sr.centres(prob.cams), prob.pts])
    assert a.shape == (nn, 3)
    rng = np.random.default_rng(nn)
    s0, t0 = SIM
    R0 = sr.random_rotation(rng)
    b = s0 * a @ R0.T + t0 + rng.normal(0.0, NOISE, size=a.shape)
    b[-HEAVY:] = s0 * a[-HEAVY:] @ R0.T + t0 + np.random.default_rng(nn + 7).normal(0.0, NOISE, size=(HEAVY, 3))
    w = np.ones(nn)
    w[-HEAVY:] = HEAVY_WEIGHT
    return prob, a, b, w, (s0, R0, t0)
