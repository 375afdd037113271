"""GPU: the staging the four pair-shaped calls share (pairs_upload of csrc/ba_hip.hip: ba_relative_pose, ba_homography and
ba_fundamental at two doubles per point, ba_sim3 at three), for each call on one handle:
(a) three pairs without a match -- buffers of one element, nothing uploaded -- return FEW_MATCHES for every pair;
(b) a small call (pairs of 0, K, K + 1 and 40 matches, K the call's minimal sample, n_hyp 64), one pair of 600 matches with n_hyp
4096, the small call again: the staging grows and is reused, and the two small results are the same bits, which a fresh handle
returns as well."""
import numpy as np
import pytest

from tests import relpose_reference as RP
from tests import sim3_reference as S3

pytestmark = pytest.mark.gpu

FEW_MATCHES = 1                # of all four status enums
CALLS = {"relative_pose": 5, "homography": 4, "sim3": 3, "fundamental": 7}   # the call's minimal sample


def _points(name, n, seed):
    """n matches of a scene: pixels (n, 2) | (n, 2), for sim3 points (n, 3) | (n, 3)."""
    width = 3 if name == "sim3" else 2
    if n == 0:
        return np.zeros((0, width)), np.zeros((0, width))
    return S3.noisy_scene(seed, n)[:2] if width == 3 else RP.noisy_scene(n, planar=name == "homography", seed=seed)[:2]


def _call(s, name, counts, seed0, **opts):
    sets = [_points(name, n, seed0 + i) for i, n in enumerate(counts)]
    a, b = np.concatenate([x[0] for x in sets]), np.concatenate([x[1] for x in sets])
    off = np.r_[0, np.cumsum(counts)].astype(np.int64)
    head = () if name == "fundamental" else (RP.K_TEST,)
    return getattr(s, name)(*head, a, b, off, **opts)


def _same(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)


@pytest.fixture(scope="module")
def solver():
    import __graft_entry__ as g
    g.build()
    from bundle_adjustment_amd import hip_backend
    with hip_backend.Solver(0) as s:
        yield s


@pytest.mark.parametrize("name", CALLS)
def test_staging_empty_grown_and_reused(solver, name):
    from bundle_adjustment_amd import hip_backend
    k = CALLS[name]
    r = _call(solver, name, (0, 0, 0), 0)
    assert r["status"].tolist() == [FEW_MATCHES] * 3 and r["n_inliers"].tolist() == [0, 0, 0] and r["match_inlier"].shape == (0,)
    counts = (0, k, k + 1, 40)
    first = _call(solver, name, counts, 10, n_hyp=64)
    big = _call(solver, name, (600,), 20, n_hyp=4096)
    again = _call(solver, name, counts, 10, n_hyp=64)
    with hip_backend.Solver(0) as fresh:
        alone = _call(fresh, name, counts, 10, n_hyp=64)
    print(f"{name}: status {first['status'].tolist()}, inliers {first['n_inliers'].tolist()}; the large pair: status {big['status'].tolist()}, "
          f"{big['n_inliers'].tolist()} inliers")
    assert first["status"][0] == FEW_MATCHES and first["status"][1] == FEW_MATCHES      # n = K is below every call's n >= K + 1
    assert first["n_inliers"][3] > 0 and big["n_inliers"][0] > 0                        # the calls ran on their data
    assert _same(first, again) and _same(first, alone)
