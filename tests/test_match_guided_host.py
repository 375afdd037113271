"""CPU: the numpy yardstick of ba_match_guided (tests/guided_match_reference.py) against a plain triple loop and at the gates'
border cases; features.fundamental / match_epipolar / match_by_projection over a fake solver that answers from the yardstick;
the options struct and the exported symbols."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import guided_match_reference as G
from tests import match_reference as M
from tests import relpose_reference as R


def _rand(rng, n, width=32):
    return rng.integers(0, 256, (n, width), dtype=np.uint8)


def _dyadic(rng, n, w=64, h=48):
    return np.c_[rng.integers(0, 4 * w, n), rng.integers(0, 4 * h, n)].astype(np.float32) / 4


# ---------------------------------------------------------------------------------------------------------- the yardstick
def _loops(q, t, gate, ratio, max_distance, mutual, single):
    """The header's definition, literally: three nested Python loops."""
    nq, nt = len(q), len(t)
    d = [[sum(bin(int(a) ^ int(b)).count("1") for a, b in zip(q[i], t[j])) for j in range(nt)] for i in range(nq)]
    out = dict(best=[], second=[], dist1=[], dist2=[], good=[], n_cand=[])
    for i in range(nq):
        keys = sorted((d[i][j], j) for j in range(nt) if gate[i][j])
        b, s = (keys[0] if keys else (-1, -1)), (keys[1] if len(keys) > 1 else (-1, -1))
        g = bool(keys)
        if ratio > 0:
            g = g and ((len(keys) == 1 and single == 1) or (len(keys) > 1 and float(b[0]) < ratio * float(s[0])))
        if max_distance >= 0:
            g = g and b[0] <= max_distance
        if mutual and g:
            g = min((d[k][b[1]], k) for k in range(nq) if gate[k][b[1]])[1] == i
        for k, v in zip(("best", "second", "dist1", "dist2", "good", "n_cand"), (b[1], s[1], b[0], s[0], g, len(keys))):
            out[k].append(v)
    return out


@pytest.mark.parametrize("seed", range(4))
def test_yardstick_against_loops(seed):
    rng = np.random.default_rng(seed)
    nq, nt = 9, 7
    q, t = _rand(rng, nq, 8), _rand(rng, nt, 8)
    t[2] = t[5] = q[3]                                           # ties
    q[4] = q[3]
    gate = rng.random((nq, nt)) < (0.2, 0.5, 0.8, 1.0)[seed]
    gate[0] = False
    gate[1] = False
    gate[1, 4] = True                                            # exactly one candidate
    for ratio in (0.75, 1.0, 0):
        for max_distance in (-1, 24):
            for mutual in (0, 1):
                for single in (0, 1):
                    ref = G.match_pair_guided(q, t, gate, ratio, max_distance, mutual, single)
                    want = _loops(q, t, gate, ratio, max_distance, mutual, single)
                    for k, v in want.items():
                        assert ref[k].tolist() == v, (k, ratio, max_distance, mutual, single)
                    assert ref["n_good"] == sum(want["good"])


def test_window_gate_borders():
    train = np.array([[3, 4], [3.25, 4], [0, 0], [np.nan, 4], [-3, -4]], dtype=np.float32)
    r5 = np.float32(5)
    below = np.nextafter(r5, np.float32(0))
    win = np.array([[0, 0, r5], [0, 0, below], [0, 0, -1], [0, 0, -0.0], [0, 0, np.nan], [np.nan, 0, 5], [0, 0, np.inf], [0, 0, 1e30]], dtype=np.float32)
    g = G.gate_window(win, train)
    assert g[0].tolist() == [True, False, True, False, True]    # 3-4-5 on the border passes
    assert g[1].tolist() == [False, False, True, False, False]  # one float32 ulp less: fails
    assert not g[2].any() and not g[4].any() and not g[5].any()  # r < 0, NaN radius, NaN centre
    assert g[3].tolist() == [False, False, True, False, False]  # r = -0.0 is not negative: the centre itself
    assert g[6].tolist() == g[7].tolist() == [True, True, True, False, True]


def test_epipolar_gate_borders():
    F = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], dtype=np.float64)      # pure x-translation: the line y = y1
    y1 = np.float32(10.25)
    m = 3.0
    beyond = np.nextafter(np.float32(y1 + 3), np.float32(np.inf))
    q = np.array([[5, y1]], dtype=np.float32)
    t = np.array([[0, y1 + 3], [100, y1 - 3], [7, beyond], [7, y1], [np.nan, y1], [7, np.nan]], dtype=np.float32)
    assert G.gate_epipolar(F, q, t, m)[0].tolist() == [True, True, False, True, False, False]
    assert not G.gate_epipolar(np.zeros((3, 3)), q, t, m).any()  # n = 0 admits nothing
    assert G.gate_epipolar(F, q, t, 0.0)[0].tolist() == [False, False, False, True, False, False]
    assert not G.gate_epipolar(F, np.array([[np.nan, 1]], dtype=np.float32), t, m).any()


def test_all_admitting_gate_reproduces_plain_matcher():
    rng = np.random.default_rng(5)
    q, t = _rand(rng, 40), _rand(rng, 30)
    t[[3, 9]] = q[7]
    for kw in (dict(), dict(ratio=0, mutual=1), dict(ratio=1.0, max_distance=100, mutual=1)):
        plain = M.match_pair(q, t, **kw)
        for single in (0, 1):
            got = G.match_pair_guided(q, t, np.ones((40, 30), dtype=bool), single=single, **kw)
            for k in ("best", "second", "dist1", "dist2", "good"):
                assert np.array_equal(got[k], plain[k]), k
            assert got["n_good"] == plain["n_good"] and (got["n_cand"] == 30).all()
    win = np.c_[_dyadic(rng, 40), np.full(40, 1e30, dtype=np.float32)]
    assert G.gate_window(win, _dyadic(rng, 30)).all()


# -------------------------------------------------------------------------------------------------------------- features
class FakeSolver:
    """hip_backend.Solver.match_guided answered by the yardstick; records what it was given."""

    def __init__(self):
        self.calls = []

    def match_guided(self, sets, keypoints, pairs=None, *, window=None, fundamental=None, **opts):
        self.calls.append(dict(sets=sets, keypoints=keypoints, pairs=pairs, window=window, fundamental=fundamental, opts=opts))
        return G.match_guided(sets, [np.asarray(k, dtype=np.float32) for k in keypoints], pairs, window=window, fundamental=fundamental, **opts)


class _KeyPoint:
    def __init__(self, pt):
        self.pt = (float(pt[0]), float(pt[1]))


def test_fundamental():
    from bundle_adjustment_amd import features
    rng = np.random.default_rng(6)
    p1, p2, Rm, t = R.make_scene(rng, 50)
    F = features.fundamental(R.K_TEST, Rm, t)
    h1, h2 = np.c_[p1, np.ones(50)], np.c_[p2, np.ones(50)]
    num = np.abs(np.einsum("ni,ij,nj->n", h2, F, h1))
    scale = np.einsum("ni,ij,nj->n", np.abs(h2), np.abs(F), np.abs(h1))
    assert (num <= 1e-9 * scale).all(), (num / scale).max()
    assert np.allclose(F, np.linalg.inv(R.K_TEST).T @ R.skew(t) @ Rm @ np.linalg.inv(R.K_TEST), rtol=0, atol=1e-15)
    assert np.allclose(features.fundamental(R.K_TEST.ravel(), Rm.ravel(), 3.0 * t), 3.0 * F, rtol=1e-12, atol=1e-12 * np.abs(F).max())      # flat inputs; linear in t


def test_match_epipolar_over_fake_solver():
    from bundle_adjustment_amd import features
    rng = np.random.default_rng(7)
    n = 40
    p1, p2, Rm, t = R.make_scene(rng, n)
    perm = rng.permutation(n)
    d1 = _rand(rng, n)
    d2 = d1[perm].copy()
    d2[:, 0] ^= np.uint8(1)
    kp2 = p2[perm]
    fake = FakeSolver()
    q, tr, dist = features.match_epipolar(d1, p1, d2, [_KeyPoint(p) for p in kp2], R.K_TEST, Rm, t, max_epi_px=1.0, solver=fake, mutual=1)
    assert q.dtype == tr.dtype == dist.dtype == np.int64
    assert q.tolist() == list(range(n)) and np.array_equal(tr, np.argsort(perm)) and (dist == 1).all()
    call = fake.calls[0]
    assert call["window"] is None and np.asarray(call["fundamental"]).shape == (1, 3, 3) and call["opts"] == dict(max_epi_px=1.0, mutual=1)
    assert np.allclose(call["keypoints"][1], kp2) and np.allclose(call["keypoints"][0], p1)
    # a wrong pose explains (almost) nothing; None and empty inputs
    wrong = features.match_epipolar(d1, p1, d2, kp2, R.K_TEST, np.eye(3), [0.0, 1.0, 0.0], max_epi_px=0.5, solver=fake)
    assert len(wrong[0]) < n // 4
    for a, b in ((None, d2), (d1, None), (d1[:0], d2), (d1, d2[:0])):
        out = features.match_epipolar(a, p1[:0] if a is not None and len(a) == 0 else p1, b, kp2[:0] if b is not None and len(b) == 0 else kp2,
                                      R.K_TEST, Rm, t, solver=fake)
        assert [len(o) for o in out] == [0, 0, 0] and out[0].dtype == np.int64
    assert len(fake.calls) == 2


def test_match_by_projection_over_fake_solver():
    from bundle_adjustment_amd import features
    rng = np.random.default_rng(8)
    n = 30
    Rm, t = R.make_pose(rng)
    X = np.c_[rng.uniform(-2.0, 2.0, n), rng.uniform(-1.5, 1.5, n), rng.uniform(4.0, 8.0, n)]
    X[0] = -(Rm.T @ t) + Rm.T @ np.array([0.1, 0.1, -3.0])      # behind the camera
    X[1] = -(Rm.T @ t) + Rm.T @ np.array([40.0, 0.0, 5.0])      # in front, far outside a 1280 x 720 image
    X[2] = -(Rm.T @ t) + Rm.T @ np.array([0.3, 0.2, -1e-3])     # just behind
    Y = X @ Rm.T + t
    with np.errstate(divide="ignore", invalid="ignore"):
        uv = ((Y / Y[:, 2:]) @ R.K_TEST.T)[:, :2]
    pd = _rand(rng, n)
    perm = rng.permutation(n)
    des = pd[perm].copy()
    des[:, 1] ^= np.uint8(3)
    kp = np.where(np.isfinite(uv), uv, 0.0)[perm] + 0.5
    fake = FakeSolver()
    pi, ki, dist = features.match_by_projection(R.K_TEST, Rm, t, X, pd, kp, des, 2.0, image_size=(1280, 720), solver=fake, ratio=0)
    call = fake.calls[0]
    win = np.asarray(call["window"])
    assert win.dtype == np.float32 and win.shape == (n, 3)
    assert win[:3, 2].tolist() == [-1, -1, -1] and (win[3:, 2] == 2).all() and np.isfinite(win).all()
    assert np.allclose(win[3:, :2], uv[3:], atol=1e-3)
    assert call["fundamental"] is None and len(call["keypoints"][0]) == n and call["opts"] == dict(ratio=0)
    assert pi.tolist() == list(range(3, n)) and np.array_equal(ki, np.argsort(perm)[3:]) and (dist == 2).all()
    # without image_size the point outside the image keeps its window (and its keypoint, half a pixel away)
    pi, ki, _ = features.match_by_projection(R.K_TEST, Rm, t, X, pd, [_KeyPoint(p) for p in kp], des, 2.0, solver=fake, ratio=0)
    assert pi.tolist() == [1] + list(range(3, n)) and fake.calls[1]["window"][1, 2] == 2
    # a radius per point
    rad = np.full(n, 2.0)
    rad[5] = 0.25
    pi, _, _ = features.match_by_projection(R.K_TEST, Rm, t, X, pd, kp, des, rad, image_size=(1280, 720), solver=fake, ratio=0)
    assert pi.tolist() == [k for k in range(3, n) if k != 5]
    for args in ((None, pd, kp, des), (X, None, kp, des), (X, pd, kp, None), (X[:0], pd[:0], kp, des), (X, pd, kp[:0], des[:0])):
        out = features.match_by_projection(R.K_TEST, Rm, t, *args, 2.0, solver=fake)
        assert [len(o) for o in out] == [0, 0, 0] and out[1].dtype == np.int64
    assert len(fake.calls) == 3
    # z = 0 exactly (identity pose): no window, whatever the division gave
    features.match_by_projection(np.eye(3), np.eye(3), np.zeros(3), [[0.3, 0.2, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 1.0]], pd[:3], kp, des, 2.0, solver=fake)
    assert fake.calls[3]["window"].tolist() == [[0, 0, -1], [0, 0, -1], [0, 0, 2]]
    with pytest.raises(ValueError):
        features.match_by_projection(R.K_TEST, Rm, t, X[:5], pd, kp, des, 2.0, solver=fake)


# ------------------------------------------------------------------------------------------------------------------- ABI
def test_guided_options_struct_and_symbols():
    import __graft_entry__ as g
    g.build()
    from bundle_adjustment_amd import hip_backend as hb
    assert C.sizeof(hb.BAGuidedOptions) == 32
    assert [n for n, _ in hb.BAGuidedOptions._fields_] == ["ratio", "max_distance", "mutual", "gate", "single", "max_epi_px"]
    assert hb.BAGuidedOptions.gate.offset == 16 and hb.BAGuidedOptions.max_epi_px.offset == 24
    lib = hb.load_library()
    assert hasattr(lib, "ba_match_guided") and hasattr(lib, "ba_default_guided_options")
    o = hb.BAGuidedOptions()
    assert lib.ba_default_guided_options(C.byref(o)) == 0
    assert (o.ratio, o.max_distance, o.mutual, o.gate, o.single, o.max_epi_px) == (0.75, -1, 0, 0, 1, 3.0)
    assert lib.ba_default_guided_options(None) == -1
    assert hb.GATE == {"window": 1, "epipolar": 2}
    assert math.isclose(o.max_epi_px, 3.0)
