"""GPU: ba_match_guided (Hamming 2-NN over the train rows a window / epipolar gate admits) against the numpy yardstick of
tests/guided_match_reference.py.  The distances are integers and the gate is fp64 with every operation rounded on its own on both
sides: every comparison is exact equality on every output array, n_cand included.

Keypoints are dyadic (multiples of 1/4 px in a 64 x 48 image) and so are window centres, radii and max_epi_px in the edge
cases: squared distances are exact multiples of 1/16, and many rows sit exactly on the border of a gate."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import guided_match_reference as G
from tests import match_reference as M
from tests import relpose_reference as R

pytestmark = pytest.mark.gpu

F_ROWS = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], dtype=np.float64)      # pure x-translation: the query's line is y = y1


@pytest.fixture(scope="module")
def hb():
    import __graft_entry__ as g
    g.build()
    from bundle_adjustment_amd import hip_backend
    return hip_backend


@pytest.fixture(scope="module")
def solver(hb):
    with hb.Solver(0) as s:
        yield s


def _rand(rng, n, width=32):
    return rng.integers(0, 256, (n, width), dtype=np.uint8)


def _dyadic(rng, n, w=64, h=48):
    return np.c_[rng.integers(0, 4 * w, n), rng.integers(0, 4 * h, n)].astype(np.float32) / 4


RADII = np.array([-1, 0, 0.25, 1, 2.5, 5, 10, 30, 100], dtype=np.float32)


def _windows(rng, n):
    return np.c_[_dyadic(rng, n), rng.choice(RADII, n)].astype(np.float32)


def _some_F(rng):
    """A fundamental matrix of a small image: a rotation of a few degrees and a sideways translation."""
    from bundle_adjustment_amd import features
    K = np.array([[60.0, 0, 32], [0, 60, 24], [0, 0, 1]])
    Rm, t = R.make_pose(rng)
    return features.fundamental(K, Rm, t)


def _check(solver, sets, kps, pairs=None, **kw):
    got = solver.match_guided(sets, kps, pairs, **kw)
    G.assert_equal(got, G.match_guided(sets, kps, pairs, **kw))
    return got


# ------------------------------------------------------------------------------------------- 1: edges of tile, block and split
NQS, NTS = (1, 255, 256, 257), (0, 1, 63, 64, 65, 127, 128, 129, 300)


@pytest.mark.parametrize("width", [8, 32, 64])
@pytest.mark.parametrize("gate", ["window", "epipolar"])
def test_edges(solver, gate, width):
    """Every (nq, nt) of the grid as one pair of one call, with and without mutual."""
    rng = np.random.default_rng(100 + width + (gate == "window"))
    sets = [_rand(rng, n, width) for n in NTS + NQS]
    kps = [_dyadic(rng, n) for n in NTS + NQS]
    pairs = [(len(NTS) + a, b) for a in range(len(NQS)) for b in range(len(NTS))]
    rows = sum(NQS) * len(NTS)
    if gate == "window":
        kw = dict(window=_windows(rng, rows))
    else:
        kw = dict(fundamental=np.array([F_ROWS if p % 2 == 0 else _some_F(rng) for p in range(len(pairs))]), max_epi_px=1.5)
    seen = set()
    for mutual in (0, 1):
        got = _check(solver, sets, kps, pairs, mutual=mutual, ratio=0.9, **kw)
        seen |= set(got["n_cand"].tolist())
        assert got["n_good"].sum() > 0
    assert {0, 1, 2} <= seen and max(seen) > 10, sorted(seen)


# ------------------------------------------------------------------------------------------------------- 2: the gates' borders
def test_window_border_on_device(solver):
    rng = np.random.default_rng(2)
    train_xy = np.array([[3, 4], [3.25, 4], [0, 0], [np.nan, 4], [-3, -4]], dtype=np.float32)
    r5 = np.float32(5)
    win = np.array([[0, 0, r5], [0, 0, np.nextafter(r5, np.float32(0))], [0, 0, -1], [0, 0, -0.0], [0, 0, np.nan], [np.nan, 0, 5],
                    [0, 0, np.inf], [0, 0, 1e30]], dtype=np.float32)
    q, t = _rand(rng, len(win)), _rand(rng, len(train_xy))
    got = _check(solver, [q, t], [np.zeros((len(win), 2), dtype=np.float32), train_xy], window=win, ratio=0)
    assert got["n_cand"].tolist() == [3, 1, 0, 1, 0, 0, 4, 4]
    d = M.distances(q[:2], t)
    assert got["best"][0] == min((d[0, j], j) for j in (0, 2, 4))[1] and got["best"][1] == 2      # row 0 of the train set: in, then out
    assert got["best"][2:6].tolist() == [-1, 2, -1, -1]


def test_epipolar_border_on_device(solver):
    rng = np.random.default_rng(3)
    y1 = np.float32(10.25)
    beyond = np.nextafter(np.float32(y1 + 3), np.float32(np.inf))
    qxy = np.array([[5, y1], [np.nan, y1], [5, np.nan]], dtype=np.float32)
    txy = np.array([[0, y1 + 3], [100, y1 - 3], [7, beyond], [7, y1], [np.nan, y1], [7, np.nan]], dtype=np.float32)
    q, t = _rand(rng, 3), _rand(rng, 6)
    got = _check(solver, [q, t], [qxy, txy], fundamental=F_ROWS[None], max_epi_px=3.0, ratio=0)
    assert got["n_cand"].tolist() == [3, 0, 0]                    # at exactly max_epi_px: in; one float32 ulp beyond: out; NaN: out
    assert got["best"][0] in (0, 1, 3) and got["best"][1:].tolist() == [-1, -1]
    got = _check(solver, [q, t], [qxy, txy], fundamental=F_ROWS[None], max_epi_px=0.0, ratio=0)
    assert got["n_cand"].tolist() == [1, 0, 0] and got["best"][0] == 3
    got = _check(solver, [q, t], [qxy, txy], fundamental=np.zeros((1, 3, 3)), max_epi_px=3.0, ratio=0)
    assert not got["n_cand"].any() and (got["best"] == -1).all() and not got["good"].any()       # F = 0: n = 0 admits nothing


# ------------------------------------------------------------------------------------------------------ 3: all-admitting gate
def test_all_admitting_gate_equals_plain_matcher(solver):
    rng = np.random.default_rng(4)
    sets = [_rand(rng, 70), _rand(rng, 300), _rand(rng, 2), _rand(rng, 257)]
    sets[1][[5, 200]] = sets[0][9]
    kps = [_dyadic(rng, len(s)) for s in sets]
    pairs = [(0, 1), (1, 0), (0, 2), (3, 1), (3, 3), (1, 3)]
    rows = sum(len(sets[a]) for a, _ in pairs)
    win = np.c_[_dyadic(rng, rows), np.full(rows, 1e30, dtype=np.float32)]
    for kw in (dict(), dict(mutual=1), dict(ratio=0, max_distance=90, mutual=1)):
        for single in (0, 1):
            got = _check(solver, sets, kps, pairs, window=win, single=single, **kw)
            plain = solver.match_descriptors(sets, pairs, **kw)
            for k in M.KEYS:
                assert np.array_equal(got[k], plain[k]), k
            assert np.array_equal(got["n_cand"], np.concatenate([np.full(len(sets[a]), len(sets[b])) for a, b in pairs]))


# ---------------------------------------------------------------------------------------------------- 4: split independence
def test_forced_split_counts_agree(hb):
    """BA_DEBUG_MATCH_SPLITS (read when the handle is created) asks for 1, 2, 3 and 5 splits: bit-equal outputs."""
    rng = np.random.default_rng(5)
    q, t = _rand(rng, 257), _rand(rng, 700)
    t[[3, 131, 259, 400, 699]] = q[100]
    kps = [_dyadic(rng, 257), _dyadic(rng, 700)]
    kps[1][[3, 131, 259, 400, 699]] = kps[0][100] + np.float32([[0, 0], [1, 0], [0, 1], [3, 4], [0, -1.5]])
    win = np.c_[kps[0], np.full(257, 5, dtype=np.float32)]
    cases = [dict(window=win, mutual=m) for m in (0, 1)] + [dict(fundamental=F_ROWS[None], max_epi_px=1.5, mutual=m) for m in (0, 1)]
    refs = [G.match_guided([q, t], kps, ratio=0.9, **kw) for kw in cases]
    assert refs[0]["n_cand"][100] >= 5 and refs[2]["n_cand"][100] >= 5
    old = os.environ.get("BA_DEBUG_MATCH_SPLITS")
    try:
        for n in (None, 1, 2, 3, 5):
            if n is None:
                os.environ.pop("BA_DEBUG_MATCH_SPLITS", None)
            else:
                os.environ["BA_DEBUG_MATCH_SPLITS"] = str(n)
            with hb.Solver(0) as s:
                for kw, ref in zip(cases, refs):
                    G.assert_equal(s.match_guided([q, t], kps, ratio=0.9, **kw), ref)
    finally:
        if old is None:
            os.environ.pop("BA_DEBUG_MATCH_SPLITS", None)
        else:
            os.environ["BA_DEBUG_MATCH_SPLITS"] = old


# ------------------------------------------------------------------------------------------------------ 5: mutual under the gate
def test_mutual_uses_the_same_gate(solver):
    """Train row 0's best query without a gate is query 0 (distance 0), whose window excludes it: under the gate query 1 is
    row 0's best query and keeps it."""
    rng = np.random.default_rng(6)
    t = _rand(rng, 130)
    q = _rand(rng, 70)
    q[0] = t[0]
    q[1] = t[0]
    q[1, 0] ^= np.uint8(0x1f)                                     # distance 5 from train row 0
    kps = [np.zeros((70, 2), dtype=np.float32), _dyadic(rng, 130) + np.float32(100)]
    kps[1][0] = (10, 10)
    win = np.c_[_dyadic(rng, 70), np.full(70, 3, dtype=np.float32)]
    win[0] = (20, 20, 3)
    win[1] = (10, 12, 2)
    plain = solver.match_descriptors([q, t], mutual=1, ratio=0)
    assert plain["best"][:2].tolist() == [0, 0] and plain["good"][:2].tolist() == [True, False]
    got = _check(solver, [q, t], kps, window=win, mutual=1, ratio=0)
    assert got["best"][:2].tolist() == [-1, 0] and got["good"][:2].tolist() == [False, True] and got["dist1"][1] == 5


# ---------------------------------------------------------------------------------- 6: single, ratio, max_distance; batches; reuse
def test_single_ratio_and_max_distance(solver):
    rng = np.random.default_rng(7)
    q, t = _rand(rng, 200), _rand(rng, 150)
    t[:100] = q[:100]
    t[:100, 3] ^= np.uint8(7)                                     # true partners at distance 3
    kps = [_dyadic(rng, 200), _dyadic(rng, 150)]
    kps[1][:100] = kps[0][:100]
    win = np.c_[kps[0], rng.choice(np.float32([0, 0.5, 2, 6]), 200)]
    counts = set()
    for single in (0, 1):
        for ratio in (0.75, 0, -1.0):
            for max_distance in (-1, 2, 3):
                got = _check(solver, [q, t], kps, window=win, single=single, ratio=ratio, max_distance=max_distance)
                one = got["n_cand"] == 1                          # (the ratio test has no second neighbour to look at)
                near = got["dist1"][one] <= (max_distance if max_distance >= 0 else 512)
                assert one.sum() >= 20 and np.array_equal(got["good"][one], near & (single == 1 or ratio <= 0))
                counts.add(int(got["n_good"][0]))
    assert len(counts) >= 4


def test_pair_alone_equals_pair_in_batch(solver):
    rng = np.random.default_rng(8)
    sets = [_rand(rng, 70), _rand(rng, 389), _rand(rng, 0), _rand(rng, 300)]
    kps = [_dyadic(rng, len(s)) for s in sets]
    pairs = [(0, 1), (1, 0), (2, 1), (0, 2), (3, 3)]
    rows = sum(len(sets[a]) for a, _ in pairs)
    off = np.r_[0, np.cumsum([len(sets[a]) for a, _ in pairs])]
    win = _windows(rng, rows)
    Fs = np.array([F_ROWS, _some_F(rng), F_ROWS, F_ROWS, _some_F(rng)])
    for mutual in (0, 1):
        for gate in ("window", "epipolar"):
            kw = dict(window=win) if gate == "window" else dict(fundamental=Fs, max_epi_px=1.5)
            batch = _check(solver, sets, kps, pairs, mutual=mutual, **kw)
            for p, (a, b) in enumerate(pairs):
                kw1 = dict(window=win[off[p]:off[p + 1]]) if gate == "window" else dict(fundamental=Fs[p:p + 1], max_epi_px=1.5)
                if a != b:
                    alone = solver.match_guided([sets[a], sets[b]], [kps[a], kps[b]], [(0, 1)], mutual=mutual, **kw1)
                else:
                    alone = solver.match_guided([sets[a]], [kps[a]], [(0, 0)], mutual=mutual, **kw1)
                for k in ("best", "second", "dist1", "dist2", "good", "n_cand"):
                    assert np.array_equal(alone[k], batch[k][off[p]:off[p + 1]]), (p, k)
                assert alone["n_good"][0] == batch["n_good"][p]


def test_two_gates_on_one_handle_and_coexistence(hb):
    from bundle_adjustment_amd.synthetic import make_problem
    rng = np.random.default_rng(9)
    small, large = [_rand(rng, 20), _rand(rng, 30)], [_rand(rng, 700), _rand(rng, 900)]
    ksmall, klarge = [_dyadic(rng, 20), _dyadic(rng, 30)], [_dyadic(rng, 700), _dyadic(rng, 900)]
    wsmall, wlarge = _windows(rng, 20), _windows(rng, 700)
    prob = make_problem(8, 400, 4, seed=0)
    kw = dict(max_iters=5, loss="huber")
    with hb.Solver(0) as s:
        for sets, kps, win in ((small, ksmall, wsmall), (large, klarge, wlarge), (small, ksmall, wsmall)):      # the staging grows, then holds more
            _check(s, sets, kps, window=win, mutual=1)
            _check(s, sets, kps, fundamental=F_ROWS[None], max_epi_px=1.5, mutual=1)
            M.assert_equal(s.match_descriptors(sets, mutual=1), M.match_descriptors(sets, mutual=1))
        s.set_problem(prob)
        plain = s.solve(**kw)
        cams0, pts0 = s.get_params()
        s.set_problem(prob)
        _check(s, large, klarge, window=wlarge)
        _check(s, large, klarge, fundamental=_some_F(rng)[None])
        mixed = s.solve(**kw)
        cams1, pts1 = s.get_params()
    assert np.array_equal(cams0, cams1) and np.array_equal(pts0, pts1)
    assert (plain["final_cost"], plain["iterations"]) == (mixed["final_cost"], mixed["iterations"])


# --------------------------------------------------------------------------------------------------------------- 7: refusals
def _raw(solver, width=32, set_off=None, desc=None, xy=None, pq=None, pt=None, opts=None, window=None, F=None, n_sets=None, n_pairs=None):
    i64, i32, u8, f32, f64 = (C.POINTER(t) for t in (C.c_int64, C.c_int32, C.c_uint8, C.c_float, C.c_double))

    def ptr(a, t):
        return None if a is None else a.ctypes.data_as(t)
    o = solver.guided_options(**(opts or {}))
    rows = np.zeros(1 << 12, dtype=np.int32)
    return solver._lib.ba_match_guided(solver._h, width, len(set_off) - 1 if n_sets is None else n_sets, ptr(set_off, i64), ptr(desc, u8),
                                       ptr(xy, f32), (0 if pq is None else len(pq)) if n_pairs is None else n_pairs, ptr(pq, i32), ptr(pt, i32),
                                       C.byref(o), ptr(window, f32), ptr(F, f64), None, ptr(rows, i32), None, None, None, None, None, None)


def test_refusals(solver, hb):
    rng = np.random.default_rng(10)
    desc, xy = _rand(rng, 10), _dyadic(rng, 10)
    off = np.array([0, 4, 10], dtype=np.int64)
    pq, pt = np.array([0], dtype=np.int32), np.array([1], dtype=np.int32)
    win, F = _windows(rng, 4), F_ROWS.copy()
    big, many = np.zeros(65537, dtype=np.int64), np.zeros(65536, dtype=np.int32)
    W, E = dict(gate=1), dict(gate=2)
    bad_F = [F.copy() for _ in range(2)]
    bad_F[0][1, 1], bad_F[1][2, 0] = np.nan, np.inf
    cases = [
        ("desc_bytes", dict(width=12)), ("desc_bytes", dict(width=0)), ("desc_bytes", dict(width=72)),
        ("n_sets", dict(set_off=big, desc=None)), ("n_sets", dict(n_sets=-1)),
        ("n_pairs", dict(pq=many, pt=many)), ("n_pairs", dict(n_pairs=-1)),
        ("ratio", dict(opts=dict(ratio=float("nan"), **W))), ("ratio", dict(opts=dict(ratio=float("inf"), **W))),
        ("set_off", dict(set_off=None, n_sets=2)), ("set_off", dict(set_off=np.array([1, 4, 10], dtype=np.int64))),
        ("set_off", dict(set_off=np.array([0, 6, 4], dtype=np.int64))),
        ("set_off", dict(set_off=np.array([0, 4, 4 + hb.MATCH_MAX_SET + 1], dtype=np.int64))),
        ("desc", dict(desc=None)), ("pair_query", dict(pq=None, n_pairs=1)), ("pair_train", dict(pt=None)),
        ("pair_query", dict(pq=np.array([2], dtype=np.int32))), ("pair_query", dict(pq=np.array([-1], dtype=np.int32))),
        ("pair_train", dict(pt=np.array([2], dtype=np.int32))), ("pair_train", dict(pt=np.array([-1], dtype=np.int32))),
        ("xy", dict(xy=None)), ("gate", dict(opts=dict(gate=0))), ("gate", dict(opts=dict(gate=3))), ("gate", dict(opts=dict(gate=-1))),
        ("window", dict(window=None)), ("F", dict(opts=E, F=None)), ("F", dict(opts=E, F=bad_F[0])), ("F", dict(opts=E, F=bad_F[1])),
        ("max_epi_px", dict(opts=dict(max_epi_px=float("nan"), **E))), ("max_epi_px", dict(opts=dict(max_epi_px=float("inf"), **E))),
        ("max_epi_px", dict(opts=dict(max_epi_px=-1.0, **E))),
        ("single", dict(opts=dict(single=2, **W))), ("single", dict(opts=dict(single=-1, **E))),
    ]
    for name, change in cases:
        kw = dict(width=32, set_off=off, desc=desc, xy=xy, pq=pq, pt=pt, opts=W, window=win, F=F)
        kw.update(change)
        rc = _raw(solver, **kw)
        msg = solver._lib.ba_last_error().decode()
        assert rc == -1 and msg.startswith("ba_match_guided: ") and name in msg.split(": ", 1)[1], (name, change.keys(), rc, msg)
        _check(solver, [desc[:4], desc[4:]], [xy[:4], xy[4:]], window=win)                       # the handle works afterwards
    assert solver._lib.ba_match_guided(None, 32, 0, None, None, None, 0, None, None, None, *([None] * 10)) == -1
    # not refused: a window gate needs no F, an epipolar gate no window; non-finite xy and window values fail the gate
    assert _raw(solver, set_off=off, desc=desc, xy=xy, pq=pq, pt=pt, opts=W, window=win, F=None) == 0
    assert _raw(solver, set_off=off, desc=desc, xy=xy, pq=pq, pt=pt, opts=E, window=None, F=F) == 0
    got = _check(solver, [desc[:4], desc[4:]], [xy[:4], np.full((6, 2), np.inf, dtype=np.float32)], window=win)
    assert not got["n_cand"].any()
    # the wrapper's own refusals
    for bad in (dict(), dict(window=win, fundamental=F)):
        with pytest.raises(ValueError, match="exactly one"):
            solver.match_guided([desc[:4], desc[4:]], [xy[:4], xy[4:]], **bad)
    with pytest.raises(ValueError, match="keypoint"):
        solver.match_guided([desc[:4], desc[4:]], [xy[:4]], window=win)
    with pytest.raises(ValueError, match="keypoints"):
        solver.match_guided([desc[:4], desc[4:]], [xy[:4], xy[:5]], window=win)
    # no-ops with well-formed outputs
    out = _check(solver, [], [], [], window=np.zeros((0, 3), dtype=np.float32))
    assert out["row_off"].tolist() == [0] and out["n_cand"].shape == (0,)
    out = _check(solver, [desc[:0], desc[:0]], [xy[:0], xy[:0]], [(0, 1), (1, 0)], fundamental=np.array([F, F]))
    assert out["row_off"].tolist() == [0, 0, 0] and out["n_good"].tolist() == [0, 0]


# --------------------------------------------------------------------------------------------------------- 8: planted scene
N_PLANTED, IMAGE = 400, (1280, 720)


def planted_scene(seed=0, n=N_PLANTED, max_epi_px=3.0, radius_px=8.0):
    """n 3-D points seen by two pinhole views (R.K_TEST, the pose of R.make_pose, 0.3 px of noise truncated at 1 px), a 32-byte
    descriptor per point, in view 2 shuffled and with up to 20 bits flipped.  A quarter of the points get a DECOY in view 2: an
    exact copy of their view-2 descriptor on a keypoint drawn again until it lies at least 3 x max_epi_px from the point's
    epipolar line and 3 x radius_px from its projection.  -> dict(X, R, t (view 2: x ~ K (R X + t)), des1, kp1, des2, kp2,
    partner (view-2 row of point i), decoyed (n,) bool)."""
    from bundle_adjustment_amd import features
    rng = np.random.default_rng(seed)
    Rm, t = R.make_pose(rng)
    t = R.BASELINE * t
    X = np.c_[rng.uniform(-2.0, 2.0, n), rng.uniform(-1.5, 1.5, n), rng.uniform(4.0, 8.0, n)]
    Y = X @ Rm.T + t
    p1 = ((X / X[:, 2:]) @ R.K_TEST.T)[:, :2] + R.truncated_noise(rng, (n, 2))
    proj2 = ((Y / Y[:, 2:]) @ R.K_TEST.T)[:, :2]
    p2 = proj2 + R.truncated_noise(rng, (n, 2))
    d1 = _rand(rng, n)
    d2 = d1.copy()
    for r in range(n):
        for bit in rng.choice(256, rng.integers(0, 21), replace=False):
            d2[r, bit // 8] ^= np.uint8(1 << (bit % 8))
    decoyed = np.zeros(n, dtype=bool)
    decoyed[rng.choice(n, n // 4, replace=False)] = True
    F = features.fundamental(R.K_TEST, Rm, t)
    lines = np.c_[p1.astype(np.float32).astype(np.float64), np.ones(n)] @ F.T
    who = np.nonzero(decoyed)[0]
    spot = np.zeros((len(who), 2))
    todo = np.arange(len(who))
    while todo.size:
        spot[todo] = np.c_[rng.uniform(0, IMAGE[0], todo.size), rng.uniform(0, IMAGE[1], todo.size)]
        ln = lines[who[todo]]
        epi = np.abs((ln[:, :2] * spot[todo]).sum(1) + ln[:, 2]) / np.hypot(ln[:, 0], ln[:, 1])
        far = np.hypot(*(spot[todo] - proj2[who[todo]]).T)
        todo = todo[(epi < 3 * max_epi_px + 1) | (far < 3 * radius_px + 1)]
    perm = rng.permutation(n + len(who))
    des2 = np.concatenate([d2, d2[who]])[perm]
    kp2 = np.concatenate([p2, spot])[perm]
    partner = np.argsort(perm)[:n]
    return dict(X=X, R=Rm, t=t, des1=d1, kp1=p1, des2=des2, kp2=kp2, partner=partner, decoyed=decoyed)


def test_planted_scene(solver):
    from bundle_adjustment_amd import features
    sc = planted_scene()
    n = N_PLANTED
    # properties of the scene, on the yardsticks alone first
    plain_ref = M.match_pair(sc["des1"], sc["des2"])
    assert not plain_ref["good"][sc["decoyed"]].any() and plain_ref["good"][~sc["decoyed"]].all()
    F = features.fundamental(R.K_TEST, sc["R"], sc["t"])
    epi_ref = G.match_pair_guided(sc["des1"], sc["des2"], G.gate_epipolar(F, sc["kp1"], sc["kp2"], 3.0))
    assert epi_ref["good"].all() and np.array_equal(epi_ref["best"], sc["partner"])
    # the device
    plain = solver.match_descriptors([sc["des1"], sc["des2"]])
    assert not plain["good"][sc["decoyed"]].any() and plain["n_good"][0] == n - n // 4
    q, tr, dist = features.match_epipolar(sc["des1"], sc["kp1"], sc["des2"], sc["kp2"], R.K_TEST, sc["R"], sc["t"], solver=solver)
    assert q.tolist() == list(range(n)) and np.array_equal(tr, sc["partner"])
    assert np.array_equal(dist, M.distances(sc["des1"], sc["des2"])[np.arange(n), sc["partner"]])
    pi, ki, pdist = features.match_by_projection(R.K_TEST, sc["R"], sc["t"], sc["X"], sc["des1"], sc["kp2"], sc["des2"], 8.0, solver=solver)
    assert pi.tolist() == list(range(n)) and np.array_equal(ki, sc["partner"]) and np.array_equal(pdist, dist)
    assert len(q) > plain["n_good"][0] and len(pi) > plain["n_good"][0]


# ----------------------------------------------------------------------------------------------------------------- 9: chain
class _KeyPoint:
    def __init__(self, pt):
        self.pt = (float(pt[0]), float(pt[1]))


CHAIN_EPI_PX = 3.0


def test_chain_match_pose_then_guided_match(solver):
    """BruteForceMatcher.match -> estimate_pose -> match_epipolar with the ESTIMATED pose on the planted scene: every
    returned match is a planted one, and there are at least as many as the pose estimate had inliers.

    Fixed on the CPU beforehand with tests/relpose_reference.py's relative_pose on the yardstick's plain matches (the 300
    points without a decoy) and the yardstick's gate under that pose, seed 0 and max_epi_px = 3.0: all 400 planted
    correspondences lie within 1.25 px of their epipolar line (1.75 px inside the gate), the nearest decoy to its point's line
    is 20.0 px away (17 px outside it), and the yardstick returns 400 matches, all planted, against 300 inliers; the same
    outcome at max_epi_px = 2 and 4 and with seeds 1 and 2 (1.56 / 1.42 px, decoys at 11.0 / 11.8 px).  The device's pose is not
    the reference's bit for bit (4l), which is what the margin is for."""
    from bundle_adjustment_amd import estimate_pose, features
    sc = planted_scene()
    kp1, kp2 = [_KeyPoint(p) for p in sc["kp1"]], [_KeyPoint(p) for p in sc["kp2"]]
    matches = features.BruteForceMatcher(solver=solver).match(sc["des1"], sc["des2"])
    Rm, t, _, _, inl = estimate_pose(matches, kp1, kp2, R.K_TEST, solver=solver, quiet=True)
    assert Rm is not None
    q, tr, _ = features.match_epipolar(sc["des1"], kp1, sc["des2"], kp2, R.K_TEST, Rm, t, max_epi_px=CHAIN_EPI_PX, solver=solver)
    assert np.array_equal(tr, sc["partner"][q])
    assert len(q) >= len(inl)
