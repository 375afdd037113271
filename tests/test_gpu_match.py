"""GPU: ba_match_descriptors (brute-force Hamming 2-NN with the ratio test on the device) against the numpy yardstick of
tests/match_reference.py.  The arithmetic is integer: every comparison is exact equality on every output array.

Shapes.  T = hip_backend.MATCH_TILE train descriptors per LDS tile, B = MATCH_BLOCK queries per workgroup, S = MATCH_MIN_SPLIT
the shortest train split.  The library asks for ceil(8 n_cu / wave rows of the call) splits per pair, at most
nt / S of them and at most MATCH_MAX_SPLITS, in whole tiles: with two wave rows (65 queries) that wish is >= 4 on any device, so
nt = 7 S + 40 = 15 tiles is cut into 4 splits of 4 tiles (one compute unit) or 5 splits of 3 tiles (two units and more), the
last one short."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import match_reference as M
from tests import relpose_reference as R

pytestmark = pytest.mark.gpu


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


def _check(solver, sets, pairs=None, **opts):
    got = solver.match_descriptors(sets, pairs, **opts)
    M.assert_equal(got, M.match_descriptors(sets, pairs, **opts))
    return got


# ------------------------------------------------------------------------------------------- 1: edges of tile, block and split
def test_edges_of_tile_block_and_split(solver, hb):
    """Every (nq, nt) of the grid as one pair of ONE call (a pair's rows do not depend on the others: case 3 checks that), the
    sets drawn once; plus the shape of the module docstring, alone, so that the split rule sees only its two wave rows."""
    T, B, S = hb.MATCH_TILE, hb.MATCH_BLOCK, hb.MATCH_MIN_SPLIT
    rng = np.random.default_rng(1)
    nts, nqs = (1, 2, T - 1, T, T + 1, 2 * T + 3), (1, 63, 64, 65, B + 1)
    sets = [_rand(rng, n) for n in nts + nqs]
    pairs = [(len(nts) + a, b) for a in range(len(nqs)) for b in range(len(nts))]
    for mutual in (0, 1):
        _check(solver, sets, pairs, mutual=mutual)
    nt = 7 * S + 40
    assert nt % S and nt // S >= 3
    q, t = _rand(rng, 65), _rand(rng, nt)
    t[[5, S + 1, 3 * S, nt - 1]] = q[7]           # the same neighbour in four splits: the lowest index wins, then the next
    got = _check(solver, [q, t])
    assert (got["best"][7], got["second"][7], got["dist1"][7], got["dist2"][7]) == (5, S + 1, 0, 0)
    _check(solver, [q, t], mutual=1)


# ------------------------------------------------------------------------------------------------------------------ 2: ties
@pytest.mark.parametrize("width", [32, 64])
def test_ties(solver, hb, width):
    T, S = hb.MATCH_TILE, hb.MATCH_MIN_SPLIT
    rng = np.random.default_rng(2)
    nt = 6 * S + 17
    base = _rand(rng, 5, width)
    # five distinct descriptors, repeated: the copies of one descriptor fall into different tiles and different splits
    t = base[np.arange(nt) % 5]
    t = t[rng.permutation(nt)]
    q = np.concatenate([base, base ^ np.uint8(1), ~base[:1]])      # exact copies, one bit off, a descriptor's complement
    got = _check(solver, [q, t], ratio=1.0)
    for i in range(5):
        where = np.nonzero((t == base[i]).all(axis=1))[0]
        assert where[-1] - where[0] > 4 * S                         # (in different splits indeed)
        for row, d in ((i, 0), (5 + i, width)):                     # base ^ 1 flips one bit per byte
            assert (got["best"][row], got["second"][row]) == (where[0], where[1])
            assert got["dist1"][row] == got["dist2"][row] == d and not got["good"][row]
    # the complement: 8 * width from its own copies, and every copy of it ties
    assert got["dist1"][10] < 8 * width
    comp = _check(solver, [~base[:1], np.repeat(base[:1], 2 * T + 1, axis=0)], ratio=0)
    assert (comp["best"][0], comp["second"][0], comp["dist1"][0], comp["dist2"][0]) == (0, 1, 8 * width, 8 * width)
    # all identical
    same = np.repeat(base[:1], 3 * S + 1, axis=0)
    got = _check(solver, [same[:70], same])
    assert (got["best"] == 0).all() and (got["second"] == 1).all() and (got["dist1"] == 0).all() and (got["dist2"] == 0).all()
    assert not got["good"].any() and got["n_good"][0] == 0
    got = _check(solver, [same], [(0, 0)], ratio=0, mutual=1)      # a set against itself: query 0 keeps train 0
    assert got["good"].tolist() == [True] + [False] * (len(same) - 1)


# ---------------------------------------------------------------------------------------------------- 3: split independence
def test_forced_split_counts_agree(hb):
    """BA_DEBUG_MATCH_SPLITS (read when the handle is created) asks for 1, 2 and 5 splits: bit-equal outputs."""
    S = hb.MATCH_MIN_SPLIT
    rng = np.random.default_rng(3)
    q, t = _rand(rng, 130), _rand(rng, 5 * S - 9)                  # 10 tiles: 1 split of 10, 2 of 5, 5 of 2
    t[[3, S + 3, 2 * S + 3, 3 * S + 3, 4 * S + 3]] = q[100]
    ref = M.match_descriptors([q, t], mutual=1)
    assert (ref["best"][100], ref["second"][100]) == (3, S + 3)
    old = os.environ.get("BA_DEBUG_MATCH_SPLITS")
    try:
        for n in (1, 2, 5):
            os.environ["BA_DEBUG_MATCH_SPLITS"] = str(n)
            with hb.Solver(0) as s:
                M.assert_equal(s.match_descriptors([q, t], mutual=1), ref)
    finally:
        if old is None:
            os.environ.pop("BA_DEBUG_MATCH_SPLITS", None)
        else:
            os.environ["BA_DEBUG_MATCH_SPLITS"] = old


def test_pair_alone_equals_pair_in_batch(solver, hb):
    S = hb.MATCH_MIN_SPLIT
    rng = np.random.default_rng(4)
    sets = [_rand(rng, 70), _rand(rng, 3 * S + 5), _rand(rng, 0), _rand(rng, 300)]
    sets[1][[2, 2 * S + 2]] = sets[0][9]
    pairs = [(0, 1), (1, 0), (2, 1), (0, 2), (3, 3), (1, 3), (3, 1), (0, 3), (1, 1)]     # empty queries, empty train, self-matches
    for mutual in (0, 1):
        batch = _check(solver, sets, pairs, mutual=mutual)
        for p, (a, b) in enumerate(pairs):
            alone = solver.match_descriptors([sets[a], sets[b]] if a != b else [sets[a]], [(0, 1)] if a != b else [(0, 0)], mutual=mutual)
            lo, hi = batch["row_off"][p], batch["row_off"][p + 1]
            assert hi - lo == len(sets[a]) == alone["row_off"][1]
            for k in ("best", "second", "dist1", "dist2", "good"):
                assert np.array_equal(alone[k], batch[k][lo:hi]), (p, k)
            assert alone["n_good"][0] == batch["n_good"][p]


# ---------------------------------------------------------------------------------------------------------------- 4: widths
@pytest.mark.parametrize("width", [8, 16, 24, 32, 40, 64])
def test_widths(solver, hb, width):
    rng = np.random.default_rng(5 + width)
    q, t = _rand(rng, 130, width), _rand(rng, hb.MATCH_TILE + 1, width)
    t[hb.MATCH_TILE] = q[129] ^ np.uint8(0x80)                     # a near neighbour in the last, one-row tile
    got = _check(solver, [q, t], mutual=1)
    assert got["best"][129] == hb.MATCH_TILE and got["dist1"][129] == width


# --------------------------------------------------------------------------------------------------------- 5: largest index
def test_largest_index(solver, hb):
    n = hb.MATCH_MAX_SET
    rng = np.random.default_rng(6)
    t = _rand(rng, n, 8)
    q = _rand(rng, 3, 8)
    t[n - 1] = q[1]
    t[5] = q[1]
    got = _check(solver, [q, t], ratio=0)
    assert (got["best"][1], got["second"][1], got["dist1"][1], got["dist2"][1]) == (5, n - 1, 0, 0)
    with pytest.raises(hb.BAHipError, match="set_off"):
        solver.match_descriptors([q, np.concatenate([t, t[:1]])])
    _check(solver, [q, t[:9]])                                     # the handle works afterwards


# --------------------------------------------------------------------------------------------------------------- 6: options
def test_options(solver):
    rng = np.random.default_rng(7)
    a = _rand(rng, 200)
    b = a[rng.permutation(200)][:150].copy()
    flips = rng.integers(0, 60, 150)
    for r in range(150):
        for bit in rng.choice(256, flips[r], replace=False):
            b[r, bit // 8] ^= np.uint8(1 << (bit % 8))
    b[0] = a[3]
    b[1] = a[3]                                                    # two queries at distance 0 from one train row
    b[2] = a[4]                                                    # distance 0: max_distance = 0 keeps something
    counts = set()
    for ratio in (0.75, 1.0, 0):
        for max_distance in (-1, 0, 40):
            for mutual in (0, 1):
                got = _check(solver, [b, a, a[:0]], [(0, 1), (1, 0), (0, 2)], ratio=ratio, max_distance=max_distance, mutual=mutual)
                ro = got["row_off"]
                assert [int(got["good"][ro[p]:ro[p + 1]].sum()) for p in range(3)] == got["n_good"].tolist()
                counts.add((ratio, max_distance, mutual, int(got["n_good"][0])))
                if mutual:
                    assert got["best"][0] == got["best"][1] == 3 and got["dist1"][0] == got["dist1"][1] == 0
                    assert not got["good"][1]                      # the lower query keeps the shared train row
                    assert got["good"][0] == (ratio <= 0 or got["dist2"][0] > 0)
    assert len({c[3] for c in counts}) >= 4                        # (the options do change the outcome on this data)


# --------------------------------------------------------------------------------------------------------- 7: planted scene
def _planted_scene(seed=0):
    rng = np.random.default_rng(seed)
    a = _rand(rng, 600)
    perm = rng.permutation(600)
    b = a[perm].copy()
    for r in range(600):
        for bit in rng.choice(256, rng.integers(0, 21), replace=False):
            b[r, bit // 8] ^= np.uint8(1 << (bit % 8))
    return a, np.concatenate([b, _rand(rng, 200)]), np.argsort(perm)


def test_planted_scene(solver):
    a, b, partner = _planted_scene()
    ref = M.match_pair(a, b)
    assert ref["good"].all() and np.array_equal(ref["best"], partner)      # a property of the data, on the yardstick first
    got = _check(solver, [a, b])
    assert got["good"].all() and np.array_equal(got["best"], partner) and got["n_good"][0] == 600
    back = _check(solver, [b, a], mutual=1)
    assert back["good"][:600].all() and np.array_equal(back["best"][:600], np.argsort(partner))


# --------------------------------------------------------------------------------------------------------------- 8: refusals
def _raw(solver, hb, width, set_off, desc, pq, pt, opts=None, n_sets=None, n_pairs=None):
    i64, i32, u8 = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)

    def ptr(a, t):
        return None if a is None else a.ctypes.data_as(t)
    o = solver.match_options(**(opts or {}))
    rows = np.zeros(1 << 12, dtype=np.int32)
    return solver._lib.ba_match_descriptors(solver._h, width, len(set_off) - 1 if n_sets is None else n_sets, ptr(set_off, i64), ptr(desc, u8),
                                            (0 if pq is None else len(pq)) if n_pairs is None else n_pairs, ptr(pq, i32), ptr(pt, i32),
                                            C.byref(o), None, ptr(rows, i32), None, None, None, None, None)


def test_refusals(solver, hb):
    rng = np.random.default_rng(8)
    desc = _rand(rng, 10)
    off = np.array([0, 4, 10], dtype=np.int64)
    pq, pt = np.array([0], dtype=np.int32), np.array([1], dtype=np.int32)
    big = np.zeros(65537, dtype=np.int64)
    many = np.zeros(65536, dtype=np.int32)
    cases = [
        ("desc_bytes", dict(width=12)), ("desc_bytes", dict(width=0)), ("desc_bytes", dict(width=72)),
        ("n_sets", dict(set_off=big, desc=None)), ("n_sets", dict(n_sets=-1)),
        ("n_pairs", dict(pq=many, pt=many)), ("n_pairs", dict(n_pairs=-1)),
        ("ratio", dict(opts=dict(ratio=float("nan")))), ("ratio", dict(opts=dict(ratio=float("inf")))),
        ("set_off", dict(set_off=None, n_sets=2)), ("set_off", dict(set_off=np.array([1, 4, 10], dtype=np.int64))),
        ("set_off", dict(set_off=np.array([0, 6, 4], dtype=np.int64))),
        ("set_off", dict(set_off=np.array([0, 4, 4 + hb.MATCH_MAX_SET + 1], dtype=np.int64))),
        ("desc", dict(desc=None)), ("pair_query", dict(pq=None, n_pairs=1)), ("pair_train", dict(pt=None)),
        ("pair_query", dict(pq=np.array([2], dtype=np.int32))), ("pair_query", dict(pq=np.array([-1], dtype=np.int32))),
        ("pair_train", dict(pt=np.array([2], dtype=np.int32))), ("pair_train", dict(pt=np.array([-1], dtype=np.int32))),
    ]
    for name, change in cases:
        kw = dict(width=32, set_off=off, desc=desc, pq=pq, pt=pt)
        kw.update(change)
        rc = _raw(solver, hb, **kw)
        msg = solver._lib.ba_last_error().decode()
        assert rc == -1 and msg.startswith("ba_match_descriptors: ") and name in msg.split(": ", 1)[1], (name, change.keys(), rc, msg)
        _check(solver, [desc[:4], desc[4:]])                       # the handle works afterwards
    assert solver._lib.ba_match_descriptors(None, 32, 0, None, None, 0, None, None, None, *([None] * 7)) == -1
    with pytest.raises(hb.BAHipError, match="pair_train"):
        solver.match_descriptors([desc[:4], desc[4:]], [(0, 2)])
    # no-ops with well-formed outputs
    out = _check(solver, [], [])
    assert out["row_off"].tolist() == [0]
    out = _check(solver, [desc[:0], desc[:0]], [(0, 1), (1, 0)])
    assert out["row_off"].tolist() == [0, 0, 0] and out["n_good"].tolist() == [0, 0]
    out = _check(solver, [desc, desc], [])
    assert out["row_off"].tolist() == [0] and out["best"].shape == (0,)


# ------------------------------------------------------------------------------------------------- 9: reuse and coexistence
def test_reuse_and_coexistence(hb):
    from bundle_adjustment_amd.synthetic import make_problem
    rng = np.random.default_rng(9)
    small, large = [_rand(rng, 20), _rand(rng, 30)], [_rand(rng, 700), _rand(rng, 900)]
    prob = make_problem(8, 400, 4, seed=0)
    kw = dict(max_iters=5, loss="huber")
    with hb.Solver(0) as s:
        for sets in (small, large, small):                         # the staging grows, then holds more than the call needs
            M.assert_equal(s.match_descriptors(sets, mutual=1), M.match_descriptors(sets, mutual=1))
        s.set_problem(prob)
        plain = s.solve(**kw)
        cams0, pts0 = s.get_params()
        s.set_problem(prob)
        M.assert_equal(s.match_descriptors(large), M.match_descriptors(large))
        mixed = s.solve(**kw)
        cams1, pts1 = s.get_params()
    assert np.array_equal(cams0, cams1) and np.array_equal(pts0, pts1)
    assert (plain["final_cost"], plain["iterations"]) == (mixed["final_cost"], mixed["iterations"])


# ----------------------------------------------------------------------------------------------------------------- 10: chain
class _KeyPoint:
    def __init__(self, pt):
        self.pt = (float(pt[0]), float(pt[1]))


def test_chain_match_then_pose(solver):
    """A two-view scene with a descriptor per 3-D point (view 2: shuffled, up to 20 bits flipped) and 30 % unrelated
    descriptors at random pixels in both views: BruteForceMatcher -> estimate_pose on the device, against estimate_pose on
    the yardstick's match list."""
    from bundle_adjustment_amd import estimate_pose, features
    n, extra = 300, 90
    p1, p2, _, _ = R.noisy_scene(n, seed=3)
    rng = np.random.default_rng(10)
    d1 = _rand(rng, n)
    perm = rng.permutation(n)
    d2 = d1[perm].copy()
    for r in range(n):
        for bit in rng.choice(256, rng.integers(0, 21), replace=False):
            d2[r, bit // 8] ^= np.uint8(1 << (bit % 8))
    des1, des2 = np.concatenate([d1, _rand(rng, extra)]), np.concatenate([d2, _rand(rng, extra)])
    junk = lambda: np.c_[rng.uniform(0, 1280, extra), rng.uniform(0, 720, extra)]      # noqa: E731
    kp1 = [_KeyPoint(p) for p in np.concatenate([p1, junk()])]
    kp2 = [_KeyPoint(p) for p in np.concatenate([p2[perm], junk()])]
    matches = features.BruteForceMatcher(solver=solver).match(des1, des2)
    ref = M.match_pair(des1, des2)
    keep = np.nonzero(ref["good"])[0]
    assert [(m.queryIdx, m.trainIdx, m.distance) for m in matches] == [(int(i), int(ref["best"][i]), float(ref["dist1"][i])) for i in keep]
    assert len(keep) >= n and np.array_equal(ref["best"][:n], np.argsort(perm))
    yard = [features.Match(i, ref["best"][i], ref["dist1"][i]) for i in keep]
    got = estimate_pose(matches, kp1, kp2, R.K_TEST, solver=solver, quiet=True)
    want = estimate_pose(yard, kp1, kp2, R.K_TEST, solver=solver, quiet=True)
    assert got[0] is not None and len(got[4]) >= 0.9 * n
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
