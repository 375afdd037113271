"""GPU: ba_match_l2 (exact L2 2-NN of uint8 descriptors on the int8 matrix cores, with the ratio test) against the numpy
yardstick of tests/match_l2_reference.py.  The arithmetic is integer: every comparison is exact equality on all seven outputs.

Shapes.  T = hip_backend.MATCH_L2_TILE train rows per LDS tile (two MFMA row blocks of 32), B = MATCH_L2_BLOCK queries per
workgroup (32 per wave), S = MATCH_L2_MIN_SPLIT the shortest train split, chunk = MATCH_L2_CHUNK[width] the train rows of a split
that share one 32-bit key range.  The library asks for ceil(8 n_cu / (2 wave rows of the call)) splits per pair, at
most nt / S of them and at most MATCH_MAX_SPLITS, in whole tiles; chunks are counted from the first row of a split.  Where a test
is about a split or chunk border it runs on a handle created under BA_DEBUG_MATCH_SPLITS, derives the split length by that rule
(_plan) and asserts that its rows lie where it says."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

from tests import match_l2_reference as L
from tests import match_reference as M

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


def _near(rng, n, width=32, spread=24):
    """Rows close to one another (a common centre plus small offsets): many near ties, distances far below the random level."""
    centre = rng.integers(40, 216, (1, width))
    return (centre + rng.integers(-spread, spread + 1, (n, width))).astype(np.uint8)


def _plan(hb, nt, want):
    """DESIGN.md 4x's split rule for nt train rows when `want` splits are asked for -> (split_len, n_splits)."""
    T, S = hb.MATCH_L2_TILE, hb.MATCH_L2_MIN_SPLIT
    tiles = -(-nt // T)
    n = max(1, min(want, hb.MATCH_MAX_SPLITS, tiles // (S // T)))
    split_len = -(-tiles // n) * T
    return split_len, -(-nt // split_len)


@contextlib.contextmanager
def _forced(hb, n):
    """A handle that asks for n splits per entry (BA_DEBUG_MATCH_SPLITS is read when the handle is created)."""
    old = os.environ.get("BA_DEBUG_MATCH_SPLITS")
    os.environ["BA_DEBUG_MATCH_SPLITS"] = str(n)
    try:
        s = hb.Solver(0)
    finally:
        if old is None:
            os.environ.pop("BA_DEBUG_MATCH_SPLITS", None)
        else:
            os.environ["BA_DEBUG_MATCH_SPLITS"] = old
    with s:
        yield s


def _check(solver, sets, pairs=None, **opts):
    got = solver.match_l2(sets, pairs, **opts)
    L.assert_equal(got, L.match_l2(sets, pairs, **opts))
    return got


# ----------------------------------------------------------------------------------- 1: edges of tile, chunk, block and split
def test_edges_of_tile_chunk_block_and_split(solver, hb):
    """nq and nt each take every size of the list, 32 bytes wide: the small sizes as a full grid, every size as nt against
    queries of 33 and B + 1 rows and as nq against train sets of 33, T + 1 and chunk + 1 rows; all pairs of ONE call (a pair's
    rows do not depend on the others: test_pair_alone_equals_pair_in_batch), the sets drawn once.  The library's own plan cuts
    a train set of about a chunk into splits shorter than a chunk, so the same call runs again on a handle forced to ONE split
    per entry: there a set of chunk - 1 rows ends inside its first chunk, one of chunk rows ends with it, and one of chunk + 1
    rows folds a full chunk and then a second chunk of one row."""
    T, B, S, chunk = hb.MATCH_L2_TILE, hb.MATCH_L2_BLOCK, hb.MATCH_L2_MIN_SPLIT, hb.MATCH_L2_CHUNK[32]
    sizes = sorted({0, 1, 2, 31, 32, 33, T - 1, T, T + 1, chunk - 1, chunk, chunk + 1, S - 1, S + 1, B - 1, B + 1})
    small = [n for n in sizes if n <= 33]
    rng = np.random.default_rng(1)
    sets = [_near(rng, n) for n in sizes]
    at = {n: k for k, n in enumerate(sizes)}
    pairs = {(at[a], at[b]) for a in small for b in small}
    pairs |= {(at[a], at[n]) for n in sizes for a in (33, B + 1)} | {(at[n], at[b]) for n in sizes for b in (33, T + 1, chunk + 1)}
    pairs = sorted(pairs)
    assert {a for a, _ in pairs} == {b for _, b in pairs} == set(range(len(sizes)))
    for mutual in (0, 1):
        _check(solver, sets, pairs, mutual=mutual)
    for n in (chunk - 1, chunk, chunk + 1):
        split_len, n_splits = _plan(hb, n, 1)
        assert n_splits == 1 and split_len >= n and (n - 1) // chunk == (n > chunk)      # one split; its last row in chunk 0, 0, 1
    with _forced(hb, 1) as one:
        for mutual in (0, 1):
            _check(one, sets, pairs, mutual=mutual)


def test_splits_with_a_short_last_one(solver, hb):
    """Two wave rows of queries against 7 S + 40 train rows: the library's own wish is >= 4 splits on any device, the last one
    short; the same neighbour in four splits -- the lowest index wins, then the next."""
    S = hb.MATCH_L2_MIN_SPLIT
    rng = np.random.default_rng(11)
    nt = 7 * S + 40
    q, t = _rand(rng, 65), _rand(rng, nt)
    t[[5, S + 1, 3 * S, nt - 1]] = q[7]
    got = _check(solver, [q, t])
    assert (got["best"][7], got["second"][7], got["dist1"][7], got["dist2"][7]) == (5, S + 1, 0, 0)
    _check(solver, [q, t], mutual=1)


# ---------------------------------------------------------------------------------------------------------------- 2: widths
@pytest.mark.parametrize("width", [32, 64, 96, 128, 160, 192, 224, 256])
def test_widths(solver, hb, width):
    assert width in hb.MATCH_L2_DESC_BYTES
    rng = np.random.default_rng(5 + width)
    q, t = _rand(rng, 300, width), _rand(rng, 517, width)
    t[516] = q[299]
    t[516, width - 1] ^= np.uint8(3)                                # a near neighbour in the last, short tile, last byte
    got = _check(solver, [q, t], mutual=1)
    assert got["best"][299] == 516 and 1 <= got["dist1"][299] <= 9
    _check(solver, [_near(rng, 300, width), _near(rng, 517, width)], ratio=0.9)


# -------------------------------------------------------------------------------------------------------------- 3: extremes
def test_extremes(solver):
    W = 256
    z, f = np.zeros((40, W), dtype=np.uint8), np.full((70, W), 255, dtype=np.uint8)
    top = 256 * 255 * 255
    assert top == 16646400
    for a, b in ((z, f), (f, z)):
        got = _check(solver, [a, b], ratio=0)
        assert (got["dist1"] == top).all() and (got["dist2"] == top).all() and (got["best"] == 0).all() and (got["second"] == 1).all()
    # the sign boundary of the shift
    lo, hi = np.full((35, W), 127, dtype=np.uint8), np.full((66, W), 128, dtype=np.uint8)
    for a, b in ((lo, hi), (hi, lo), (lo, lo), (hi, hi)):
        got = _check(solver, [a, b], ratio=0)
        assert (got["dist1"] == (0 if a is b else W)).all()
    # one query whose nearest and second nearest are at the extremes: every train row is as far as a row can be, but two
    rng = np.random.default_rng(3)
    q = np.zeros((1, W), dtype=np.uint8)
    t = np.full((200, W), 255, dtype=np.uint8)
    t[150, 0] = 254
    t[70, :2] = 254
    got = _check(solver, [q, t], ratio=0)
    assert (got["best"][0], got["second"][0]) == (70, 150) and (got["dist1"][0], got["dist2"][0]) == (top - 1018, top - 509)   # 255^2 - 254^2 = 509
    # ... and the other end: nearest at 0 and 1, everything else at the top
    t[150], t[70] = 0, 0
    t[70, 9] = 1
    got = _check(solver, [q, t], ratio=0.8)
    assert (got["best"][0], got["second"][0], got["dist1"][0], got["dist2"][0], got["good"][0]) == (150, 70, 0, 1, True)
    mix = np.concatenate([z[:3], f[:3], lo[:3], hi[:3], _rand(rng, 20, W)])
    _check(solver, [mix, mix[::-1].copy()], mutual=1, ratio=0)


# ------------------------------------------------------------------------------------------------------------------ 4: ties
def _place(hb, j, split_len, chunk):
    """(split, chunk within the split, tile within the split) of train row j."""
    return j // split_len, (j % split_len) // chunk, (j % split_len) // hb.MATCH_L2_TILE


@pytest.mark.parametrize("want", [1, 2, 5])
def test_ties_across_borders(hb, want):
    """Duplicate train rows, the lower index wins: across a tile border, a chunk border, a split border, in the two lane halves
    (j and j + 4 of one 32-row block) and far apart, on a handle forced to `want` splits.  4 chunk + 17 rows at 32 bytes are 65
    tiles: one split of all rows (chunk ends at every multiple of chunk), two of 33 tiles (longer than a chunk: split 1 has chunk
    ends of its own, counted from its first row) or five of 13 tiles (shorter than a chunk: a chunk ends only with its split)."""
    T, chunk = hb.MATCH_L2_TILE, hb.MATCH_L2_CHUNK[32]
    nt = 4 * chunk + 17
    split_len, n_splits = _plan(hb, nt, want)
    assert (split_len, n_splits) == {1: (65 * T, 1), 2: (33 * T, 2), 5: (13 * T, 5)}[want]
    at = lambda j: _place(hb, j, split_len, chunk)      # noqa: E731
    mid = nt // 2 // 32 * 32
    spots = [(T - 1, T), (3, 7), (mid + 5, mid + 9), (10, nt - 1)]
    assert at(T - 1)[:2] == at(T)[:2] and at(T - 1)[2] + 1 == at(T)[2]                         # a tile border inside one chunk
    assert all(at(a) == at(b) and a // 32 == b // 32 and (a % 8) // 4 != (b % 8) // 4 for a, b in spots[1:3])     # the two lane halves
    if split_len > chunk:                               # chunk borders inside a split: the first, and the last one of the last split
        last0 = (n_splits - 1) * split_len
        c = last0 + (nt - 1 - last0) // chunk * chunk
        for a, b in ((chunk - 1, chunk), (c - 1, c)):
            assert at(a)[0] == at(b)[0] and at(a)[1] + 1 == at(b)[1] and last0 < c
            spots.append((a, b))
        spots.append((chunk - 2, c + 1))                # and in different chunks, not adjacent
    if n_splits > 1:                                    # split borders: the first and the last
        for a, b in sorted({(split_len - 1, split_len), ((n_splits - 1) * split_len - 1, (n_splits - 1) * split_len)}):
            assert at(a)[0] + 1 == at(b)[0] and at(b)[1:] == (0, 0)
            spots.append((a, b))
    assert len({j for ab in spots for j in ab}) == 2 * len(spots) and max(b for _, b in spots) < nt
    rng = np.random.default_rng(2)
    t, q = _rand(rng, nt), _rand(rng, len(spots))
    for i, (a, b) in enumerate(spots):
        t[a] = q[i]
        t[b] = q[i]
    t2 = t.copy()                                       # near-duplicates at distance 1 tie the same way
    for a, b in spots:
        t2[a, 0] ^= np.uint8(1)
        t2[b, 0] ^= np.uint8(1)
    with _forced(hb, want) as s:
        for train, d in ((t, 0), (t2, 1)):
            for mutual in (0, 1):
                got = _check(s, [q, train], ratio=1.0, mutual=mutual)
                assert [(int(a), int(b)) for a, b in zip(got["best"], got["second"])] == spots
                assert got["dist1"].tolist() == [d] * len(spots) == got["dist2"].tolist() and not got["good"].any()


def test_ties(solver, hb):
    T, S = hb.MATCH_L2_TILE, hb.MATCH_L2_MIN_SPLIT
    rng = np.random.default_rng(2)
    t = _rand(rng, 1)
    # all identical
    same = np.repeat(t[:1], S + T + 1, axis=0)
    got = _check(solver, [same[:70], same])
    assert (got["best"] == 0).all() and (got["second"] == 1).all() and (got["dist1"] == 0).all() and (got["dist2"] == 0).all()
    assert not got["good"].any() and got["n_good"][0] == 0
    # a set against itself: best = i at distance 0; on duplicated rows dist2 = 0 and the ratio never passes
    own = _rand(rng, 2 * S + 9)
    own[S + 3] = own[4]
    got = _check(solver, [own], [(0, 0)], ratio=0.8, mutual=1)
    assert (got["dist1"] == 0).all() and got["best"][4] == 4 and got["best"][S + 3] == 4
    assert np.array_equal(np.delete(got["best"], S + 3), np.delete(np.arange(len(own)), S + 3))
    assert not got["good"][4] and not got["good"][S + 3] and got["good"].sum() == len(own) - 2


# ---------------------------------------------------------------------------------------------------- 5: geometry independence
def test_forced_split_counts_agree(hb):
    """BA_DEBUG_MATCH_SPLITS (read when the handle is created) asks for 1, 2 and 5 splits: bit-equal outputs."""
    S = hb.MATCH_L2_MIN_SPLIT
    rng = np.random.default_rng(3)
    q, t = _near(rng, 130), _near(rng, 5 * S - 9)                  # 20 tiles: 1 split of 20, 2 of 10, 5 of 4
    t[[3, S + 3, 2 * S + 3, 3 * S + 3, 4 * S + 3]] = q[100]
    ref = L.match_l2([q, t], mutual=1)
    assert (ref["best"][100], ref["second"][100]) == (3, S + 3)
    assert [_plan(hb, len(t), n) for n in (1, 2, 5)] == [(20 * hb.MATCH_L2_TILE, 1), (10 * hb.MATCH_L2_TILE, 2), (4 * hb.MATCH_L2_TILE, 5)]
    for n in (1, 2, 5):
        with _forced(hb, n) as s:
            L.assert_equal(s.match_l2([q, t], mutual=1), ref)


def test_pair_alone_equals_pair_in_batch(solver, hb):
    S = hb.MATCH_L2_MIN_SPLIT
    rng = np.random.default_rng(4)
    sets = [_rand(rng, 70), _rand(rng, 3 * S + 5), _rand(rng, 0), _rand(rng, 300)]
    sets[1][[2, 2 * S + 2]] = sets[0][9]
    pairs = [(0, 1), (1, 0), (2, 1), (0, 2), (3, 3), (1, 3), (3, 1), (0, 3), (1, 1)]     # empty queries, empty train, self-matches
    for mutual in (0, 1):
        batch = _check(solver, sets, pairs, mutual=mutual)
        for p, (a, b) in enumerate(pairs):
            alone = solver.match_l2([sets[a], sets[b]] if a != b else [sets[a]], [(0, 1)] if a != b else [(0, 0)], mutual=mutual)
            lo, hi = batch["row_off"][p], batch["row_off"][p + 1]
            assert hi - lo == len(sets[a]) == alone["row_off"][1]
            for k in ("best", "second", "dist1", "dist2", "good"):
                assert np.array_equal(alone[k], batch[k][lo:hi]), (p, k)
            assert alone["n_good"][0] == batch["n_good"][p]


# --------------------------------------------------------------------------------------------------------- 6: largest index
def test_largest_index(solver, hb):
    """2^20 train rows of 32 bytes and three queries whose partners sit at indices 0, 2^20 - 2 and 2^20 - 1 (one of them one
    step away, with a runner-up at index 7); the yardstick's distances and stable order over all rows, three queries only."""
    n = hb.MATCH_MAX_SET
    rng = np.random.default_rng(6)
    t = _rand(rng, n)
    q = _rand(rng, 3)
    t[0], t[n - 2], t[n - 1] = q[0], q[1], q[2]
    t[n - 1, 0] ^= np.uint8(1)
    t[7] = q[2]
    t[7, :2] ^= np.uint8(1)
    got = solver.match_l2([q, t], ratio=0)
    d = L.distances(q, t)
    order = np.argsort(d, axis=1, kind="stable")[:, :2]
    assert np.array_equal(got["best"], order[:, 0].astype(np.int32)) and np.array_equal(got["second"], order[:, 1].astype(np.int32))
    assert np.array_equal(got["dist1"], d[np.arange(3), order[:, 0]]) and np.array_equal(got["dist2"], d[np.arange(3), order[:, 1]])
    assert got["best"].tolist() == [0, n - 2, n - 1] and got["dist1"].tolist() == [0, 0, 1] and got["second"][2] == 7 and got["dist2"][2] == 2
    assert got["good"].all() and got["n_good"][0] == 3 and got["row_off"].tolist() == [0, 3]
    with pytest.raises(hb.BAHipError, match="set_off"):
        solver.match_l2([q, np.concatenate([t, t[:1]])])
    _check(solver, [q, t[:9]])                                     # the handle works afterwards


# --------------------------------------------------------------------------------------------------------------- 7: options
def test_ratio_border(solver):
    """dist1 = 9, dist2 = 16, ratio = 0.75: 9 < 0.5625 * 16 = 9.0 is false, exactly on the border (0.75^2 and the product are
    exact in fp64); dist1 = 8 passes; ratio 0 passes both; a zero dist2 never passes."""
    q = np.zeros((3, 32), dtype=np.uint8)
    q[1, 5] = 200
    q[2, 7] = 90
    t = np.zeros((5, 32), dtype=np.uint8)
    t[0, 0] = 4                                                     # 16 from query 0
    t[1, 1] = 3                                                     # 9 from query 0
    t[2] = q[1]
    t[2, :2] = 2                                                    # 8 from query 1
    t[3] = q[1]
    t[3, 0] = 4                                                     # 16 from query 1
    t[4] = q[2]                                                     # 0 from query 2 ...
    ts = np.concatenate([t, q[2:3]])                                # ... and a duplicate of it: dist2 = 0
    for ratio, want in ((0.75, [False, True, False]), (0.0, [True, True, True]), (0.8, [True, True, False])):
        got = _check(solver, [q, ts], ratio=ratio)
        assert got["dist1"].tolist() == [9, 8, 0] and got["dist2"].tolist() == [16, 16, 0] and got["good"].tolist() == want


def test_options(solver):
    rng = np.random.default_rng(7)
    a = _rand(rng, 200)
    b = a[rng.permutation(200)][:150].copy()
    b = (b.astype(np.int64) + rng.integers(-6, 7, b.shape) * (rng.random((150, 1)) < 0.7)).clip(0, 255).astype(np.uint8)
    b[0] = a[3]
    b[1] = a[3]                                                    # two queries at distance 0 from one train row
    counts = set()
    for ratio in (0.8, 1.0, 0):
        for max_distance in (-1, 0, 300):
            for mutual in (0, 1):
                got = _check(solver, [b, a, a[:0]], [(0, 1), (1, 0), (0, 2)], ratio=ratio, max_distance=max_distance, mutual=mutual)
                ro = got["row_off"]
                assert [int(got["good"][ro[p]:ro[p + 1]].sum()) for p in range(3)] == got["n_good"].tolist()
                counts.add((ratio, max_distance, mutual, int(got["n_good"][0])))
                if mutual:
                    assert got["best"][0] == got["best"][1] == 3 and got["dist1"][0] == got["dist1"][1] == 0
                    assert got["good"][0] and not got["good"][1]    # the lower query keeps the shared train row
    assert len({c[3] for c in counts}) >= 4                        # (the options do change the outcome on this data)


# --------------------------------------------------------------------------------------------------------- 8: planted scene
def _sift_like(rng, n, width=128):
    """Non-negative, heavy-tailed rows, L2-normalised and clipped at 0.2 (SIFT's own clip)."""
    x = rng.exponential(1.0, (n, width)) ** 2
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return np.minimum(x, 0.2)


def _planted_scene(seed=0, n=1500, sigma=0.04):
    from bundle_adjustment_amd import quantize_descriptors
    rng = np.random.default_rng(seed)
    x = _sift_like(rng, n)
    perm = rng.permutation(2 * n)
    y = np.concatenate([x + rng.normal(0.0, sigma, x.shape), _sift_like(rng, n)])[perm]
    partner = np.argsort(perm)[:n]                                  # row i of the first image is row partner[i] of the second
    return quantize_descriptors(x), quantize_descriptors(np.maximum(y, 0.0)), partner


def test_planted_scene(solver):
    a, b, partner = _planted_scene()
    assert a.dtype == np.uint8 and a.shape == (1500, 128) and b.shape == (3000, 128)
    ref = L.match_pair(a, b, ratio=0.8)
    found = (ref["best"] == partner) & ref["good"]
    print("planted partners that are best and good on the yardstick:", found.mean())
    assert found.mean() >= 0.99                                     # a property of the data, on the yardstick alone
    got = solver.match_l2([a, b], ratio=0.8)
    ref_all = L.match_l2([a, b], ratio=0.8)
    L.assert_equal(got, ref_all)


# -------------------------------------------------------------------------------------------------------------- 9: refusals
def _raw(solver, width, set_off, desc, pq, pt, opts=None, n_sets=None, n_pairs=None):
    i64, i32, u8 = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)

    def ptr(a, t):
        return None if a is None else a.ctypes.data_as(t)
    o = solver.match_options(**(opts or {}))
    rows = np.zeros(1 << 12, dtype=np.int32)
    return solver._lib.ba_match_l2(solver._h, width, len(set_off) - 1 if n_sets is None else n_sets, ptr(set_off, i64), ptr(desc, u8),
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
        ("desc_bytes", dict(width=48)), ("desc_bytes", dict(width=0)), ("desc_bytes", dict(width=288)), ("desc_bytes", dict(width=8)),
        ("desc_bytes", dict(width=-32)),
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
        rc = _raw(solver, **kw)
        msg = solver._lib.ba_last_error().decode()
        assert rc == -1 and msg.startswith("ba_match_l2: ") and name in msg.split(": ", 1)[1], (name, change.keys(), rc, msg)
        _check(solver, [desc[:4], desc[4:]])                       # the handle works afterwards
    assert solver._lib.ba_match_l2(None, 32, 0, None, None, 0, None, None, None, *([None] * 7)) == -1
    with pytest.raises(hb.BAHipError, match="pair_train"):
        solver.match_l2([desc[:4], desc[4:]], [(0, 2)])
    with pytest.raises(hb.BAHipError, match="desc_bytes"):
        solver.match_l2([_rand(rng, 4, 40), _rand(rng, 4, 40)])
    # no-ops with well-formed outputs
    out = _check(solver, [], [])
    assert out["row_off"].tolist() == [0]
    out = _check(solver, [desc[:0], desc[:0]], [(0, 1), (1, 0)])
    assert out["row_off"].tolist() == [0, 0, 0] and out["n_good"].tolist() == [0, 0]
    out = _check(solver, [desc, desc], [])
    assert out["row_off"].tolist() == [0] and out["best"].shape == (0,)
    out = _check(solver, [desc, desc[:0], desc[:1]], [(0, 1), (0, 2)], ratio=0)
    assert out["best"].tolist() == [-1] * 10 + [0] * 10 and out["second"].tolist() == [-1] * 20 and out["n_good"].tolist() == [0, 10]


# ------------------------------------------------------------------------------------------------ 10: reuse and coexistence
def test_reuse_and_coexistence(hb):
    from bundle_adjustment_amd.synthetic import make_problem
    rng = np.random.default_rng(9)
    small, large = [_rand(rng, 20), _rand(rng, 30)], [_rand(rng, 700), _rand(rng, 900)]
    binary = [_rand(rng, 300), _rand(rng, 400)]
    prob = make_problem(8, 400, 4, seed=0)
    kw = dict(max_iters=5, loss="huber")
    ref = {id(s): L.match_l2(s, mutual=1) for s in (small, large)}
    ref_bin = M.match_descriptors(binary, mutual=1)
    with hb.Solver(0) as s:
        allocs = []
        for _ in range(3):                                         # alternating calls, each equal to its yardstick
            for sets in (small, large, small):
                L.assert_equal(s.match_l2(sets, mutual=1), ref[id(sets)])
                M.assert_equal(s.match_descriptors(binary, mutual=1), ref_bin)
            allocs.append(s.stats()["scratch_allocs"])
        assert allocs[1] == allocs[2], allocs                      # constant from the second round on
        s.set_problem(prob)
        plain = s.solve(**kw)
        cams0, pts0 = s.get_params()
        s.set_problem(prob)
        L.assert_equal(s.match_l2(large, mutual=1), ref[id(large)])
        mixed = s.solve(**kw)
        cams1, pts1 = s.get_params()
    assert np.array_equal(cams0, cams1) and np.array_equal(pts0, pts1)
    assert (plain["final_cost"], plain["iterations"]) == (mixed["final_cost"], mixed["iterations"])


# ----------------------------------------------------------------------------------------------------------------- 11: chain
def test_chain_match_then_fundamental(solver, hb):
    """Quantised planted descriptors on the points of a two-view scene, 30 % unrelated keypoints in both views: match_l2 ->
    pose_estimator.fundamental on the matched keypoints, status OK -- the uncalibrated path end to end."""
    from bundle_adjustment_amd import features, pose_estimator, quantize_descriptors
    from tests import relpose_reference as R
    n, extra = 300, 90
    p1, p2, _, _ = R.noisy_scene(n, seed=3)
    rng = np.random.default_rng(10)
    x = _sift_like(rng, n)
    perm = rng.permutation(n)
    d1 = quantize_descriptors(np.concatenate([x, _sift_like(rng, extra)]))
    d2 = quantize_descriptors(np.maximum(np.concatenate([(x + rng.normal(0.0, 0.04, x.shape))[perm], _sift_like(rng, extra)]), 0.0))
    kp1 = np.concatenate([p1, np.c_[rng.uniform(0, 1280, extra), rng.uniform(0, 720, extra)]])
    kp2 = np.concatenate([p2[perm], np.c_[rng.uniform(0, 1280, extra), rng.uniform(0, 720, extra)]])
    qi, ti, sq = features.match_l2(d1, d2, solver=solver, ratio=0.8)
    ref = L.match_pair(d1, d2, ratio=0.8)
    keep = np.nonzero(ref["good"])[0]
    assert np.array_equal(qi, keep) and np.array_equal(ti, ref["best"][keep]) and np.array_equal(sq, ref["dist1"][keep])
    inv = np.argsort(perm)
    assert (ti[qi < n] == inv[qi[qi < n]]).mean() >= 0.99 and (qi < n).sum() >= 0.95 * n
    ms = features.BruteForceMatcher(ratio=0.8, solver=solver, norm="l2").match(d1, d2)
    assert [(m.queryIdx, m.trainIdx, m.distance) for m in ms] == [(int(i), int(ref["best"][i]), float(np.sqrt(float(ref["dist1"][i])))) for i in keep]
    out = pose_estimator.fundamental(kp1[qi], kp2[ti], solver=solver)
    assert out["status"] == hb.FUNDAMENTAL_STATUS["ok"], out["status"]
    assert out["n_inliers"] >= 0.9 * (qi < n).sum()
