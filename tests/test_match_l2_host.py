"""CPU: the yardstick of the ba_match_l2 tests (tests/match_l2_reference.py) against a triple Python loop, quantize_descriptors,
and the surface of ba_match_l2 that needs no device: the symbol, the constants, the host side of features.py, and the refusals
the library decides before any device call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import match_l2_reference as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from bundle_adjustment_amd import hip_backend
    return hip_backend.load_library()


def _loops(q, t, ratio=0.75, max_distance=-1, mutual=0):
    """The header's definition by three Python loops: (d, j) order by explicit comparison of tuples."""
    nq, nt = len(q), len(t)
    d = [[sum((int(a) - int(b)) ** 2 for a, b in zip(q[i], t[j])) for j in range(nt)] for i in range(nq)]
    out = dict(best=[], second=[], dist1=[], dist2=[], good=[])
    for i in range(nq):
        keys = sorted((d[i][j], j) for j in range(nt))
        b, s = (keys[0] if nt >= 1 else (-1, -1)), (keys[1] if nt >= 2 else (-1, -1))
        g = b[1] >= 0
        if ratio > 0:
            g = g and s[1] >= 0 and float(b[0]) < (ratio * ratio) * float(s[0])
        if max_distance >= 0:
            g = g and b[0] <= max_distance
        if mutual and g:
            g = min((d[k][b[1]], k) for k in range(nq))[1] == i
        for k, v in zip(("best", "second", "dist1", "dist2", "good"), (b[1], s[1], b[0], s[0], g)):
            out[k].append(v)
    return out


@pytest.mark.parametrize("mutual", [0, 1])
@pytest.mark.parametrize("ratio", [0.75, 1.0, 0.0])
def test_yardstick_against_loops(ratio, mutual):
    rng = np.random.default_rng(3)
    cases = 0
    for nq in range(0, 8):
        for nt in range(0, 8):
            # few distinct rows with few small entries: ties in d, duplicates among the train rows and among the queries
            pool = (rng.integers(0, 4, (3, 8)) * (rng.random((3, 8)) < 0.5)).astype(np.uint8)
            pool[2, 0] = 255                      # and one large byte: a square that an 8- or 16-bit product would lose
            q, t = pool[rng.integers(0, 3, nq)], pool[rng.integers(0, 3, nt)]
            if nq and nt > 2:
                q[0] = t[2]                       # a planted exact match that ties with every copy of it
            for max_distance in (-1, 0, 3):
                ref = L.match_pair(q, t, ratio=ratio, max_distance=max_distance, mutual=mutual)
                want = _loops(q, t, ratio, max_distance, mutual)
                for k, v in want.items():
                    assert ref[k].tolist() == v, (nq, nt, k)
                assert ref["n_good"] == sum(want["good"])
                cases += 1
    assert cases == 64 * 3
    q, t = rng.integers(0, 256, (9, 32), dtype=np.uint8), rng.integers(0, 256, (11, 32), dtype=np.uint8)
    ref, want = L.match_pair(q, t, ratio=ratio, mutual=mutual), _loops(q, t, ratio, -1, mutual)
    assert all(ref[k].tolist() == v for k, v in want.items())


def test_yardstick_edges_and_ratio_boundaries():
    z = np.zeros((1, 32), dtype=np.uint8)

    def row(*vals):
        r = np.zeros(32, dtype=np.uint8)
        r[:len(vals)] = vals
        return r
    r = L.match_pair(z, np.zeros((0, 32), dtype=np.uint8))
    assert (r["best"][0], r["second"][0], r["dist1"][0], r["dist2"][0], r["good"][0]) == (-1, -1, -1, -1, False)
    r = L.match_pair(z, z)
    assert (r["best"][0], r["second"][0], r["dist1"][0], r["dist2"][0], r["good"][0]) == (0, -1, 0, -1, False)
    assert L.match_pair(z, z, ratio=0)["good"][0]
    # d1 = 9, d2 = 16, ratio 0.75: 9 < 0.5625 * 16 = 9.0 is false; d1 = 8 is good
    r = L.match_pair(z, np.stack([row(4), row(3)]))
    assert (r["best"][0], r["second"][0], r["dist1"][0], r["dist2"][0], r["good"][0]) == (1, 0, 9, 16, False)
    r = L.match_pair(z, np.stack([row(4), row(2, 2)]))
    assert (r["dist1"][0], r["dist2"][0], r["good"][0]) == (8, 16, True)
    # ties go to the lower index; a zero dist2 never passes, whatever the ratio
    r = L.match_pair(z, np.stack([row(5), row(2), row(2)]), ratio=1.0)
    assert (r["best"][0], r["second"][0], r["dist1"][0], r["dist2"][0], r["good"][0]) == (1, 2, 4, 4, False)
    assert not L.match_pair(z, np.stack([z[0], z[0]]), ratio=100.0)["good"][0]
    # the top of the range at 256 bytes
    r = L.match_pair(np.zeros((1, 256), dtype=np.uint8), np.full((2, 256), 255, dtype=np.uint8), ratio=0)
    assert (r["dist1"][0], r["dist2"][0]) == (16646400, 16646400) and r["dist1"].dtype == np.int32
    # mutual: one train row the best of two queries at equal distance -- the lower query keeps it
    r = L.match_pair(np.stack([row(1), row(1)]), np.stack([row(0), row(40)]), mutual=1)
    assert r["best"].tolist() == [0, 0] and r["good"].tolist() == [True, False]
    out = L.match_l2([z, np.stack([row(4), row(2, 2)]), np.zeros((0, 32), dtype=np.uint8)], [(0, 1), (2, 1), (1, 0), (1, 2)])
    assert out["row_off"].tolist() == [0, 1, 1, 3, 5] and out["n_good"].tolist() == [1, 0, 0, 0]
    assert out["best"].tolist() == [1, 0, 0, -1, -1] and out["dist2"].tolist() == [16, -1, -1, -1, -1]
    empty = L.match_l2([], [])
    assert empty["row_off"].tolist() == [0] and empty["best"].shape == (0,) and empty["n_good"].shape == (0,)


def test_quantize_descriptors():
    from bundle_adjustment_amd import features, quantize_descriptors
    assert quantize_descriptors is features.quantize_descriptors
    x = np.array([[3.0, 4.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0], [1.0, 1.0, 1.0, 1.0], [0.0, 7.0, 0.0, 0.0]])
    got = quantize_descriptors(x)
    assert got.dtype == np.uint8 and got.shape == (4, 4)
    # 512 * 0.6 + 0.5 = 307.7 and 512 * 0.8 + 0.5 clip at 255; a zero row stays zero; 512 * 0.5 + 0.5 = 256.5 clips; 512 clips
    assert got.tolist() == [[255, 255, 0, 0], [0, 0, 0, 0], [255, 255, 255, 255], [0, 255, 0, 0]]
    # below the clip: 16 equal entries are 0.25 each -> floor(128.5) = 128; the rounding is floor(512 x + 0.5)
    assert quantize_descriptors(np.ones((1, 16))).tolist() == [[128] * 16]
    y = np.zeros((1, 128))
    y[0, :4] = [0.3, 0.1, 0.004, 0.0009]
    n = np.linalg.norm(y)
    assert quantize_descriptors(y)[0, :5].tolist() == [int(min(255, np.floor(512 * v / n + 0.5))) for v in (0.3, 0.1, 0.004, 0.0009, 0.0)]
    # root: L1-normalise, square root, then the same; (9, 16, 0, 0) -> sqrt(9/25, 16/25) = (0.6, 0.8), already of unit L2 norm
    r = quantize_descriptors(np.array([[9.0, 16.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.0]] + [[1.0] * 4]), root=True)
    assert r.tolist() == [[255, 255, 0, 0], [0, 0, 0, 0], [255, 255, 255, 255]]
    z = np.zeros((1, 64))
    z[0, :4] = [1.0, 4.0, 9.0, 50.0]
    want = np.sqrt(z / 64.0)
    want = np.floor(512 * want / np.linalg.norm(want) + 0.5).clip(0, 255).astype(np.uint8)
    assert np.array_equal(quantize_descriptors(z, root=True), want) and want[0, 0] == 64       # sqrt(1/64) = 0.125 of norm 1
    assert quantize_descriptors(np.zeros((0, 128))).shape == (0, 128)
    with pytest.raises(ValueError):
        quantize_descriptors(np.zeros(128))
    assert "NOT verified" in quantize_descriptors.__doc__


def test_symbol_and_constants(lib):
    from bundle_adjustment_amd import hip_backend as hb
    assert hasattr(lib, "ba_match_l2") and "ba_match_l2" in hb.SYMBOLS
    assert hb.SYMBOLS["ba_match_l2"] == hb.SYMBOLS["ba_match_descriptors"]                     # the same surface
    assert C.sizeof(hb.BAMatchOptions) == 16
    hdr = open(os.path.join(ROOT, "include", "ba_hip.h")).read()
    assert re.search(r"int ba_match_l2\(ba_handle\* h, int32_t desc_bytes, int32_t n_sets,", hdr)
    src = open(os.path.join(ROOT, "bundle_adjustment_amd", "csrc", "ba_match_l2.hpp")).read()
    consts = {k: int(v) for k, v in re.findall(r"constexpr int (ML_[A-Z_]+) = (\d+);", src)}
    assert (consts["ML_BLOCK"], consts["ML_TILE"], consts["ML_MIN_SPLIT"]) == (hb.MATCH_L2_BLOCK, hb.MATCH_L2_TILE, hb.MATCH_L2_MIN_SPLIT)
    assert hb.MATCH_L2_DESC_BYTES == tuple(range(32, 32 * consts["ML_MAX_W"] + 1, 32))
    assert hb.MATCH_L2_MIN_SPLIT % hb.MATCH_L2_TILE == 0 and hb.MATCH_L2_TILE % 32 == 0

    def idx_bits(w):                              # ml_idx_bits of the kernel: 2^n > 3 * 32 w * 2^14, 31 - n index bits
        assert "while ((3ll * 32 * W << 14) > (1ll << n)) ++n;" in src and "return 31 - n;" in src
        n = 0
        while (3 * 32 * w << 14) > (1 << n):
            n += 1
        return 31 - n
    assert hb.MATCH_L2_CHUNK == {32 * w: 1 << idx_bits(w) for w in range(1, consts["ML_MAX_W"] + 1)}
    assert all(c % hb.MATCH_L2_TILE == 0 for c in hb.MATCH_L2_CHUNK.values())
    for w in range(1, 9):                         # the key's range: (d - |q'|^2) << bits | index fits a signed int32 below INT_MAX
        top = 3 * 32 * w * 128 * 128 - 1
        assert ((top << idx_bits(w)) | ((1 << idx_bits(w)) - 1)) < 0x7fffffff and -(32 * w * 128 * 128) << idx_bits(w) >= -(1 << 31)


def test_shifted_formula_equals_plain():
    """What the kernel computes -- |q'|^2 + (|t'|^2 + 2 sum t') + 2 t'.q" with x' = x ^ 0x80 and q" = q ^ 0x7f as int8 -- equals the
    plain formula, on random rows and on rows of all 0, 255, 127 and 128."""
    rng = np.random.default_rng(0)
    for width in (32, 128, 256):
        q, t = rng.integers(0, 256, (12, width), dtype=np.uint8), rng.integers(0, 256, (13, width), dtype=np.uint8)
        for k, v in enumerate((0, 255, 127, 128)):
            q[k], t[3 - k] = v, v
        t[4:8] = q[:4]
        qs, q2 = (q ^ 0x80).view(np.int8).astype(np.int64), (q ^ 0x7f).view(np.int8).astype(np.int64)
        ts = (t ^ 0x80).view(np.int8).astype(np.int64)
        acc = q2 @ ts.T
        assert np.abs(acc).max() <= width * 128 * 128
        d = (qs * qs).sum(1)[:, None] + ((ts * ts).sum(1) + 2 * ts.sum(1))[None, :] + 2 * acc
        assert np.array_equal(d, L.distances(q, t)) and d.max() == width * 255 * 255


class _FakeSolver:
    """hip_backend.Solver.match_l2 / match_descriptors answered by the yardsticks."""

    def __init__(self):
        self.calls = []

    def match_l2(self, sets, pairs=None, **opts):
        self.calls.append(("l2", sets, None if pairs is None else np.asarray(pairs).tolist(), opts))
        return L.match_l2(sets, pairs, **opts)

    def match_descriptors(self, sets, pairs=None, **opts):
        from tests import match_reference as M
        self.calls.append(("hamming", sets, None if pairs is None else np.asarray(pairs).tolist(), opts))
        return M.match_descriptors(sets, pairs, **opts)


def _scene(seed=0, n=40, extra=15, width=128):
    """n descriptors, and a permuted copy with small offsets plus `extra` unrelated ones."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (n, width), dtype=np.uint8)
    perm = rng.permutation(n)
    b = (a[perm].astype(np.int64) + rng.integers(-5, 6, (n, width))).clip(0, 255).astype(np.uint8)
    return a, np.concatenate([b, rng.integers(0, 256, (extra, width), dtype=np.uint8)]), np.argsort(perm)


def test_features_host_side():
    import bundle_adjustment_amd as pkg
    from bundle_adjustment_amd import BruteForceMatcher, features
    assert pkg.match_l2 is features.match_l2
    a, b, partner = _scene()
    ref = L.match_pair(a, b)
    assert ref["good"].all() and np.array_equal(ref["best"], partner)        # (the scene: every copy is found)
    fake = _FakeSolver()
    q, t, d = features.match_l2(a, b, solver=fake)
    assert fake.calls[-1][0] == "l2" and fake.calls[-1][2] is None and fake.calls[-1][3] == {} and len(fake.calls[-1][1]) == 2
    assert q.tolist() == list(range(len(a))) and np.array_equal(t, partner) and np.array_equal(d, ref["dist1"]) and d.dtype == np.int64
    refr = L.match_pair(b, a)
    ms = BruteForceMatcher(solver=fake, norm="l2").match(b, a)
    assert fake.calls[-1][0] == "l2" and fake.calls[-1][3] == dict(ratio=0.75)
    keep = np.nonzero(refr["good"])[0]
    assert 0 < len(keep) < len(b)
    assert [m.queryIdx for m in ms] == keep.tolist() and [m.trainIdx for m in ms] == refr["best"][keep].tolist()
    assert [m.distance for m in ms] == [float(np.sqrt(float(v))) for v in refr["dist1"][keep]]       # cv2's NORM_L2: the distance itself
    assert all(m.imgIdx == 0 and type(m.distance) is float for m in ms)
    assert len(BruteForceMatcher(ratio=0.5, solver=fake, norm="l2").match(b, a)) == L.match_pair(b, a, ratio=0.5)["n_good"]
    # the default stays Hamming
    BruteForceMatcher(solver=fake).match(a[:, :32], b[:, :32])
    assert fake.calls[-1][0] == "hamming"
    n_calls = len(fake.calls)
    m = BruteForceMatcher(solver=fake, norm="l2")
    assert m.match(None, a) == [] and m.match(a, None) == [] and len(fake.calls) == n_calls
    assert m.match(a, b[:1]) == [] and m.match(a, b[:0]) == [] and m.match(a[:0], b) == []
    with pytest.raises(ValueError):
        BruteForceMatcher(norm="cosine")
    with pytest.raises(ValueError):
        features.match_l2(a.astype(np.float32), b, solver=fake)


def test_match_to_keyframes_norm():
    from bundle_adjustment_amd import features
    a, b, _ = _scene(1)
    c, _, _ = _scene(2, n=25)
    fake = _FakeSolver()
    lists = features.match_to_keyframes(b, [a, None, c], solver=fake, norm="l2", ratio=0.8)
    assert len(fake.calls) == 1 and fake.calls[0][0] == "l2" and fake.calls[0][2] == [[1, 0], [2, 0]] and fake.calls[0][3] == dict(ratio=0.8)
    assert lists[1] == []
    for got, kf in ((lists[0], a), (lists[2], c)):
        ref = L.match_pair(kf, b, ratio=0.8)
        keep = np.nonzero(ref["good"])[0]
        assert [(m.queryIdx, m.trainIdx, m.distance) for m in got] == [(int(i), int(ref["best"][i]), float(np.sqrt(float(ref["dist1"][i])))) for i in keep]
    features.match_to_keyframes(b[:, :32], [a[:, :32]], solver=fake)
    assert fake.calls[-1][0] == "hamming"                              # the default
    with pytest.raises(ValueError):
        features.match_to_keyframes(b, [a], solver=fake, norm="l1")


def test_refusals_before_any_device_call(lib):
    """Every refusal of the contract is decided on the host before the handle is touched: the handle here is a block of zero
    bytes, and a call that reached the device through it could not answer with the field's name."""
    from bundle_adjustment_amd import hip_backend as hb
    i64, i32, u8 = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    handle = C.create_string_buffer(1 << 16)
    rng = np.random.default_rng(8)
    desc = rng.integers(0, 256, (10, 32), dtype=np.uint8)
    off = np.array([0, 4, 10], dtype=np.int64)
    pq, pt = np.array([0], dtype=np.int32), np.array([1], dtype=np.int32)
    o = hb.BAMatchOptions()
    assert lib.ba_default_match_options(C.byref(o)) == 0

    def ptr(a, t):
        return None if a is None else a.ctypes.data_as(t)

    def raw(width=32, set_off=off, desc=desc, pq=pq, pt=pt, ratio=0.75, n_sets=None, n_pairs=None, row_off=None):
        o.ratio = ratio
        return lib.ba_match_l2(C.cast(handle, C.c_void_p), width, len(set_off) - 1 if n_sets is None else n_sets, ptr(set_off, i64), ptr(desc, u8),
                               (0 if pq is None else len(pq)) if n_pairs is None else n_pairs, ptr(pq, i32), ptr(pt, i32), C.byref(o),
                               ptr(row_off, i64), None, None, None, None, None, None)
    big, many = np.zeros(65537, dtype=np.int64), np.zeros(65536, dtype=np.int32)
    cases = [
        ("desc_bytes", dict(width=48)), ("desc_bytes", dict(width=0)), ("desc_bytes", dict(width=288)), ("desc_bytes", dict(width=16)),
        ("n_sets", dict(set_off=big, desc=None)), ("n_sets", dict(n_sets=-1)),
        ("n_pairs", dict(pq=many, pt=many)), ("n_pairs", dict(n_pairs=-1)),
        ("ratio", dict(ratio=float("nan"))), ("ratio", dict(ratio=float("inf"))),
        ("set_off", dict(set_off=None, n_sets=2)), ("set_off", dict(set_off=np.array([1, 4, 10], dtype=np.int64))),
        ("set_off", dict(set_off=np.array([0, 6, 4], dtype=np.int64))),
        ("set_off", dict(set_off=np.array([0, 4, 4 + hb.MATCH_MAX_SET + 1], dtype=np.int64))),
        ("desc", dict(desc=None)), ("pair_query", dict(pq=None, n_pairs=1)), ("pair_train", dict(pt=None)),
        ("pair_query", dict(pq=np.array([2], dtype=np.int32))), ("pair_query", dict(pq=np.array([-1], dtype=np.int32))),
        ("pair_train", dict(pt=np.array([2], dtype=np.int32))), ("pair_train", dict(pt=np.array([-1], dtype=np.int32))),
    ]
    for name, change in cases:
        rc = raw(**change)
        msg = lib.ba_last_error().decode()
        assert rc == -1 and msg.startswith("ba_match_l2: ") and name in msg.split(": ", 1)[1], (name, list(change), rc, msg)
    assert "multiple of 32 in 32 .. 256" in (raw(width=48), lib.ba_last_error().decode())[1]
    assert lib.ba_match_l2(None, 32, 0, None, None, 0, None, None, None, *([None] * 7)) == -1 and b"null" in lib.ba_last_error()
    # the empty cases need no device either: row_off is written and the call returns
    ro = np.full(3, -1, dtype=np.int64)
    assert raw(set_off=np.array([0, 0, 4], dtype=np.int64), desc=desc[:4], pq=np.array([0, 0], dtype=np.int32),
               pt=np.array([1, 0], dtype=np.int32), row_off=ro) == 0 and ro.tolist() == [0, 0, 0]
    ro = np.full(1, -1, dtype=np.int64)
    assert raw(pq=None, pt=None, row_off=ro) == 0 and ro.tolist() == [0]
    # every width of the contract passes the width rule (refused here for the next field in line)
    for width in hb.MATCH_L2_DESC_BYTES:
        assert raw(width=width, set_off=None, n_sets=0) == -1 and "set_off" in lib.ba_last_error().decode()
    # Solver.match_l2 refuses mixed widths and dtypes before the library is asked
    s = hb.Solver.__new__(hb.Solver)
    s._lib, s._h = lib, None
    a = np.zeros((3, 32), dtype=np.uint8)
    with pytest.raises(ValueError, match="widths"):
        s.match_l2([a, np.zeros((3, 64), dtype=np.uint8)])
    with pytest.raises(ValueError, match="uint8"):
        s.match_l2([a, a.astype(np.float32)])
    with pytest.raises(ValueError, match="two sets"):
        s.match_l2([a, a, a])
