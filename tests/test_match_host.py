"""CPU: the yardstick of the descriptor-matching tests (tests/match_reference.py) against a triple Python loop, and the surface
of ba_match_descriptors that needs no device: the exported symbols, the options struct, the host side of features.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import match_reference as M

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
    d = [[sum(bin(int(a) ^ int(b)).count("1") for a, b in zip(q[i], t[j])) for j in range(nt)] for i in range(nq)]
    out = dict(best=[], second=[], dist1=[], dist2=[], good=[])
    for i in range(nq):
        keys = sorted((d[i][j], j) for j in range(nt))
        b, s = (keys[0] if nt >= 1 else (-1, -1)), (keys[1] if nt >= 2 else (-1, -1))
        g = b[1] >= 0
        if ratio > 0:
            g = g and s[1] >= 0 and float(b[0]) < ratio * float(s[0])
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
            # few distinct rows of few set bits: ties in d, duplicates among the train rows and among the queries
            pool = (rng.integers(0, 256, (3, 8)) & rng.integers(0, 256, (3, 8)) & 0x0F).astype(np.uint8)
            q, t = pool[rng.integers(0, 3, nq)], pool[rng.integers(0, 3, nt)]
            if nq and nt > 2:
                q[0] = t[2]                       # a planted exact match that ties with every copy of it
            for max_distance in (-1, 0, 3):
                ref = M.match_pair(q, t, ratio=ratio, max_distance=max_distance, mutual=mutual)
                want = _loops(q, t, ratio, max_distance, mutual)
                for k, v in want.items():
                    assert ref[k].tolist() == v, (nq, nt, k)
                assert ref["n_good"] == sum(want["good"])
                cases += 1
    assert cases == 64 * 3


def test_yardstick_edges_and_ratio_boundaries():
    z = np.zeros((1, 8), dtype=np.uint8)

    def row(bits):
        r = np.zeros(8, dtype=np.uint8)
        for b in range(bits):
            r[b // 8] |= 1 << (b % 8)
        return r
    # nt = 0 and nt = 1
    r = M.match_pair(z, np.zeros((0, 8), dtype=np.uint8))
    assert (r["best"][0], r["second"][0], r["dist1"][0], r["dist2"][0], r["good"][0]) == (-1, -1, -1, -1, False)
    r = M.match_pair(z, z)
    assert (r["best"][0], r["second"][0], r["dist1"][0], r["dist2"][0], r["good"][0]) == (0, -1, 0, -1, False)
    assert M.match_pair(z, z, ratio=0)["good"][0]
    # d1 = 3, d2 = 4, ratio 0.75: 3 < 3.0 is false; d1 = 2 is good
    r = M.match_pair(z, np.stack([row(4), row(3)]))
    assert (r["best"][0], r["second"][0], r["dist1"][0], r["dist2"][0], r["good"][0]) == (1, 0, 3, 4, False)
    r = M.match_pair(z, np.stack([row(4), row(2)]))
    assert (r["dist1"][0], r["dist2"][0], r["good"][0]) == (2, 4, True)
    # ties go to the lower index, and dist1 == dist2 fails every ratio <= 1
    r = M.match_pair(z, np.stack([row(5), row(2), row(2)]), ratio=1.0)
    assert (r["best"][0], r["second"][0], r["dist1"][0], r["dist2"][0], r["good"][0]) == (1, 2, 2, 2, False)
    # mutual: one train row the best of two queries at equal distance -- the lower query keeps it
    r = M.match_pair(np.stack([row(1), row(1)]), np.stack([row(0), row(40)]), mutual=1)
    assert r["best"].tolist() == [0, 0] and r["good"].tolist() == [True, False]
    # the batch form
    out = M.match_descriptors([z, np.stack([row(4), row(2)]), np.zeros((0, 8), dtype=np.uint8)], [(0, 1), (2, 1), (1, 0), (1, 2)])
    assert out["row_off"].tolist() == [0, 1, 1, 3, 5] and out["n_good"].tolist() == [1, 0, 0, 0]
    assert out["best"].tolist() == [1, 0, 0, -1, -1] and out["dist2"].tolist() == [4, -1, -1, -1, -1]
    empty = M.match_descriptors([], [])
    assert empty["row_off"].tolist() == [0] and empty["best"].shape == (0,) and empty["n_good"].shape == (0,)


def test_abi(lib):
    """The two symbols, the defaults, and struct ba_match_options of include/ba_hip.h: double, int32 x 2 = 16 bytes."""
    from bundle_adjustment_amd import hip_backend as hb
    assert hasattr(lib, "ba_match_descriptors") and hasattr(lib, "ba_default_match_options")
    assert "ba_match_descriptors" in hb.SYMBOLS and "ba_default_match_options" in hb.SYMBOLS
    o = hb.BAMatchOptions()
    o.ratio, o.max_distance, o.mutual = 9.0, 9, 9
    assert lib.ba_default_match_options(C.byref(o)) == 0
    assert (o.ratio, o.max_distance, o.mutual) == (0.75, -1, 0)
    assert C.sizeof(hb.BAMatchOptions) == 16
    off = {k: getattr(hb.BAMatchOptions, k).offset for k, _ in hb.BAMatchOptions._fields_}
    assert off == dict(ratio=0, max_distance=8, mutual=12)
    hdr = open(os.path.join(ROOT, "include", "ba_hip.h")).read()
    body = re.search(r"typedef struct ba_match_options \{(.*?)\} ba_match_options;", hdr, flags=re.S).group(1)
    fields = re.findall(r"(int32_t|double)\s+([a-z_0-9]+)\s*;", body)
    ctype = {"double": C.c_double, "int32_t": C.c_int32}
    assert [(n, ctype[t]) for t, n in fields] == list(hb.BAMatchOptions._fields_)
    assert lib.ba_default_match_options(None) == -1 and b"null" in lib.ba_last_error()
    # the constants the GPU tests size their shapes by are the kernels'
    src = open(os.path.join(ROOT, "bundle_adjustment_amd", "csrc", "ba_match.hpp")).read()
    consts = {k: int(v) for k, v in re.findall(r"constexpr int (MT_[A-Z_]+) = (\d+);", src)}
    assert (consts["MT_THREADS"], consts["MT_TILE"], consts["MT_MIN_SPLIT"], consts["MT_MAX_SPLITS"], 1 << consts["MT_IDX_BITS"]) == \
        (hb.MATCH_BLOCK, hb.MATCH_TILE, hb.MATCH_MIN_SPLIT, hb.MATCH_MAX_SPLITS, hb.MATCH_MAX_SET)
    assert hb.MATCH_DESC_BYTES == tuple(range(8, 8 * consts["MT_MAX_WORDS"] + 1, 8))


def test_options_by_name():
    from bundle_adjustment_amd import hip_backend as hb

    class Lib:
        @staticmethod
        def ba_default_match_options(ref):
            ref._obj.ratio, ref._obj.max_distance, ref._obj.mutual = 0.75, -1, 0
            return 0
    s = hb.Solver.__new__(hb.Solver)
    s._lib = Lib()
    o = s.match_options(ratio=0.8, mutual=1)
    assert (o.ratio, o.max_distance, o.mutual) == (0.8, -1, 1)
    with pytest.raises(TypeError):
        s.match_options(cross_check=1)
    # refused before the library is asked: mixed widths, a wrong dtype, pairs=None with three sets
    a, b = np.zeros((3, 32), dtype=np.uint8), np.zeros((3, 64), dtype=np.uint8)
    with pytest.raises(ValueError, match="widths"):
        s.match_descriptors([a, b])
    with pytest.raises(ValueError, match="uint8"):
        s.match_descriptors([a, a.astype(np.float32)])
    with pytest.raises(ValueError, match="two sets"):
        s.match_descriptors([a, a, a])


class _FakeSolver:
    """hip_backend.Solver.match_descriptors answered by the yardstick."""

    def __init__(self):
        self.calls = []

    def match_descriptors(self, sets, pairs=None, **opts):
        self.calls.append((sets, None if pairs is None else np.asarray(pairs).tolist(), opts))
        return M.match_descriptors(sets, pairs, **opts)


def _scene(seed=0, n=40, extra=15):
    """n descriptors, and a permuted copy with up to 12 flipped bits each plus `extra` unrelated ones."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    perm = rng.permutation(n)
    b = a[perm].copy()
    for r in range(n):
        for bit in rng.choice(256, rng.integers(0, 13), replace=False):
            b[r, bit // 8] ^= np.uint8(1 << (bit % 8))
    b = np.concatenate([b, rng.integers(0, 256, (extra, 32), dtype=np.uint8)])
    return a, b, np.argsort(perm)


def test_features_host_side():
    import bundle_adjustment_amd as pkg
    from bundle_adjustment_amd import BruteForceMatcher, features, match
    assert pkg.BruteForceMatcher is features.BruteForceMatcher and match is features.match
    a, b, partner = _scene()
    ref = M.match_pair(a, b)
    assert ref["good"].all() and np.array_equal(ref["best"], partner)        # (the scene: every copy is found)
    fake = _FakeSolver()
    q, t, d = features.match(a, b, solver=fake)
    assert fake.calls[-1][1] is None and fake.calls[-1][2] == {} and len(fake.calls[-1][0]) == 2
    assert q.tolist() == list(range(len(a))) and np.array_equal(t, partner) and np.array_equal(d, ref["dist1"])
    # the other direction: the unrelated rows fail the ratio test, the list stays in query order
    refr = M.match_pair(b, a)
    ms = BruteForceMatcher(solver=fake).match(b, a)
    assert fake.calls[-1][2] == dict(ratio=0.75)
    keep = np.nonzero(refr["good"])[0]
    assert 0 < len(keep) < len(b)
    assert [m.queryIdx for m in ms] == keep.tolist() and [m.trainIdx for m in ms] == refr["best"][keep].tolist()
    assert [m.distance for m in ms] == [float(v) for v in refr["dist1"][keep]]
    assert all(m.imgIdx == 0 and type(m.distance) is float and type(m.queryIdx) is int and type(m.trainIdx) is int for m in ms)
    assert len(BruteForceMatcher(ratio=0.5, solver=fake).match(b, a)) == M.match_pair(b, a, ratio=0.5)["n_good"]
    assert fake.calls[-1][2] == dict(ratio=0.5)
    # None and too few train descriptors: [] as in the reference, and None does not reach the solver
    n_calls = len(fake.calls)
    m = BruteForceMatcher(solver=fake)
    assert m.match(None, a) == [] and m.match(a, None) == [] and m.match(None, None) == [] and len(fake.calls) == n_calls
    assert m.match(a, b[:1]) == [] and m.match(a, b[:0]) == [] and m.match(a[:0], b) == []
    with pytest.raises(ValueError):
        features.match(a.astype(np.int32), b, solver=fake)


def test_match_to_keyframes_host_side():
    from bundle_adjustment_amd import features
    a, b, _ = _scene(1)
    c, _, _ = _scene(2, n=25)
    fake = _FakeSolver()
    lists = features.match_to_keyframes(b, [a, None, c, a[:0]], solver=fake, ratio=0.8)
    assert len(fake.calls) == 1                                   # ONE call for the whole loop
    sets, pairs, opts = fake.calls[0]
    assert len(sets) == 4 and sets[0] is b and pairs == [[1, 0], [2, 0], [3, 0]] and opts == dict(ratio=0.8)
    assert lists[1] == [] and lists[3] == []
    for got, kf in ((lists[0], a), (lists[2], c)):
        ref = M.match_pair(kf, b, ratio=0.8)                      # keyframe = queries, the new frame = train
        keep = np.nonzero(ref["good"])[0]
        assert [(m.queryIdx, m.trainIdx, m.distance) for m in got] == [(int(i), int(ref["best"][i]), float(ref["dist1"][i])) for i in keep]
    assert len(lists[0]) == len(a)
    assert features.match_to_keyframes(None, [a, c], solver=fake) == [[], []]
    assert features.match_to_keyframes(b, [], solver=fake) == [] and features.match_to_keyframes(b, [None], solver=fake) == [[]]
    assert len(fake.calls) == 1
