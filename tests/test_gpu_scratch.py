"""GPU: the scratch arena ("The scratch arena") under the calls that keep nothing on the device between calls --
relative_pose, homography, sim3, fundamental, match_descriptors, match_guided, extract_orb, pose_graph, pose_graph_system,
train_vocabulary, bow_transform, bow_score, build_tracks.  Results are compared bit for bit (NaN equal to NaN):
(1) no leftovers: a call on a fresh handle, after the arena was filled with 0xff, after it was filled with 0x00 and after a
    larger call of another feature returns the same arrays: it reads nothing that it did not upload, clear or compute;
(2) grown and reused: small, large, small again on one handle and small on a fresh one (the pair-shaped calls: also three
    pairs without a match, which return FEW_MATCHES);
(3) maximum, not sum: one small call of each feature in turn leaves the arena at most twice the largest that any of them
    reaches alone, and a repeated call stops allocating."""
import numpy as np
import pytest

from tests import bow_reference as B
from tests import posegraph_reference as PG
from tests import relpose_reference as RP
from tests import sim3_reference as S3

pytestmark = pytest.mark.gpu

FEW_MATCHES = 1                # of all four status enums
PAIR_CALLS = {"relative_pose": 5, "homography": 4, "sim3": 3, "fundamental": 7}   # the call's minimal sample


def _points(name, n, seed):
    """n matches of a scene: pixels (n, 2) | (n, 2), for sim3 points (n, 3) | (n, 3)."""
    width = 3 if name == "sim3" else 2
    if n == 0:
        return np.zeros((0, width)), np.zeros((0, width))
    return S3.noisy_scene(seed, n)[:2] if width == 3 else RP.noisy_scene(n, planar=name == "homography", seed=seed)[:2]


def _pairs(s, name, counts, seed0, **opts):
    sets = [_points(name, n, seed0 + i) for i, n in enumerate(counts)]
    a, b = np.concatenate([x[0] for x in sets]), np.concatenate([x[1] for x in sets])
    off = np.r_[0, np.cumsum(counts)].astype(np.int64)
    head = () if name == "fundamental" else (RP.K_TEST,)
    return getattr(s, name)(*head, a, b, off, **opts)


def _pair_call(name):
    k = PAIR_CALLS[name]
    return lambda s, large: _pairs(s, name, (600,), 20, n_hyp=4096) if large else _pairs(s, name, (0, k, k + 1, 40), 10, n_hyp=64)


def _desc(seed, n, width=32):
    return np.random.default_rng(seed).integers(0, 256, (n, width), dtype=np.uint8)


def _match_sets(large):
    """Small: one pair of 1 x 300 and one of 257 x 65 descriptors; large: one pair of 1500 x 1500.  Every second query is a train
    descriptor with 10 bits flipped, so that the ratio test keeps some."""
    sets = []
    for i, (nq, nt) in enumerate(((1500, 1500),) if large else ((1, 300), (257, 65))):
        rng = np.random.default_rng(45 + i)
        q, t = _desc(40 + 2 * i, nq), _desc(41 + 2 * i, nt)
        q[::2] = t[np.arange(0, nq, 2) % nt]
        for r in range(0, nq, 2):
            bits = rng.choice(256, 10, replace=False)
            np.bitwise_xor.at(q[r], bits // 8, (1 << (bits % 8)).astype(np.uint8))
        sets += [q, t]
    return sets, [(2 * p, 2 * p + 1) for p in range(len(sets) // 2)]


def _match(s, large):
    sets, pairs = _match_sets(large)
    return s.match_descriptors(sets, pairs, mutual=1)


def _match_guided(s, large):
    sets, pairs = _match_sets(large)
    rng = np.random.default_rng(50)
    xy = lambda n: (np.c_[rng.integers(0, 256, n), rng.integers(0, 192, n)] / 4).astype(np.float32)      # noqa: E731
    kps = [xy(len(d)) for d in sets]
    rows = sum(len(sets[q]) for q, _ in pairs)
    window = np.c_[xy(rows), rng.choice(np.array([-1, 0, 2.5, 10, 100], dtype=np.float32), rows)].astype(np.float32)
    return s.match_guided(sets, kps, pairs, window=window, mutual=1)


def orb_image(seed, h, w):
    """Random rectangles on a flat ground, with their corners at least 20 pixels from the border."""
    rng = np.random.default_rng(seed)
    img = np.full((h, w), 60, np.uint8)
    for _ in range(h * w // 700):
        x0, y0 = int(rng.integers(20, w - 28)), int(rng.integers(20, h - 28))
        img[y0:y0 + int(rng.integers(4, 12)), x0:x0 + int(rng.integers(4, 12))] ^= 0xc0
    return img


def _orb(s, large):
    if large:
        return s.extract_orb(np.stack([orb_image(60 + i, 270, 310) for i in range(4)]), n_features=1000)
    return s.extract_orb(orb_image(0, 64, 64), n_features=50, n_levels=2, edge_threshold=25)


def _graph(large):
    return PG.ring(n=200 if large else 6, skip_every=3)      # small: 6 nodes, 5 + 1 + 2 = 8 edges


def _pose_graph(s, large):
    sc = _graph(large)
    out = s.pose_graph(sc["start"], sc["ei"], sc["ej"], sc["meas"], info=sc["info"], held=sc["held"])
    return {k: v for k, v in out.items() if not k.startswith("seconds")}


def _pose_graph_system(s, large):
    sc = _graph(large)
    return s.pose_graph_system(sc["start"], sc["ei"], sc["ej"], sc["meas"], info=sc["info"], held=sc["held"], lam=0.3)


def _bow_sets(large):
    """Small: 400 descriptors in 4 sets (branching 3, levels 3: the second and third level re-take their buffers)."""
    return [_desc(70 + i, 2000 if large else 100) for i in range(4)]


def _train(s, large):
    return s.train_vocabulary(_bow_sets(large), branching=10 if large else 3, levels=3, iters=5, seed=3)


_VOCAB = {}


def _bow_transform(s, large):
    if not _VOCAB:
        _VOCAB.update(B.train(_bow_sets(False), branching=3, levels=3, iters=5, seed=3))
    s.set_vocabulary(_VOCAB)      # resident: not the arena's
    return s.bow_transform(_bow_sets(large))


def _bow_score(s, large):
    rng = np.random.default_rng(80)
    d, q = B.random_vectors(rng, 3000 if large else 40, empty=(3,)), B.random_vectors(rng, 200 if large else 9, empty=(4,))
    return s.bow_score(q, d, top_k=5, dense=True)


def _track_graph(n_nodes, seed):
    rng = np.random.default_rng(seed)
    kp_counts = np.diff(np.r_[0, np.sort(rng.integers(0, n_nodes + 1, 11)), n_nodes])      # 12 images, some may be empty
    a, b = rng.integers(0, n_nodes, n_nodes).astype(np.int32), rng.integers(0, n_nodes, n_nodes).astype(np.int32)
    return kp_counts, a, b


def _tracks(s, large):
    if large:
        return s.build_tracks(*_track_graph(200000, 92))
    return {n: s.build_tracks(*_track_graph(n, 90 + i)) for i, n in enumerate((255, 4097))}


CALLS = {name: _pair_call(name) for name in PAIR_CALLS}
CALLS.update(match_descriptors=_match, match_guided=_match_guided, extract_orb=_orb, pose_graph=_pose_graph,
             pose_graph_system=_pose_graph_system, train_vocabulary=_train, bow_transform=_bow_transform, bow_score=_bow_score,
             build_tracks=_tracks)


def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind in "fc")


@pytest.fixture(scope="module")
def hb():
    import __graft_entry__ as g
    g.build()
    from bundle_adjustment_amd import hip_backend
    return hip_backend


@pytest.fixture(scope="module")
def alone(hb):
    """Every small call on a handle of its own: the result, and what the arena holds after it."""
    out = {}
    for name, call in CALLS.items():
        with hb.Solver(0) as s:
            out[name] = (call(s, False), s.stats()["scratch_bytes"])
    return out


def test_the_small_calls_run_on_their_data(alone):
    r = {name: res for name, (res, _) in alone.items()}
    for name in PAIR_CALLS:
        assert r[name]["n_inliers"][3] > 0
    assert r["match_descriptors"]["good"].any() and r["match_guided"]["n_cand"].max() > 1
    assert r["extract_orb"]["n_kp"][0] > 0
    assert r["pose_graph"]["iterations"] > 0 and r["pose_graph_system"]["H"].shape == (42, 42)
    assert r["train_vocabulary"]["levels"] == 3 and r["train_vocabulary"]["n_nodes"] > 1 + 3 + 9      # three levels were split
    assert r["bow_transform"]["vec_off"][-1] > 0 and r["bow_score"]["top_score"].max() > 0
    assert all(r["build_tracks"][n]["counts"]["tracks"] > 0 for n in (255, 4097))
    assert all(nbytes > 0 and nbytes % 256 == 0 for _, nbytes in alone.values())


@pytest.mark.parametrize("name", CALLS)
def test_no_leftovers(hb, alone, name):
    call, first = CALLS[name], alone[name][0]
    other = CALLS["build_tracks" if name in PAIR_CALLS else "relative_pose"]
    with hb.Solver(0) as s:
        s.debug_scratch_fill(0xff)      # (an empty arena: nothing to fill)
        assert _same(first, call(s, False))
        s.debug_scratch_fill(0xff)
        assert _same(first, call(s, False)), "differs after the arena was filled with 0xff"
        s.debug_scratch_fill(0x00)
        assert _same(first, call(s, False)), "differs after the arena was filled with 0x00"
        other(s, True)
        assert s.stats()["scratch_bytes"] > alone[name][1]      # the other call was the larger one
        assert _same(first, call(s, False)), "differs after a larger call of another feature"


@pytest.mark.parametrize("name", CALLS)
def test_grown_and_reused(hb, alone, name):
    call = CALLS[name]
    with hb.Solver(0) as s:
        if name in PAIR_CALLS:
            r = _pairs(s, name, (0, 0, 0), 0)
            assert r["status"].tolist() == [FEW_MATCHES] * 3 and r["n_inliers"].tolist() == [0, 0, 0] and r["match_inlier"].shape == (0,)
        first = call(s, False)
        small_bytes = s.stats()["scratch_bytes"]
        big = call(s, True)
        assert s.stats()["scratch_bytes"] > small_bytes      # the arena grew under the large call
        again = call(s, False)
    if name in PAIR_CALLS:
        print(f"{name}: status {first['status'].tolist()}, inliers {first['n_inliers'].tolist()}; the large pair: status {big['status'].tolist()}, "
              f"{big['n_inliers'].tolist()} inliers")
        assert first["status"][0] == FEW_MATCHES and first["status"][1] == FEW_MATCHES      # n = K is below every call's n >= K + 1
        assert first["n_inliers"][3] > 0 and big["n_inliers"][0] > 0                        # the calls ran on their data
    assert _same(first, again) and _same(first, alone[name][0])


def test_maximum_not_sum(hb, alone):
    largest = max(nbytes for _, nbytes in alone.values())
    with hb.Solver(0) as s:
        for name, call in CALLS.items():
            call(s, False)
            print(f"{name}: alone {alone[name][1]} bytes, arena now {s.stats()['scratch_bytes']} bytes after {s.stats()['scratch_allocs']} allocations")
        assert s.stats()["scratch_bytes"] <= 2 * largest
        last = list(CALLS.values())[-1]
        last(s, False)      # (the first repeat may still merge the blocks the call before it added)
        allocs = s.stats()["scratch_allocs"]
        last(s, False)
        last(s, False)
        assert s.stats()["scratch_allocs"] == allocs
        assert s.stats()["scratch_bytes"] <= 2 * largest
