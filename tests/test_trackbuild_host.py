"""CPU: the numpy yardstick of ba_build_tracks (tests/tracks_reference.py) against an independent depth-first search, three
mutants of the yardstick that the cases must catch, and the host helpers of bundle_adjustment_amd/tracks.py (observations,
to_problem, chain_edges, build_tracks' edge assembly through a stand-in solver)."""
import numpy as np
import pytest

from tests import tracks_reference as R

POLICIES = [("drop", 2), ("drop", 3), ("first", 2), ("first", 3)]


def dfs_tracks(kp_counts, edge_a, edge_b, edge_keep, min_length, conflict):
    """The definitions again, with adjacency lists, a stack and Python sets: no numpy in the logic."""
    kp_off = [0]
    for c in kp_counts:
        kp_off.append(kp_off[-1] + int(c))
    n = kp_off[-1]
    img = []
    for i, c in enumerate(kp_counts):
        img += [i] * int(c)
    adj = [[] for _ in range(n)]
    same = 0
    for e, (a, b) in enumerate(zip(edge_a.tolist(), edge_b.tolist())):
        if edge_keep is not None and not edge_keep[e]:
            continue
        if img[a] == img[b]:
            same += 1
            continue
        adj[a].append(b); adj[b].append(a)
    label = [-1] * n
    comps = []
    for s in range(n):
        if label[s] >= 0:
            continue
        label[s] = s
        stack, mem = [s], [s]
        while stack:
            v = stack.pop()
            for w in adj[v]:
                if label[w] < 0:
                    label[w] = s; stack.append(w); mem.append(w)
        comps.append(sorted(mem))
    track = [-1] * n
    status = [R.STATUS["isolated"]] * n
    counts = dict.fromkeys(R.COUNTS, 0)
    counts["same_image_edges"] = same
    tracks = []
    for mem in comps:                                       # found in ascending order of their smallest node
        if len(mem) < 2:
            continue
        counts["components"] += 1
        seen, kept, lost = set(), [], []
        for v in mem:
            (lost if img[v] in seen else kept).append(v)
            seen.add(img[v])
        if lost:
            counts["conflict_components"] += 1
            if conflict == "drop":
                counts["conflict_nodes"] += len(mem)
                for v in mem:
                    status[v] = R.STATUS["conflict"]
                continue
            counts["conflict_nodes"] += len(lost)
            for v in lost:
                status[v] = R.STATUS["conflict"]
        if len(kept) < min_length:
            counts["short_components"] += 1
            for v in kept:
                status[v] = R.STATUS["short"]
            continue
        for v in kept:
            track[v] = len(tracks); status[v] = R.STATUS["in_track"]
        tracks.append(kept)
    off = [0]
    for t in tracks:
        off.append(off[-1] + len(t))
    counts["tracks"], counts["members"] = len(tracks), off[-1]
    return dict(kp_off=np.array(kp_off, dtype=np.int64), node_label=np.array(label, dtype=np.int32).reshape(-1), node_track=np.array(track, dtype=np.int32).reshape(-1),
                node_status=np.array(status, dtype=np.uint8).reshape(-1), track_off=np.array(off, dtype=np.int64),
                track_node=np.array([v for t in tracks for v in t], dtype=np.int32), counts=counts)


def _cases():
    """A few hundred small random graphs: sparse ones (many short components), denser ones (conflicts, long components),
    with and without a mask."""
    rng = np.random.default_rng(20240607)
    out = []
    for k in range(240):
        n_images = int(rng.integers(1, 9))
        max_kp = int(rng.integers(1, 7))
        kp_counts, a, b = R.random_graph(rng, n_images, max_kp, int(rng.integers(0, 3 * n_images * max_kp // 2 + 1)))
        keep = (rng.random(a.shape[0]) < 0.7).astype(np.uint8) if k % 3 == 0 else None
        out.append((kp_counts, a, b, keep))
    return out


CASES = _cases()


def _differs(x, y):
    try:
        R.assert_same(x, y)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("conflict,min_length", POLICIES)
def test_yardstick_equals_depth_first_search(conflict, min_length):
    seen = dict.fromkeys(R.STATUS, 0)
    for kp_counts, a, b, keep in CASES:
        got = R.build(kp_counts, a, b, keep, min_length, conflict)
        R.assert_same(got, dfs_tracks(kp_counts, a, b, keep, min_length, conflict))
        for name, code in R.STATUS.items():
            seen[name] += int((got["node_status"] == code).sum())
    # the cases reach every status under every policy (a component spans at least two images: none is short of two)
    assert all(v > 0 for k, v in seen.items() if k != "short" or min_length > 2), seen


@pytest.mark.parametrize("mutant", ["no_conflicts", "scatter_order", "by_size"])
def test_each_mutant_of_the_yardstick_is_caught(mutant):
    caught = 0
    for conflict, min_length in POLICIES:
        for kp_counts, a, b, keep in CASES:
            caught += _differs(R.build(kp_counts, a, b, keep, min_length, conflict, mutant=mutant),
                               dfs_tracks(kp_counts, a, b, keep, min_length, conflict))
    assert caught > 0


def test_definitions_on_a_hand_made_graph():
    # images: 0 -> nodes 0 1 2, 1 -> 3 4, 2 -> (none), 3 -> 5 6 7
    kp = [3, 2, 0, 3]
    a = np.array([0, 3, 1, 4, 2, 2, 6], dtype=np.int32)
    b = np.array([3, 5, 4, 6, 2, 1, 1], dtype=np.int32)      # 0-3-5 | 1-4-6-1 | 2-2 (self) | 2-1 (same image) ; 7 isolated
    t = R.build(kp, a, b)
    assert t["node_label"].tolist() == [0, 1, 2, 0, 1, 0, 1, 7]
    assert t["track_off"].tolist() == [0, 3, 6] and t["track_node"].tolist() == [0, 3, 5, 1, 4, 6]
    assert t["node_status"].tolist() == [0, 0, 1, 0, 0, 0, 0, 1] and t["counts"]["same_image_edges"] == 2
    # join the two components through image 0's nodes 0 and 1: a conflict
    a2, b2 = np.append(a, 5).astype(np.int32), np.append(b, 4).astype(np.int32)
    drop = R.build(kp, a2, b2)
    assert drop["counts"]["tracks"] == 0 and drop["node_status"].tolist() == [2, 2, 1, 2, 2, 2, 2, 1] and drop["counts"]["conflict_nodes"] == 6
    first = R.build(kp, a2, b2, conflict="first")
    assert first["track_node"].tolist() == [0, 3, 5] and first["node_status"].tolist() == [0, 2, 1, 0, 2, 0, 2, 1]
    assert first["counts"]["conflict_nodes"] == 3 and first["counts"]["conflict_components"] == 1


# ---- the helpers of bundle_adjustment_amd/tracks.py -------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    """A yardstick dict on planted components over 7 images, and keypoint pixels for every node."""
    rng = np.random.default_rng(5)
    kp_counts, a, b, comps = R.planted_graph(rng, [2, 3, 5, 7, 4, 2, 6], 7, conflicts=(4,), extra_nodes=5)
    tr = R.build(kp_counts, a, b)
    pix = [rng.uniform(0, 640, (int(c), 2)) for c in kp_counts]
    return dict(kp_counts=kp_counts, a=a, b=b, comps=comps, tracks=tr, pix=pix)


def test_observations_follow_the_tracks(scene):
    from bundle_adjustment_amd import tracks as T
    from bundle_adjustment_amd.map_structures import KeyPoint
    tr = scene["tracks"]
    cam_idx, pt_idx, uv = T.observations(tr, scene["pix"])
    kp_off = tr["kp_off"]
    assert cam_idx.dtype == np.int32 and pt_idx.dtype == np.int32 and uv.dtype == np.float64 and uv.shape == (len(tr["track_node"]), 2)
    for row, node in enumerate(tr["track_node"]):
        i = int(R.image_of(kp_off, node))
        assert cam_idx[row] == i and pt_idx[row] == tr["node_track"][node]
        assert np.array_equal(uv[row], scene["pix"][i][node - kp_off[i]].astype(np.float32).astype(np.float64))
    assert np.array_equal(uv, uv.astype(np.float32))          # float32 values, as cv2's pixels are
    # no point twice in one camera
    pairs = set(zip(cam_idx.tolist(), pt_idx.tolist()))
    assert len(pairs) == len(cam_idx)
    # KeyPoint lists give the same
    kps = [[KeyPoint(pt=(float(x), float(y))) for x, y in p] for p in scene["pix"]]
    for got, want in zip(T.observations(tr, kps), (cam_idx, pt_idx, uv)):
        assert np.array_equal(got, want)
    with pytest.raises(ValueError):
        T.observations(tr, scene["pix"][:-1])


def test_to_problem_validates_for_both_problem_kinds(scene):
    from bundle_adjustment_amd import tracks as T
    from bundle_adjustment_amd.bal import BALProblem
    from bundle_adjustment_amd.problem import BAProblem
    tr, n_img = scene["tracks"], len(scene["kp_counts"])
    p = T.to_problem(tr, scene["pix"], np.zeros((n_img, 6)), K4=[500.0, 500.0, 320.0, 240.0])
    assert isinstance(p, BAProblem) and p.validate() is p and p.n_pts == tr["counts"]["tracks"] and p.n_obs == tr["counts"]["members"]
    assert not p.pts.any()
    q = T.to_problem(tr, scene["pix"], np.zeros((n_img, 9)))
    assert isinstance(q, BALProblem) and q.validate() is q and np.array_equal(q.pt_idx, p.pt_idx) and np.array_equal(q.uv, p.uv)
    for cams, K4 in ((np.zeros((n_img, 6)), None), (np.zeros((n_img, 9)), [1.0, 1.0, 0.0, 0.0]), (np.zeros((n_img + 1, 6)), [1.0, 1.0, 0.0, 0.0])):
        with pytest.raises(ValueError):
            T.to_problem(tr, scene["pix"], cams, K4)


def test_chain_edges_reproduce_the_tracks(scene):
    from bundle_adjustment_amd import tracks as T
    for conflict in ("drop", "first"):
        tr = R.build(scene["kp_counts"], scene["a"], scene["b"], conflict=conflict)
        ca, cb = T.chain_edges(tr)
        assert ca.dtype == np.int32 and len(ca) == tr["counts"]["members"] - tr["counts"]["tracks"]
        again = R.build(scene["kp_counts"], ca, cb, conflict=conflict)
        for k in ("track_off", "track_node", "node_track"):
            assert np.array_equal(again[k], tr[k]), k
        # the incremental use: old tracks as chain edges next to a new image's matches keep their order and first members
        kp2 = list(scene["kp_counts"]) + [2]
        n_old = int(tr["kp_off"][-1])
        firsts = tr["track_node"][tr["track_off"][:-1]]
        grown = R.build(kp2, np.append(ca, firsts[0]), np.append(cb, n_old), conflict=conflict)
        assert np.array_equal(grown["node_track"][firsts], np.arange(len(firsts)))
        assert grown["node_track"][n_old] == 0 and grown["node_track"][n_old + 1] == -1


class StandInSolver:
    """Records what build_tracks hands to Solver.build_tracks and answers with the yardstick."""

    def __init__(self):
        self.calls = []

    def build_tracks(self, kp_counts, edge_a, edge_b, edge_keep=None, **opts):
        self.calls.append((np.array(kp_counts), np.array(edge_a), np.array(edge_b), None if edge_keep is None else np.array(edge_keep), opts))
        return R.build(kp_counts, edge_a, edge_b, edge_keep, **opts)


def test_build_tracks_assembles_the_edges_of_the_pairs():
    import bundle_adjustment_amd as pkg
    from bundle_adjustment_amd import tracks as T
    assert pkg.build_tracks is T.build_tracks and pkg.chain_edges is T.chain_edges and pkg.to_problem is T.to_problem
    n_kp = [4, 3, 5]
    s = StandInSolver()
    pairs = [(0, 1, [0, 3], [2, 1]), (1, 2, np.array([2, 0]), np.array([4, 4]), np.array([1, 0])), (2, 0, [1], [1], None)]
    out = T.build_tracks(n_kp, pairs, solver=s, min_length=2, conflict="first")
    kp_counts, a, b, keep, opts = s.calls[0]
    assert a.dtype == np.int32 and b.dtype == np.int32 and keep.dtype == np.uint8 and opts == dict(min_length=2, conflict="first")
    assert a.tolist() == [0, 3, 6, 4, 8] and b.tolist() == [6, 5, 11, 11, 1] and keep.tolist() == [1, 1, 1, 0, 1]
    assert out["track_node"].tolist() == [0, 6, 11, 1, 8, 3, 5]
    assert out["track_image"].tolist() == [0, 1, 2, 0, 2, 0, 1] and out["track_kp"].tolist() == [0, 2, 4, 1, 1, 3, 1]
    # no mask anywhere: None goes down; no pairs at all: empty edge arrays
    T.build_tracks(n_kp, pairs[:1], solver=s)
    assert s.calls[1][3] is None and s.calls[1][4] == {}
    empty = T.build_tracks(n_kp, [], solver=s)
    assert s.calls[2][1].shape == (0,) and empty["track_image"].shape == (0,) and empty["counts"]["tracks"] == 0
    for bad in ([(0, 3, [0], [0])], [(0, 1, [4], [0])], [(0, 1, [0, 1], [0])], [(0, 1, [0], [0], [1, 1])], [(0, 1, [0])]):
        with pytest.raises(ValueError):
            T.build_tracks(n_kp, bad, solver=s)


def test_node_numbers_are_checked_before_they_are_narrowed():
    """An int64 node number outside int32 must not wrap into a valid node on its way to the library (2^32 + 5 -> 5)."""
    from bundle_adjustment_amd.hip_backend import _node_array
    for good in ([0, 5, (1 << 31) - 1], np.array([3, 4], dtype=np.int64), np.array([[1, 2]], dtype=np.int32), np.array([7], dtype=np.uint64), []):
        out = _node_array(good, "edge_a")
        assert out.dtype == np.int32 and out.flags["C_CONTIGUOUS"] and out.tolist() == np.asarray(good).reshape(-1).tolist()
    assert _node_array([-1], "edge_a").tolist() == [-1]      # (in int32: the library's to refuse, by edge number)
    for bad, where in (([1, (1 << 32) + 5], r"edge_b\[1\] = 4294967301"), ([-(1 << 31) - 1], r"edge_b\[0\]"),
                       (np.array([0, 0, 1 << 63], dtype=np.uint64), r"edge_b\[2\]"), ([1 << 31], r"edge_b\[0\] = 2147483648"), ([1.5], "integers")):
        with pytest.raises(ValueError, match=where):
            _node_array(bad, "edge_b")


def test_binding_lists_the_call(tmp_path):
    """The ABI side of the feature: the symbols, the options struct and the status names."""
    import ctypes as C
    import __graft_entry__ as g
    g.build()
    from bundle_adjustment_amd import hip_backend as hb
    lib = hb.load_library()
    assert hasattr(lib, "ba_build_tracks") and C.sizeof(hb.BATrackBuildOptions) == 16
    o = hb.BATrackBuildOptions(9, 9, 9, 9)
    assert lib.ba_default_trackbuild_options(C.byref(o)) == 0 and (o.min_length, o.conflict, o.max_rounds, o.reserved) == (2, 0, 0, 0)
    assert hb.TRACKBUILD_STATUS == R.STATUS and tuple(hb.TRACKBUILD_COUNTS) == R.COUNTS
    assert lib.ba_build_tracks(None, 0, None, 0, None, None, None, None, None, None, None, None, None, None) == -1
