"""GPU: ba_build_tracks against the numpy yardstick of tests/tracks_reference.py.  The arithmetic is integer: every comparison
is exact equality on every array and every count except the hook-round count.

Shapes.  256 lanes per workgroup: n_edges = 255, 256, 257, 1025 over 600 nodes; N = 255, 256, 257 nodes; N = 4097 = one scan block
of 4096 plus one, so that the scan's second level runs.  Segment classes: a wave sorts segments of at most 64 nodes, a workgroup
stages at most 12288 in LDS, longer ones are ranked from global memory; BA_DEBUG_TRACK_SEG=64 moves the borders to 32 and 64, and
components of 2, 31, 32, 33, 64, 65, 200 nodes reach all three classes and both borders."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import tracks_reference as R

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


def round_cap(n):
    """The library's cap on hook rounds (include/ba_hip.h): ceil(log2 max(N, 2)) + 2."""
    return math.ceil(math.log2(max(n, 2))) + 2


def check(solver, kp_counts, a, b, keep=None, **opts):
    got = solver.build_tracks(kp_counts, a, b, keep, **opts)
    R.assert_same(got, R.build(kp_counts, a, b, keep, **opts), what=f"{opts}: ")
    n = int(np.sum(kp_counts))
    assert got["counts"]["rounds"] <= round_cap(n) and (got["counts"]["rounds"] >= 1 or len(a) == 0)
    return got


def both_policies(solver, kp_counts, a, b, keep=None):
    return [check(solver, kp_counts, a, b, keep, min_length=m, conflict=c) for c in ("drop", "first") for m in (2, 3)]


# ------------------------------------------------------------------------------------------------ tile borders
@pytest.mark.parametrize("n_edges", [255, 256, 257, 1025])
def test_edge_counts_at_the_workgroup_borders(solver, n_edges):
    rng = np.random.default_rng(n_edges)
    kp_counts = 5 + rng.multinomial(450, np.full(30, 1 / 30))      # 600 nodes in 30 images
    n = int(kp_counts.sum())
    a = rng.integers(0, n, n_edges).astype(np.int32)
    b = rng.integers(0, n, n_edges).astype(np.int32)
    both_policies(solver, kp_counts, a, b)
    # the LAST edge matters: it alone joins two nodes that nothing else touches
    kp2 = np.append(kp_counts, [1, 1])
    out = check(solver, kp2, np.append(a, n).astype(np.int32), np.append(b, n + 1).astype(np.int32))
    assert out["node_label"][n + 1] == n and out["node_track"][n] == out["counts"]["tracks"] - 1


@pytest.mark.parametrize("n", [255, 256, 257, 4097])
def test_node_counts_at_the_workgroup_and_scan_borders(solver, n):
    rng = np.random.default_rng(n)
    kp_counts = np.full(n // 16, 16)
    kp_counts = np.append(kp_counts, n - kp_counts.sum())
    n_edges = 40 if n < 1000 else 3000
    a = rng.integers(0, n, n_edges).astype(np.int32)
    b = rng.integers(0, n, n_edges).astype(np.int32)
    a[0], b[0] = n - 1, 0                                   # the last node is in a component, and it is the first's
    outs = both_policies(solver, kp_counts, a, b)
    assert outs[0]["node_label"][n - 1] == 0


def test_more_nodes_than_one_scan_pass(solver):
    """One pass of the scan kernels takes 1024 * 4096 items; with 300 nodes more the running total is carried into a second pass.
    A fault here shows only at this size.  Few components, so that the yardstick stays quick."""
    one_pass = 1024 * 4096
    kp_counts = np.append(np.full(64, one_pass // 64), [150, 150])
    n = one_pass + 300
    a = np.array([5, 70000, 70001, one_pass - 1, one_pass + 10, one_pass + 11, 3, one_pass + 149, 200000], dtype=np.int32)
    b = np.array([one_pass + 20, 140000, 140000, one_pass + 5, one_pass + 160, one_pass + 161, n - 1, n - 2, 300000], dtype=np.int32)
    out = check(solver, kp_counts, a, b)
    assert out["counts"]["tracks"] == 7 and out["counts"]["conflict_components"] == 1 and out["node_track"][n - 2] == 6
    first = check(solver, kp_counts, a, b, conflict="first")
    assert first["counts"]["tracks"] == 8 and first["node_status"][70001] == R.STATUS["conflict"]


# ------------------------------------------------------------------------------------------------ segment classes
@pytest.mark.parametrize("conflicts", [(), (1, 3, 5, 6)], ids=["clean", "conflicts"])
def test_every_sort_class_and_both_borders(hb, solver, monkeypatch, conflicts):
    rng = np.random.default_rng(64)
    sizes = [2, 31, 32, 33, 64, 65, 200]
    kp_counts, a, b, comps = R.planted_graph(rng, sizes, 200, conflicts=conflicts, extra_nodes=9)
    want = {c: R.build(kp_counts, a, b, conflict=c) for c in ("drop", "first")}
    if not conflicts:
        assert np.diff(want["drop"]["track_off"]).tolist() == sorted(sizes, key=lambda s: comps[sizes.index(s)][0])
    monkeypatch.setenv("BA_DEBUG_TRACK_SEG", "64")
    with hb.Solver(0) as small:
        monkeypatch.delenv("BA_DEBUG_TRACK_SEG")
        for c in ("drop", "first"):
            lowered = small.build_tracks(kp_counts, a, b, conflict=c)
            default = solver.build_tracks(kp_counts, a, b, conflict=c)
            R.assert_same(lowered, want[c], what=f"BA_DEBUG_TRACK_SEG=64 {c}: ")
            R.assert_same(default, want[c], what=f"default {c}: ")
            R.assert_same(lowered, default)


# ------------------------------------------------------------------------------------------------ chain depth
@pytest.mark.parametrize("order", ["shuffled", "far_end_first", "random_numbering"])
def test_a_path_of_2000_nodes(solver, order):
    n = 2000
    rng = np.random.default_rng(2000)
    kp_counts = np.ones(n, dtype=np.int64)                  # one node per image: no conflict anywhere
    a, b = np.arange(n - 1, dtype=np.int32), np.arange(1, n, dtype=np.int32)
    if order == "shuffled":
        p = rng.permutation(n - 1); a, b = a[p], b[p]
    elif order == "far_end_first":
        a, b = b[::-1].copy(), a[::-1].copy()
    else:                                                   # the path visits the nodes in a random order: many local minima, long chains of retries
        name = rng.permutation(n).astype(np.int32); a, b = name[a], name[b]
    out = check(solver, kp_counts, a, b)
    assert not out["node_label"].any() and out["counts"]["tracks"] == 1
    assert np.array_equal(out["track_node"], np.arange(n)) and out["track_off"].tolist() == [0, n]
    print(f"{order}: {out['counts']['rounds']} hook rounds, cap {round_cap(n)}")
    assert out["counts"]["rounds"] == 2                     # (a lane leaves the first round only with its edge joined)


@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_a_star_with_the_hub_as_its_largest_node(solver, order):
    """One keypoint of the last image matched into 2000 earlier images: every lane of the first hook round contends for the hub's
    parent word, and only one link can go in there.  A lane that loses must go on until its edge is joined, or a schedule exists
    that needs a round per leaf.  Two rounds, whatever the edge order, and the yardstick's arrays."""
    k = 2000
    kp_counts = np.ones(k + 1, dtype=np.int64)
    leaves = np.arange(k, dtype=np.int32)
    if order == "descending":
        leaves = leaves[::-1].copy()
    elif order == "shuffled":
        leaves = np.random.default_rng(k).permutation(k).astype(np.int32)
    hub = np.full(k, k, dtype=np.int32)
    for a, b in ((hub, leaves), (leaves, hub)):
        out = check(solver, kp_counts, a, b)
        assert not out["node_label"].any() and out["counts"]["tracks"] == 1 and np.array_equal(out["track_node"], np.arange(k + 1))
        print(f"{order}: {out['counts']['rounds']} hook rounds, cap {round_cap(k + 1)}")
        assert out["counts"]["rounds"] == 2
    # the same hub inside a larger graph: stars of 2 .. 300 leaves around high-numbered hubs, leaves shared between neighbouring stars
    rng = np.random.default_rng(order == "ascending")
    n = 3000
    kp_counts = np.ones(n, dtype=np.int64)
    ea, eb = [], []
    for h in range(n - 1, n - 21, -1):
        m = int(rng.integers(2, 301))
        ea.append(np.full(m, h)); eb.append(rng.choice(n - 20, size=m, replace=False))
    ea, eb = np.concatenate(ea).astype(np.int32), np.concatenate(eb).astype(np.int32)
    o = np.argsort(eb)[::-1] if order == "descending" else (np.argsort(eb) if order == "ascending" else rng.permutation(len(ea)))
    out = check(solver, kp_counts, ea[o], eb[o])
    assert out["counts"]["rounds"] <= 2


def test_max_rounds_is_a_safety_net_that_reports(hb, solver):
    kp_counts = np.ones(64, dtype=np.int64)
    name = np.random.default_rng(3).permutation(64).astype(np.int32)
    with pytest.raises(hb.BAHipError, match="BA_ERR_INTERNAL.*max_rounds"):
        solver.build_tracks(kp_counts, name[:-1], name[1:], max_rounds=1)
    check(solver, kp_counts, name[:-1], name[1:])           # the handle is fine afterwards


# ------------------------------------------------------------------------------------------------ invariance
@pytest.fixture(scope="module")
def big_graph():
    """About 5000 nodes in 700 components of 2 .. 12 nodes over 40 images, about 20 000 edges, a conflict planted in every tenth
    component; and the yardstick's answers under both policies."""
    rng = np.random.default_rng(5000)
    sizes = rng.integers(2, 13, 700).tolist()
    kp_counts, a, b, _ = R.planted_graph(rng, sizes, 40, conflicts=set(range(0, 700, 10)), extra_nodes=100, extra_per_node=3.0)
    assert 4500 < kp_counts.sum() < 5500 and 17000 < len(a) < 23000
    want = {c: R.build(kp_counts, a, b, conflict=c) for c in ("drop", "first")}
    assert want["drop"]["counts"]["conflict_components"] >= 60
    return kp_counts, a, b, want


@pytest.mark.parametrize("conflict", ["drop", "first"])
def test_the_result_depends_on_the_edge_set_only(solver, big_graph, conflict):
    kp_counts, a, b, want = big_graph
    rng = np.random.default_rng(1)
    n = int(kp_counts.sum())
    base = solver.build_tracks(kp_counts, a, b, conflict=conflict)
    R.assert_same(base, want[conflict])
    R.assert_same(solver.build_tracks(kp_counts, a, b, conflict=conflict), base, what="again: ")
    p = rng.permutation(len(a))
    R.assert_same(solver.build_tracks(kp_counts, a[p], b[p], conflict=conflict), base, what="permuted: ")
    R.assert_same(solver.build_tracks(kp_counts, b, a, conflict=conflict), base, what="reversed: ")
    twice = solver.build_tracks(kp_counts, np.tile(a, 2), np.tile(b, 2), conflict=conflict)
    R.assert_same(twice, base, what="twice: ", skip=("same_image_edges",))      # (that one counts edges, duplicates included)
    assert twice["counts"]["same_image_edges"] == 2 * base["counts"]["same_image_edges"] > 0
    extra = int(0.3 * len(a))
    xa, xb = rng.integers(0, n, extra).astype(np.int32), rng.integers(0, n, extra).astype(np.int32)
    where = rng.permutation(len(a) + extra)
    keep = (where < len(a)).astype(np.uint8)
    ma, mb = np.concatenate([a, xa])[where], np.concatenate([b, xb])[where]
    R.assert_same(solver.build_tracks(kp_counts, ma, mb, keep, conflict=conflict), base, what="masked: ")


# ------------------------------------------------------------------------------------------------ policies
def test_policies_on_a_hand_made_graph(solver):
    names = R.STATUS
    # images: 0 -> nodes 0 1 2, 1 -> 3 4, 2 -> (none), 3 -> 5 6 7
    kp = [3, 2, 0, 3]
    a = np.array([0, 3, 1, 4, 2, 2, 6], dtype=np.int32)
    b = np.array([3, 5, 4, 6, 2, 1, 1], dtype=np.int32)      # 0-3-5 | 1-4-6-1 | 2-2 (self) | 2-1 (same image); 7 isolated
    out = check(solver, kp, a, b)
    assert out["track_node"].tolist() == [0, 3, 5, 1, 4, 6] and out["counts"]["same_image_edges"] == 2
    assert out["node_status"].tolist() == [0, 0, names["isolated"], 0, 0, 0, 0, names["isolated"]]
    without = check(solver, kp, a[[0, 1, 2, 3, 6]], b[[0, 1, 2, 3, 6]])
    for k in R.ARRAYS:
        assert np.array_equal(out[k], without[k]), k         # same-image and self edges change nothing
    # join the two through 5-4: nodes 0 and 1 of image 0 (and 3, 4 of image 1; 5, 6 of image 3) in one component
    a2, b2 = np.append(a, 5).astype(np.int32), np.append(b, 4).astype(np.int32)
    drop = check(solver, kp, a2, b2, conflict="drop")
    assert drop["counts"]["tracks"] == 0 and drop["node_status"].tolist() == [2, 2, 1, 2, 2, 2, 2, 1]
    first = check(solver, kp, a2, b2, conflict="first")
    assert first["track_node"].tolist() == [0, 3, 5] and first["node_status"].tolist() == [0, 2, 1, 0, 2, 0, 2, 1]
    # 0-3, 3-1: FIRST keeps {0, 3}: two nodes, short of min_length = 3
    short = check(solver, kp, np.array([0, 3], dtype=np.int32), np.array([3, 1], dtype=np.int32), conflict="first", min_length=3)
    assert short["node_status"].tolist()[:4] == [names["short"], names["conflict"], names["isolated"], names["short"]]
    assert short["counts"]["short_components"] == 1 and short["counts"]["tracks"] == 0 and (short["node_track"] == -1).all()


# ------------------------------------------------------------------------------------------------ edges of the domain
def test_empty_inputs(solver):
    none = np.zeros(0, dtype=np.int32)
    out = check(solver, [3, 0, 4], none, none)               # n_edges = 0
    assert out["counts"]["rounds"] == 0 and (out["node_status"] == R.STATUS["isolated"]).all() and out["track_off"].tolist() == [0]
    assert out["node_label"].tolist() == list(range(7))
    for kp in ([], [0, 0]):                                  # N = 0
        out = check(solver, kp, none, none)
        assert out["node_label"].shape == (0,) and out["track_off"].tolist() == [0] and out["counts"]["tracks"] == 0
    # an image without keypoints in the middle; all edges masked
    a, b = np.array([0, 2, 3, 6], dtype=np.int32), np.array([3, 5, 4, 1], dtype=np.int32)
    out = check(solver, [3, 0, 4], a, b)
    assert out["counts"]["tracks"] == 3 and out["counts"]["same_image_edges"] == 1      # {0, 3} {1, 6} {2, 5}; 3-4 lies in image 2
    masked = check(solver, [3, 0, 4], a, b, np.zeros(4, dtype=np.uint8))
    assert masked["counts"]["tracks"] == 0 and (masked["node_status"] == R.STATUS["isolated"]).all()


def _raw(hb, solver, kp_off, a, b, keep, opts, null=None):
    """The C call with caller-made arrays; `null` names one pointer argument passed as NULL.  -> (rc, message)."""
    lib = hb.load_library()
    kp_off = np.asarray(kp_off, dtype=np.int64)
    a, b = np.asarray(a, dtype=np.int32), np.asarray(b, dtype=np.int32)
    n = 16
    label, track, node = (np.zeros(n, dtype=np.int32) for _ in range(3))
    status, track_off, counts = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.int64), np.zeros(8, dtype=np.int64)
    p64, p8, ip = C.POINTER(C.c_int64), C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
    args = dict(kp_off=kp_off.ctypes.data_as(p64), edge_a=a.ctypes.data_as(ip), edge_b=b.ctypes.data_as(ip),
                edge_keep=None if keep is None else keep.ctypes.data_as(p8), opts=C.byref(opts), node_label=label.ctypes.data_as(ip),
                node_track=track.ctypes.data_as(ip), node_status=status.ctypes.data_as(p8), track_off=track_off.ctypes.data_as(p64),
                track_node=node.ctypes.data_as(ip), counts=counts.ctypes.data_as(p64))
    if null:
        args[null] = None
    rc = lib.ba_build_tracks(solver._h, len(kp_off) - 1, args["kp_off"], len(a), args["edge_a"], args["edge_b"], args["edge_keep"], args["opts"],
                             args["node_label"], args["node_track"], args["node_status"], args["track_off"], args["track_node"], args["counts"])
    return rc, lib.ba_last_error().decode()


def test_refusals_name_the_argument(hb, solver):
    ok = hb.BATrackBuildOptions(2, 0, 0, 0)
    kp_off, a, b = [0, 2, 4], [0, 1], [2, 3]
    assert _raw(hb, solver, kp_off, a, b, None, ok)[0] == 0
    for name in ("kp_off", "edge_a", "edge_b", "opts", "node_label", "node_track", "node_status", "track_off", "track_node", "counts"):
        rc, msg = _raw(hb, solver, kp_off, a, b, None, ok, null=name)
        assert rc == -1 and name in msg, (name, msg)
    for bad_off, word in (([1, 2, 4], "kp_off"), ([0, 3, 2], "kp_off"), ([0, 1 << 31], "N")):
        rc, msg = _raw(hb, solver, bad_off, [], [], None, ok)
        assert rc == -1 and word in msg and "kp_off" in msg, msg
    for opts, word in ((hb.BATrackBuildOptions(1, 0, 0, 0), "min_length"), (hb.BATrackBuildOptions(2, 2, 0, 0), "conflict"),
                       (hb.BATrackBuildOptions(2, -1, 0, 0), "conflict")):
        rc, msg = _raw(hb, solver, kp_off, a, b, None, opts)
        assert rc == -1 and word in msg, msg
    with pytest.raises(ValueError, match="conflict"):
        solver.build_tracks([2, 2], a, b, conflict="nope")
    # an end out of range: found on the device, the smallest offending edge is named
    rng = np.random.default_rng(9)
    kp_counts = [300, 300]
    ea, eb = rng.integers(0, 300, 700).astype(np.int32), rng.integers(300, 600, 700).astype(np.int32)
    eb[650] = 600; ea[311] = -1; eb[640] = 1 << 30
    with pytest.raises(hb.BAHipError, match=r"edge 311\b"):
        solver.build_tracks(kp_counts, ea, eb)
    keep = np.ones(700, dtype=np.uint8); keep[311] = 0       # a removed edge is not examined
    with pytest.raises(hb.BAHipError, match=r"edge 640\b"):
        solver.build_tracks(kp_counts, ea, eb, keep)
    keep[[640, 650]] = 0
    check(solver, kp_counts, np.where(keep, ea, 0), np.where(keep, eb, 0), keep)


# ------------------------------------------------------------------------------------------------ end to end
def test_matches_to_an_adjusted_scene(solver):
    """6 cameras, 200 points, 4 views each.  Keypoints: the points' observations, shuffled per image.  Matches: the true
    correspondences of every image pair plus 8 wrong ones, each joining two different points (16 points touched).  Every untouched
    point must come back as exactly one track with exactly its observations; every touched point as `conflict` under DROP (two
    points of 4 views among 6 cameras share a camera).  Then to_problem -> triangulate_tracks(write=True) -> filter_tracks ->
    solve, against the same scene built from the ground-truth pt_idx: the untouched points in the tracks' order.

    What carries the check: the per-point assertions on the tracks, the array equality of the two problems (the tracks give
    exactly the observations the ground truth gives, point for point and row for row), and an adjusted RMSE below one pixel for
    N(0, 0.5) noise.  The RMSE comparison itself then runs two solves on equal input: tests/test_gpu_tracks.py compares two solves
    of one scene without a tolerance (equal summaries on equal input; `rmse2 < rmse1` otherwise), so it is `<=` with no slack here,
    and what it can still catch is a solve that depends on something other than its input."""
    from bundle_adjustment_amd import tracks as T
    from bundle_adjustment_amd.problem import BAProblem
    from bundle_adjustment_amd.synthetic import make_problem
    from bundle_adjustment_amd.triangulation import filter_tracks, triangulate_tracks
    rng = np.random.default_rng(6)
    prob = make_problem(6, 200, 4, seed=21)
    n_cams, n_pts = 6, 200
    rows = [rng.permutation(np.nonzero(prob.cam_idx == i)[0]) for i in range(n_cams)]      # observation rows, in keypoint order
    keypoints = [prob.uv[r] for r in rows]
    kp_of = -np.ones((n_cams, n_pts), dtype=np.int64)                                       # keypoint of point p in image i
    for i, r in enumerate(rows):
        kp_of[i, prob.pt_idx[r]] = np.arange(len(r))
    pairs = []
    for i in range(n_cams):
        for j in range(i + 1, n_cams):
            both = np.nonzero((kp_of[i] >= 0) & (kp_of[j] >= 0))[0]
            pairs.append((i, j, kp_of[i, both], kp_of[j, both]))
    touched = rng.choice(n_pts, size=16, replace=False)
    for p, q in touched.reshape(8, 2):
        i = int(rng.choice(np.nonzero(kp_of[:, p] >= 0)[0]))
        j = int(rng.choice([c for c in np.nonzero(kp_of[:, q] >= 0)[0] if c != i]))
        pairs.append((i, j, [kp_of[i, p]], [kp_of[j, q]]))
    order = rng.permutation(len(pairs))
    tr = T.build_tracks([len(r) for r in rows], [pairs[k] for k in order], solver=solver)
    kp_off = tr["kp_off"]
    clean = np.setdiff1d(np.arange(n_pts), touched)
    assert tr["counts"]["tracks"] == len(clean) and tr["counts"]["conflict_components"] == 8
    for p in range(n_pts):
        imgs = np.nonzero(kp_of[:, p] >= 0)[0]
        nodes = kp_off[imgs] + kp_of[imgs, p]
        if p in touched:
            assert (tr["node_status"][nodes] == R.STATUS["conflict"]).all() and (tr["node_track"][nodes] == -1).all()
        else:
            t = tr["node_track"][nodes[0]]
            assert t >= 0 and np.array_equal(tr["track_node"][tr["track_off"][t]:tr["track_off"][t + 1]], nodes)
    from_tracks = T.to_problem(tr, keypoints, prob.cams, prob.K4)
    # the ground truth's build of the same scene: point t = the true point whose first observation is track t's first member
    first_nodes = np.array([kp_off[np.argmax(kp_of[:, p] >= 0)] + kp_of[np.argmax(kp_of[:, p] >= 0), p] for p in clean])
    truth_pts = clean[np.argsort(first_nodes)]
    new_of_old = -np.ones(n_pts, dtype=np.int64); new_of_old[truth_pts] = np.arange(len(truth_pts))
    sel = np.nonzero(new_of_old[prob.pt_idx] >= 0)[0]
    sel = sel[np.lexsort((prob.cam_idx[sel], new_of_old[prob.pt_idx[sel]]))]                 # by point, then by camera
    from_truth = BAProblem(prob.cams, np.zeros((len(truth_pts), 3)), prob.cam_idx[sel], new_of_old[prob.pt_idx[sel]].astype(np.int32),
                           prob.uv[sel], prob.K4, 0).validate()
    for k in ("cam_idx", "pt_idx", "uv"):
        assert np.array_equal(getattr(from_tracks, k), getattr(from_truth, k)), k
    rmse = {}
    for name, p0 in (("tracks", from_tracks), ("truth", from_truth)):
        out, merged = triangulate_tracks(p0, solver=solver, write=True, max_reproj_px=50.0)
        kept, _ = filter_tracks(merged, out["status"] == 0)
        assert kept.n_pts >= 0.9 * len(clean)
        solver.set_problem(kept)
        s = solver.solve(loss="huber", max_iters=15)
        rmse[name] = float(np.sqrt(s["final_sse"] / kept.n_obs))
    print(f"rmse from tracks {rmse['tracks']:.6f} px, from the ground truth {rmse['truth']:.6f} px")
    assert rmse["tracks"] < 1.0                              # (pixel noise is N(0, 0.5) per coordinate)
    assert rmse["tracks"] <= rmse["truth"]
