"""The yardstick of ba_build_tracks in plain numpy: labels by repeated np.minimum.at over the kept edges until nothing
changes, then the bookkeeping exactly as include/ba_hip.h defines it.  Shares no code with bundle_adjustment_amd/tracks.py.

`mutant` deliberately breaks one rule (tests/test_trackbuild_host.py checks that each break is caught):
  "no_conflicts"   conflicts ignored
  "scatter_order"  members listed in a scrambled order instead of ascending
  "by_size"        tracks numbered by descending size instead of ascending label"""
import numpy as np

STATUS = {"in_track": 0, "isolated": 1, "conflict": 2, "short": 3}
COUNTS = ("tracks", "members", "components", "conflict_components", "conflict_nodes", "short_components", "same_image_edges", "rounds")


def offsets(kp_counts):
    off = np.zeros(len(kp_counts) + 1, dtype=np.int64)
    off[1:] = np.cumsum(np.asarray(kp_counts, dtype=np.int64))
    return off


def image_of(kp_off, nodes):
    return np.searchsorted(kp_off, nodes, side="right") - 1


def build(kp_counts, edge_a, edge_b, edge_keep=None, min_length=2, conflict="drop", mutant=None):
    kp_off = offsets(kp_counts)
    assert (np.diff(kp_off) >= 0).all(), "keypoint counts are not negative"
    n = int(kp_off[-1])
    a = np.asarray(edge_a, dtype=np.int64).reshape(-1)
    b = np.asarray(edge_b, dtype=np.int64).reshape(-1)
    if edge_keep is not None:
        k = np.asarray(edge_keep).reshape(-1) != 0
        a, b = a[k], b[k]
    assert ((a >= 0) & (a < n) & (b >= 0) & (b < n)).all(), "the yardstick takes valid edges only"
    img = image_of(kp_off, np.arange(n))
    same = img[a] == img[b]
    same_edges = int(same.sum())
    a, b = a[~same], b[~same]
    label = np.arange(n, dtype=np.int64)
    while True:
        new = label.copy()
        np.minimum.at(new, a, label[b])
        np.minimum.at(new, b, label[a])
        new = np.minimum(new, new[new])
        if np.array_equal(new, label):
            break
        label = new
    node_track = np.full(n, -1, dtype=np.int32)
    status = np.full(n, STATUS["isolated"], dtype=np.uint8)
    size = np.bincount(label, minlength=n)
    roots = np.nonzero((label == np.arange(n)) & (size >= 2))[0]
    counts = dict.fromkeys(COUNTS, 0)
    counts["components"] = len(roots)
    counts["same_image_edges"] = same_edges
    tracks = []
    for r in roots:                                         # ascending label
        mem = np.nonzero(label == r)[0]                     # ascending node
        dup = np.zeros(len(mem), dtype=bool)
        dup[1:] = img[mem[1:]] == img[mem[:-1]]             # an image's nodes are contiguous: duplicates are neighbours
        if mutant == "no_conflicts":
            dup[:] = False
        if dup.any():
            counts["conflict_components"] += 1
            if conflict == "drop":
                counts["conflict_nodes"] += len(mem)
                status[mem] = STATUS["conflict"]
                continue
            counts["conflict_nodes"] += int(dup.sum())
            status[mem[dup]] = STATUS["conflict"]
            mem = mem[~dup]
        if len(mem) < min_length:
            counts["short_components"] += 1
            status[mem] = STATUS["short"]
            continue
        tracks.append(mem)
    if mutant == "by_size":
        tracks.sort(key=lambda m: -len(m))                  # (stable: equal sizes stay in label order)
    if mutant == "scatter_order":
        tracks = [np.concatenate([m[:1], m[1:][::-1]]) for m in tracks]
    for t, mem in enumerate(tracks):
        node_track[mem] = t
        status[mem] = STATUS["in_track"]
    track_off = np.zeros(len(tracks) + 1, dtype=np.int64)
    track_off[1:] = np.cumsum([len(m) for m in tracks])
    track_node = np.concatenate(tracks).astype(np.int32) if tracks else np.zeros(0, dtype=np.int32)
    counts["tracks"], counts["members"] = len(tracks), len(track_node)
    return dict(kp_off=kp_off, node_label=label.astype(np.int32), node_track=node_track, node_status=status, track_off=track_off,
                track_node=track_node, counts=counts)


ARRAYS = ("kp_off", "node_label", "node_track", "node_status", "track_off", "track_node")


def assert_same(got, want, what="", skip=()):
    """Exact equality on every array and every count except the round count (and the counts named in `skip`)."""
    for k in ARRAYS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape and np.array_equal(g, w), f"{what}{k}: {g[:12]} ... vs {w[:12]} ..."
    for k in COUNTS[:-1]:
        if k in skip:
            continue
        assert int(got["counts"][k]) == int(want["counts"][k]), f"{what}counts[{k}]: {got['counts'][k]} vs {want['counts'][k]}"


def random_graph(rng, n_images, max_kp, n_edges, p_same=0.05):
    """A small random match graph: kp_counts (some images may be empty), edges mostly between different images, a few
    inside one image or from a node to itself, duplicates likely."""
    kp_counts = rng.integers(0, max_kp + 1, n_images)
    n = int(kp_counts.sum())
    if n == 0:
        return kp_counts, np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32)
    a = rng.integers(0, n, n_edges).astype(np.int32)
    b = rng.integers(0, n, n_edges).astype(np.int32)
    selfs = rng.random(n_edges) < p_same
    b[selfs] = a[selfs]
    return kp_counts, a, b


def planted_graph(rng, sizes, n_images, conflicts=(), extra_nodes=0, extra_per_node=0.25):
    """Components of the given sizes, each a random spanning tree plus extra_per_node * size extra edges, each spread over as many images as
    it has nodes (image q of a component's q-th node, so sizes must not exceed n_images), except that for every index in
    `conflicts` two nodes of that component share an image.  Returns (kp_counts, edge_a, edge_b, node lists per component);
    the node numbering interleaves the components."""
    per_image = [[] for _ in range(n_images)]               # (component, slot) per keypoint of an image
    for c, s in enumerate(sizes):
        assert s <= n_images
        start = int(rng.integers(0, n_images))
        imgs = [(start + q) % n_images for q in range(s)]
        if c in conflicts:
            imgs[-1] = imgs[0]
        for q, i in enumerate(imgs):
            per_image[i].append((c, q))
    for _ in range(extra_nodes):
        per_image[int(rng.integers(0, n_images))].append((-1, 0))
    node_of = {}
    node = 0
    kp_counts = []
    for i in range(n_images):
        order = rng.permutation(len(per_image[i]))
        for o in order:
            c, q = per_image[i][o]
            if c >= 0:
                node_of[(c, q)] = node
            node += 1
        kp_counts.append(len(per_image[i]))
    ea, eb, comps = [], [], []
    for c, s in enumerate(sizes):
        nodes = [node_of[(c, q)] for q in range(s)]
        comps.append(sorted(nodes))
        perm = rng.permutation(s)
        for q in range(1, s):
            ea.append(nodes[perm[q]]); eb.append(nodes[perm[int(rng.integers(0, q))]])
        for _ in range(int(s * extra_per_node)):
            x, y = rng.integers(0, s, 2)
            ea.append(nodes[x]); eb.append(nodes[y])
    order = rng.permutation(len(ea))
    return np.array(kp_counts), np.array(ea, dtype=np.int32)[order], np.array(eb, dtype=np.int32)[order], comps
