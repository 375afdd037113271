"""Wall time of Solver.build_tracks on a synthetic match graph, next to the same job on the host (output kept in
profiles/trackbuild_times.txt).

    python tools/trackbuild_times.py [--out FILE] [--images N] [--keypoints N] [--pairs N] [--matches N] [--wrong F] [--reps N]

The graph (defaults: 2000 images x 3000 keypoints, 20 pairs per image, 500 matches per pair, 5 % of them wrong): every image
has `keypoints` lanes, a lane is cut along the image sequence into 3D points that live for a geometric number of images (mean
35), and a point's keypoint index in an image is a per-image permutation of its lane.  Image i is paired with i + 1 .. i + pairs;
a pair gets matches * (1 - wrong) true correspondences drawn among the points the two images share and matches * wrong edges
between random keypoints of the two.  Random wrong edges at that rate chain nearly every point into one giant component; a
second run with --wrong 0 semantics (the same graph without its wrong edges) shows the call on tracks that stay apart.

device   host wall time of Solver.build_tracks with every output copied back (median, min, max of --reps calls after one warm-up
         call; the call ends in a stream synchronise), and its hook rounds.
host     scipy.sparse.csgraph.connected_components plus the numpy bookkeeping of the definitions (labels = smallest node,
         members sorted by (label, node), conflicts between neighbours, policy, compaction), timed once.
The two results are compared array by array.  Recorded, not gated."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def match_graph(rng, n_images, n_kp, n_pairs, n_matches, wrong):
    """-> (kp_counts, edge_a, edge_b, is_wrong) as described above."""
    cut = rng.random((n_images, n_kp)) < 1.0 / 35.0
    point = np.cumsum(cut, axis=0, dtype=np.int32)                     # the lane's point at every image (lanes never share one)
    slot = rng.permuted(np.tile(np.arange(n_kp, dtype=np.int32), (n_images, 1)), axis=1)
    base = (np.arange(n_images, dtype=np.int64) * n_kp)[:, None]
    n_wrong = int(round(n_matches * wrong))
    n_true = n_matches - n_wrong
    ea, eb, ew = [], [], []
    for d in range(1, n_pairs + 1):
        if d >= n_images:
            break
        rows = n_images - d
        key = rng.random((rows, n_kp), dtype=np.float32)
        key[point[:-d] != point[d:]] = 2.0
        take = min(n_true, n_kp - 1)
        lanes = np.argpartition(key, take, axis=1)[:, :take]
        ok = np.take_along_axis(key, lanes, axis=1) < 2.0
        a = base[:rows] + np.take_along_axis(slot[:rows], lanes, axis=1)
        b = base[d:] + np.take_along_axis(slot[d:], lanes, axis=1)
        ea.append(a[ok]); eb.append(b[ok]); ew.append(np.zeros(int(ok.sum()), dtype=bool))
        if n_wrong:
            ea.append((base[:rows] + rng.integers(0, n_kp, (rows, n_wrong))).ravel())
            eb.append((base[d:] + rng.integers(0, n_kp, (rows, n_wrong))).ravel())
            ew.append(np.ones(rows * n_wrong, dtype=bool))
    order = rng.permutation(sum(len(x) for x in ea))
    return (np.full(n_images, n_kp, dtype=np.int64), np.concatenate(ea).astype(np.int32)[order], np.concatenate(eb).astype(np.int32)[order],
            np.concatenate(ew)[order])


def host_tracks(kp_counts, a, b, min_length=2, drop=True):
    """The definitions of ba_build_tracks with scipy's connected components and numpy: -> dict like Solver.build_tracks'."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    kp_off = np.concatenate([[0], np.cumsum(kp_counts)]).astype(np.int64)
    n = int(kp_off[-1])
    img = np.repeat(np.arange(len(kp_counts), dtype=np.int32), kp_counts)
    cross = img[a] != img[b]
    a, b = a[cross], b[cross]
    _, comp = connected_components(coo_matrix((np.ones(len(a), dtype=np.int8), (a, b)), shape=(n, n)), directed=False)
    smallest = np.full(comp.max() + 1 if n else 0, n, dtype=np.int64)
    np.minimum.at(smallest, comp, np.arange(n))
    label = smallest[comp]
    size = np.bincount(label, minlength=n)
    member = np.nonzero(size[label] >= 2)[0]                          # ascending node
    member = member[np.argsort(label[member], kind="stable")]         # by (label, node)
    lab = label[member]
    first = np.ones(len(member), dtype=bool)
    first[1:] = lab[1:] != lab[:-1]
    conf = np.zeros(len(member), dtype=bool)
    conf[1:] = ~first[1:] & (img[member[1:]] == img[member[:-1]])
    seg = np.cumsum(first) - 1
    n_seg = int(seg[-1]) + 1 if len(seg) else 0
    n_conf = np.bincount(seg[conf], minlength=n_seg)
    seg_len = np.bincount(seg, minlength=n_seg)
    kept = np.where(drop & (n_conf > 0), 0, seg_len - n_conf)
    is_track = kept >= min_length
    out = is_track[seg] & ~conf
    track_node = member[out].astype(np.int32)
    track_id = np.cumsum(is_track) - 1
    node_track = np.full(n, -1, dtype=np.int32)
    node_track[track_node] = track_id[seg[out]]
    status = np.ones(n, dtype=np.uint8)
    status[member] = np.where(out, 0, np.where((n_conf[seg] > 0) if drop else conf, 2, 3))
    track_off = np.concatenate([[0], np.cumsum(kept[is_track])]).astype(np.int64)
    return dict(node_label=label.astype(np.int32), node_track=node_track, node_status=status, track_off=track_off, track_node=track_node,
                largest=int(seg_len.max()) if n_seg else 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trackbuild_times.txt"))
    ap.add_argument("--images", type=int, default=2000)
    ap.add_argument("--keypoints", type=int, default=3000)
    ap.add_argument("--pairs", type=int, default=20)
    ap.add_argument("--matches", type=int, default=500)
    ap.add_argument("--wrong", type=float, default=0.05)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from bundle_adjustment_amd import hip_backend as hb
    lines = []

    def note(line):
        lines.append(line)
        print(line, flush=True)
    rng = np.random.default_rng(0)
    kp_counts, ea, eb, ew = match_graph(rng, a.images, a.keypoints, a.pairs, a.matches, a.wrong)
    note(f"graph: {a.images} images x {a.keypoints} keypoints = {int(kp_counts.sum())} nodes, {a.pairs} pairs per image, {a.matches} matches "
         f"per pair, {a.wrong:.0%} wrong: {len(ea)} edges")
    with hb.Solver(0) as s:
        for name, keep in (("with the wrong edges", None), ("without the wrong edges", (~ew).astype(np.uint8))):
            for conflict in ("drop", "first"):
                s.build_tracks(kp_counts, ea, eb, keep, conflict=conflict)
                w = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    out = s.build_tracks(kp_counts, ea, eb, keep, conflict=conflict)
                    w.append(time.perf_counter() - t0)
                c = out["counts"]
                note(f"device, {name}, {conflict}: wall {1e3 * float(np.median(w)):.1f} ms (min {1e3 * min(w):.1f}, max {1e3 * max(w):.1f}); "
                     f"{c['rounds']} hook rounds; {c['tracks']} tracks, {c['members']} members, {c['components']} components, "
                     f"{c['conflict_components']} with a conflict, {c['conflict_nodes']} nodes dropped for one")
                ha, hb_ = (ea, eb) if keep is None else (ea[keep != 0], eb[keep != 0])
                t0 = time.perf_counter()
                host = host_tracks(kp_counts, ha, hb_, drop=conflict == "drop")
                t_host = time.perf_counter() - t0
                same = all(np.array_equal(out[k], host[k]) for k in ("node_label", "node_track", "node_status", "track_off", "track_node"))
                note(f"host,   {name}, {conflict}: wall {1e3 * t_host:.1f} ms (scipy connected_components + numpy bookkeeping, once); "
                     f"largest component {host['largest']} nodes; device result {'equal' if same else 'DIFFERENT'}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
