"""numpy restatement of ba_vocab_train, ba_bow_transform and ba_bow_score (include/ba_hip.h): the yardstick of the place
recognition tests.  Everything is integer arithmetic except the one log of the idf weights, so every device output is
compared with these by exact equality.

Training, per node at depth d < levels with member rows M, |M| >= min_split: slot j starts from the descriptor of the
member row x with the smallest key (draw(seed, d, j, x) & ~0xFFFFFF) | x (draw: tests/ransac_reference.py); a slot whose row
an earlier slot already drew is VOID: it takes part in no assignment and stays empty.  At most `iters` times: every member
goes to the slot with the smallest (Hamming distance, slot) over the slots that are not void; stop when no member's slot
changed; every non-empty slot's centre becomes the bitwise majority of its members (bit = 1 iff 2 count >= size), an empty
slot keeps its centre.  A closing assignment to the final centres; the non-empty slots become children in slot order, with
fewer than two the node stays a leaf.  Nodes are numbered breadth-first by (parent id, slot); leaves are the words, in node order.
"""
import math

import numpy as np

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
ROW_BITS = 24
ROW_MASK = (1 << ROW_BITS) - 1
BOW_ONE = 1 << 30
IDF_ONE = 4096
POP8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.int64)


def _mix(z):
    """The splitmix64 finaliser on uint64 arrays (arithmetic modulo 2^64)."""
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def draw_rows(seed, d, j, rows):
    """ransac_reference.draw(seed, d, j, x) for every x of rows, as uint64."""
    one = np.ones(1, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = _mix(one * np.uint64((int(seed) + GOLDEN) & M64))
        z = _mix(z + np.uint64(d))
        z = _mix(z + np.uint64(j))
        return _mix(z + (np.asarray(rows).astype(np.uint64) + np.uint64(1)) * np.uint64(GOLDEN))


def seed_rows(seed, d, k, members):
    """The row every slot of a node at depth d draws: the member x with the smallest (draw(seed, d, j, x) & ~0xFFFFFF) | x."""
    M = np.asarray(members, dtype=np.int64)
    return [int(((draw_rows(seed, d, j, M) & np.uint64(M64 ^ ROW_MASK)) | M.astype(np.uint64)).min()) & ROW_MASK for j in range(k)]


def hamming(a, b):
    """(len(a), len(b)) Hamming distances of uint8 rows."""
    return POP8[a[:, None, :] ^ b[None, :, :]].sum(axis=2)


def assign(desc, centres, usable):
    """The slot with the smallest (distance, slot) among the usable ones, per row."""
    key = hamming(desc, centres) * 64 + np.arange(centres.shape[0])[None, :]
    key[:, ~usable] = 1 << 40
    return np.argmin(key, axis=1)


def majority(rows):
    cnt = np.unpackbits(rows, axis=1).sum(axis=0)
    return np.packbits(2 * cnt >= rows.shape[0])


def stack(sets, width=None):
    """(desc uint8 (rows, B), set_off int64) of a list of descriptor sets."""
    arrs = [np.asarray(a, dtype=np.uint8) for a in sets]
    width = arrs[0].shape[1] if arrs else width
    off = np.zeros(len(arrs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([a.shape[0] for a in arrs])
    desc = np.concatenate(arrs, axis=0) if arrs else np.zeros((0, width), dtype=np.uint8)
    return np.ascontiguousarray(desc), off


def idf_of(n_sets, n_with):
    """floor(ln(N / N_i) * 4096 + 0.5); 0 for a word no set reaches."""
    return np.array([int(math.floor(math.log(n_sets / n) * IDF_ONE + 0.5)) if n > 0 else 0 for n in n_with], dtype=np.int32)


def train(sets, branching=10, levels=6, iters=10, min_split=0, seed=0, stats=None):
    """The vocabulary of the sets: dict(desc_bytes, n_nodes, n_words, branching, levels, child0, n_child, node_desc,
    word_of_node, idf_q, train_word).  stats (a dict) receives `capped`, the number of nodes that stopped at the iteration cap."""
    desc, set_off = stack(sets)
    rows, B = desc.shape
    k = int(branching)
    min_split = 2 * k if min_split == 0 else int(min_split)
    child0, n_child, node_desc, members = [-1], [0], [np.zeros(B, dtype=np.uint8)], [np.arange(rows, dtype=np.int64)]
    level, capped = [0], 0
    for d in range(int(levels)):
        nxt = []
        for n in level:
            M = members[n]
            if len(M) < min_split:
                continue
            dn = desc[M]
            centres, usable, seen = np.zeros((k, B), dtype=np.uint8), np.zeros(k, dtype=bool), set()
            for j, x in enumerate(seed_rows(seed, d, k, M)):
                centres[j] = desc[x]
                usable[j] = x not in seen
                seen.add(x)
            prev, stopped = None, False
            for _ in range(int(iters)):
                a = assign(dn, centres, usable)
                if prev is not None and np.array_equal(a, prev):
                    stopped = True
                    break
                prev = a
                for j in range(k):
                    if (a == j).any():
                        centres[j] = majority(dn[a == j])
            capped += 0 if stopped else 1
            a = assign(dn, centres, usable)
            full = [j for j in range(k) if (a == j).any()]
            if len(full) < 2:
                continue
            child0[n], n_child[n] = len(child0), len(full)
            for j in full:
                nxt.append(len(child0))
                child0.append(-1)
                n_child.append(0)
                node_desc.append(centres[j].copy())
                members.append(M[a == j])
        level = nxt
    if stats is not None:
        stats["capped"] = capped
    child0, n_child = np.array(child0, dtype=np.int32), np.array(n_child, dtype=np.int32)
    word_of_node = np.full(len(child0), -1, dtype=np.int32)
    leaves = np.flatnonzero(child0 < 0)
    word_of_node[leaves] = np.arange(len(leaves), dtype=np.int32)
    train_word = np.zeros(rows, dtype=np.int32)
    for n in leaves:
        train_word[members[n]] = word_of_node[n]
    set_of_row = np.searchsorted(set_off, np.arange(rows), side="right") - 1
    n_with = [len(np.unique(set_of_row[members[n]])) for n in leaves]
    return dict(desc_bytes=B, n_nodes=len(child0), n_words=len(leaves), branching=k, levels=int(levels), child0=child0, n_child=n_child,
                node_desc=np.array(node_desc, dtype=np.uint8).reshape(len(child0), B), word_of_node=word_of_node,
                idf_q=idf_of(len(set_off) - 1, n_with), train_word=train_word)


def depth_of(child0, n_child):
    depth = np.zeros(len(child0), dtype=np.int64)
    for n in range(len(child0)):
        if child0[n] >= 0:
            depth[child0[n]:child0[n] + n_child[n]] = depth[n] + 1
    return depth


def descend(vocab, desc):
    """The word of every row: at each inner node the child with the smallest (Hamming distance, slot)."""
    desc = np.asarray(desc, dtype=np.uint8)
    node = np.zeros(desc.shape[0], dtype=np.int64)
    child0, n_child, nd = vocab["child0"], vocab["n_child"], vocab["node_desc"]
    while True:
        inner = np.flatnonzero(child0[node] >= 0)
        if len(inner) == 0:
            break
        for n in np.unique(node[inner]):
            at = np.flatnonzero(node == n)
            cen = nd[child0[n]:child0[n] + n_child[n]]
            node[at] = child0[n] + assign(desc[at], cen, np.ones(len(cen), dtype=bool))
    return vocab["word_of_node"][node].astype(np.int32)


def transform(vocab, sets, weighting="tf_idf"):
    """dict(desc_word, vec_off, vec_word, vec_val) of the sets."""
    desc, set_off = stack(sets, vocab["desc_bytes"])
    word = descend(vocab, desc)
    off, vw, vv = [0], [], []
    for s in range(len(set_off) - 1):
        w, c = np.unique(word[set_off[s]:set_off[s + 1]], return_counts=True)
        a = [int(ci) * (IDF_ONE if weighting == "tf" else int(vocab["idf_q"][wi])) for wi, ci in zip(w, c)]
        A = sum(a)
        for wi, ai in zip(w, a):
            v = (ai << 30) // A if A > 0 else 0
            if v > 0:
                vw.append(int(wi))
                vv.append(v)
        off.append(len(vw))
    return dict(desc_word=word, vec_off=np.array(off, dtype=np.int64), vec_word=np.array(vw, dtype=np.int32),
                vec_val=np.array(vv, dtype=np.int32))


def vector(csr, i):
    """(words, values) of vector i of a CSR dict."""
    a, b = int(csr["vec_off"][i]), int(csr["vec_off"][i + 1])
    return csr["vec_word"][a:b], csr["vec_val"][a:b]


def score_pair(wq, vq, wd, vd):
    _, iq, idd = np.intersect1d(wq, wd, assume_unique=True, return_indices=True)
    return int(np.minimum(vq[iq].astype(np.int64), vd[idd].astype(np.int64)).sum())


def score(query, db, db_end=None, top_k=10):
    """dict(score int32 (nq, nd), top_idx, top_score int32 (nq, top_k))."""
    nq, nd = len(query["vec_off"]) - 1, len(db["vec_off"]) - 1
    dense = np.zeros((nq, nd), dtype=np.int32)
    top_idx, top_score = np.full((nq, top_k), -1, dtype=np.int32), np.zeros((nq, top_k), dtype=np.int32)
    for q in range(nq):
        end = nd if db_end is None else min(nd, max(0, int(db_end[q])))
        wq, vq = vector(query, q)
        for j in range(end):
            dense[q, j] = score_pair(wq, vq, *vector(db, j))
        order = sorted((j for j in range(end) if dense[q, j] > 0), key=lambda j: (-int(dense[q, j]), j))[:top_k]
        top_idx[q, :len(order)] = order
        top_score[q, :len(order)] = dense[q, order]
    return dict(score=dense, top_idx=top_idx, top_score=top_score)


def _seed_drawing(rows, wanted):
    return next(s for s in range(4096) if sorted(seed_rows(s, 0, 2, np.arange(rows))) == wanted)


def majority_tie_case(width=8):
    """(rows, options): x, x, ~x, ~x under k = 2, one level, ONE iteration, at the first seed whose two slots draw the rows 0 and
    1 (both x).  All four rows then sit in slot 0 (the ~x rows by the assignment tie), its centre becomes the majority of
    x, x, ~x, ~x -- every bit a tie, so all ones -- and the closing assignment sends x to slot 1 (centre x): the children are
    all-ones and x."""
    x = np.random.default_rng(5).integers(0, 256, size=width, dtype=np.uint8)
    x[0] = 0x0f                         # (neither all zeros nor all ones)
    rows = np.stack([x, x, ~x, ~x])
    return rows, dict(branching=2, levels=1, iters=1, min_split=2, seed=_seed_drawing(4, [0, 1]))


def assign_tie_case(width=8):
    """(rows, options): all zeros, all ones and a row of alternating bits (4 width bits from either), k = 2, one level, at the
    first seed whose slots draw the rows 0 and 1: the third row is equidistant and goes to the lower slot."""
    rows = np.stack([np.zeros(width, np.uint8), np.full(width, 255, np.uint8), np.full(width, 0x55, np.uint8)])
    return rows, dict(branching=2, levels=1, iters=10, min_split=2, seed=_seed_drawing(3, [0, 1]))


def random_vectors(rng, n, n_words=300, nnz=40, empty=()):
    """A CSR dict of n L1-normalised vectors of about nnz words each; the ones listed in `empty` have no entry."""
    off, vw, vv = [0], [], []
    for i in range(n):
        if i not in empty:
            w = np.unique(rng.integers(0, n_words, size=nnz))
            a = rng.integers(1, 1000, size=len(w))
            v = (a.astype(np.int64) << 30) // int(a.sum())
            vw += w[v > 0].tolist()
            vv += v[v > 0].tolist()
        off.append(len(vw))
    return dict(vec_off=np.array(off, dtype=np.int64), vec_word=np.array(vw, dtype=np.int32), vec_val=np.array(vv, dtype=np.int32))


def join_vectors(parts):
    """The CSR dict of a list of (words, values)."""
    off = np.zeros(len(parts) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(w) for w, _ in parts])
    cat = lambda k: np.concatenate([p[k] for p in parts]).astype(np.int32) if parts else np.zeros(0, dtype=np.int32)  # noqa: E731
    return dict(vec_off=off, vec_word=cat(0), vec_val=cat(1))


def take_vectors(csr, idx):
    """The CSR dict of the vectors idx of csr, in that order."""
    return join_vectors([vector(csr, i) for i in idx])


class YardstickSolver:
    """Stand-in for hip_backend.Solver's place recognition methods, backed by the functions above: lets the host-side
    bookkeeping of bundle_adjustment_amd.place be tested where there is no GPU.  Test infrastructure only."""

    def __init__(self):
        self.vocab = None
        self.score_calls = []

    def train_vocabulary(self, sets, **opts):
        self.vocab = train(sets, **opts)
        return dict(self.vocab)

    def set_vocabulary(self, vocab):
        get = vocab.get if isinstance(vocab, dict) else lambda k: getattr(vocab, k)
        child0 = np.asarray(get("child0"), dtype=np.int32)
        word_of_node = np.full(len(child0), -1, dtype=np.int32)
        word_of_node[child0 < 0] = np.arange(int((child0 < 0).sum()), dtype=np.int32)
        node_desc = np.asarray(get("node_desc"), dtype=np.uint8)
        n_child = np.asarray(get("n_child"), dtype=np.int32)
        self.vocab = dict(desc_bytes=node_desc.shape[1], n_nodes=len(child0), n_words=int((child0 < 0).sum()), branching=int(n_child.max()),
                          levels=int(depth_of(child0, n_child).max()), child0=child0, n_child=n_child, node_desc=node_desc,
                          word_of_node=word_of_node, idf_q=np.asarray(get("idf_q"), dtype=np.int32))

    def vocabulary(self):
        return {k: v for k, v in self.vocab.items() if k != "train_word"}

    def vocabulary_size(self):
        return {k: self.vocab[k] for k in ("desc_bytes", "n_nodes", "n_words", "branching", "levels")}

    def bow_transform(self, sets, weighting="tf_idf"):
        return transform(self.vocab, list(sets), weighting=weighting)

    def bow_score(self, query, db, db_end=None, top_k=10, dense=False):
        self.score_calls.append(dict(nq=len(query["vec_off"]) - 1, nd=len(db["vec_off"]) - 1, db_end=None if db_end is None else list(db_end), top_k=top_k))
        out = score(query, db, db_end=db_end, top_k=top_k)
        if not dense:
            del out["score"]
        return out


def planted(n_places=12, pool=150, per_image=100, noise=30, flip=0.04, n_db=4, n_query=2, width=32, seed=0):
    """The planted retrieval data: (db sets, db place, query sets, query place)."""
    rng = np.random.default_rng(seed)
    pools = rng.integers(0, 256, size=(n_places, pool, width), dtype=np.uint8)

    def image(p):
        pick = pools[p][rng.choice(pool, size=per_image, replace=False)]
        flips = np.packbits(rng.random((per_image, width * 8)) < flip, axis=1)
        return np.concatenate([pick ^ flips, rng.integers(0, 256, size=(noise, width), dtype=np.uint8)], axis=0)

    db = [image(p) for p in range(n_places) for _ in range(n_db)]
    qs = [image(p) for p in range(n_places) for _ in range(n_query)]
    return db, np.repeat(np.arange(n_places), n_db), qs, np.repeat(np.arange(n_places), n_query)
