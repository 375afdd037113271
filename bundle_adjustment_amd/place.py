"""Place recognition on top of the device calls (hip_backend.Solver.train_vocabulary / bow_transform / bow_score): which
earlier keyframe a new one revisits -- the loop_i, loop_j that posegraph.close_loop takes as given -- and which image pairs
of a collection are worth matching at all.  A binary bag of words as in DBoW2 and COLMAP's vocabulary-tree matcher.

    voc = Vocabulary.train(solver, training_descriptor_sets)       # or Vocabulary.load(path).upload(solver)
    db = KeyframeDatabase(solver)
    vec = bow_vector(solver, descriptors)
    candidates = db.loop_candidates(vec, ref_score=db.score_against(vec, len(db) - 1))
    db.add(vec)

Everything here is bookkeeping on the host; the arithmetic is the library's.
"""
from __future__ import annotations

import numpy as np

BOW_ONE = 1 << 30
MAX_BRANCHING, MAX_LEVELS, MAX_IDF = 32, 8, (1 << 17) - 1
_ARRAYS = ("child0", "n_child", "node_desc", "idf_q")


class Vocabulary:
    """A vocabulary tree: child0, n_child (n_nodes,) int32 (child0 = -1, n_child = 0 at a leaf), node_desc (n_nodes, desc_bytes)
    uint8, idf_q (n_words,) int32, one per leaf in node order.  Validated on construction with the library's rules
    (ba_vocab_set); a violation raises ValueError naming it."""

    def __init__(self, child0, n_child, node_desc, idf_q):
        self.child0 = np.ascontiguousarray(child0, dtype=np.int32)
        self.n_child = np.ascontiguousarray(n_child, dtype=np.int32)
        self.node_desc = np.ascontiguousarray(node_desc)
        self.idf_q = np.ascontiguousarray(idf_q, dtype=np.int32)
        self.validate()

    @property
    def n_nodes(self):
        return int(self.child0.shape[0])

    @property
    def n_words(self):
        return int((self.child0 < 0).sum())

    @property
    def desc_bytes(self):
        return int(self.node_desc.shape[1])

    @property
    def word_of_node(self):
        w = np.full(self.n_nodes, -1, dtype=np.int32)
        w[self.child0 < 0] = np.arange(self.n_words, dtype=np.int32)
        return w

    def validate(self):
        c0, nc, nd, idf = self.child0, self.n_child, self.node_desc, self.idf_q
        if nd.dtype != np.uint8 or nd.ndim != 2:
            raise ValueError(f"node_desc must be a 2-D uint8 array, not {nd.dtype} with shape {nd.shape}")
        if nd.shape[1] % 8 != 0 or not 8 <= nd.shape[1] <= 64:
            raise ValueError(f"desc_bytes {nd.shape[1]} is not a multiple of 8 in 8 .. 64")
        if c0.ndim != 1 or c0.shape[0] < 1 or nc.shape != c0.shape or nd.shape[0] != c0.shape[0]:
            raise ValueError("child0, n_child and node_desc must have one entry per node, and at least the root")
        depth = np.zeros(len(c0), dtype=np.int64)
        nxt = 1
        for n in range(len(c0)):
            if c0[n] < 0:
                if nc[n] != 0:
                    raise ValueError(f"n_child[{n}] = {nc[n]} at a leaf must be 0")
                continue
            if not 2 <= nc[n] <= MAX_BRANCHING:
                raise ValueError(f"n_child[{n}] = {nc[n]} is neither 0 nor in 2 .. {MAX_BRANCHING}")
            if c0[n] != nxt:
                raise ValueError(f"child0[{n}] = {c0[n]}: children are not breadth-first contiguous (expected {nxt})")
            if nc[n] > len(c0) - nxt:
                raise ValueError(f"the children of node {n} reach past n_nodes")
            if depth[n] + 1 > MAX_LEVELS:
                raise ValueError(f"depth of the children of node {n} exceeds {MAX_LEVELS}")
            depth[nxt:nxt + nc[n]] = depth[n] + 1
            nxt += int(nc[n])
        if nxt != len(c0):
            raise ValueError(f"node {nxt} is the child of no node")
        if idf.ndim != 1 or idf.shape[0] != self.n_words:
            raise ValueError(f"idf_q must have one entry per word ({self.n_words}), not shape {idf.shape}")
        if len(idf) and (idf.min() < 0 or idf.max() > MAX_IDF):
            raise ValueError(f"idf_q must lie in 0 .. {MAX_IDF}")

    @classmethod
    def from_dict(cls, d):
        return cls(*(d[k] for k in _ARRAYS))

    def as_dict(self):
        return {k: getattr(self, k) for k in _ARRAYS}

    @classmethod
    def train(cls, solver, sets, **opts):
        """Train on the descriptor sets (Solver.train_vocabulary); the result is resident on the solver and returned."""
        return cls.from_dict(solver.train_vocabulary(sets, **opts))

    def upload(self, solver):
        solver.set_vocabulary(self)
        return self

    def save(self, path):
        """The four arrays as a .npz (numpy's own format; DBoW2's files are not read or written)."""
        with open(path, "wb") as f:
            np.savez(f, **self.as_dict())

    @classmethod
    def load(cls, path):
        with np.load(path, allow_pickle=False) as z:
            missing = [k for k in _ARRAYS if k not in z.files]
            if missing:
                raise ValueError(f"{path}: not a vocabulary file (no {', '.join(missing)})")
            return cls(*(z[k] for k in _ARRAYS))


def stack_vectors(vectors):
    """The CSR dict (vec_off, vec_word, vec_val) of a list of (words, values) vectors."""
    off = np.zeros(len(vectors) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(w) for w, _ in vectors])
    cat = lambda i: (np.concatenate([np.asarray(v[i], dtype=np.int32) for v in vectors]) if vectors else np.zeros(0, dtype=np.int32))  # noqa: E731
    return dict(vec_off=off, vec_word=cat(0), vec_val=cat(1))


def split_vectors(csr):
    """The list of (words, values) vectors of a CSR dict as Solver.bow_transform returns it."""
    off = np.asarray(csr["vec_off"])
    return [(np.asarray(csr["vec_word"][off[i]:off[i + 1]], dtype=np.int32), np.asarray(csr["vec_val"][off[i]:off[i + 1]], dtype=np.int32))
            for i in range(len(off) - 1)]


def bow_vector(solver, descriptors, weighting="tf_idf"):
    """(words, values) of one image's descriptors under the solver's vocabulary."""
    return split_vectors(solver.bow_transform([descriptors], weighting=weighting))[0]


class KeyframeDatabase:
    """The bag-of-words vectors of the keyframes so far, in the order they were added; entry i is keyframe i."""

    def __init__(self, solver):
        self.solver = solver
        self.vectors = []

    def __len__(self):
        return len(self.vectors)

    def add(self, vec):
        """Append a (words, values) vector; returns its index."""
        w, v = np.asarray(vec[0], dtype=np.int32), np.asarray(vec[1], dtype=np.int32)
        if w.ndim != 1 or w.shape != v.shape:
            raise ValueError("a vector is a pair (words, values) of equal-length 1-D arrays")
        self.vectors.append((w, v))
        return len(self.vectors) - 1

    def query(self, vec, min_gap=0, top_k=10):
        """[(index, score)] of the best entries among all but the newest min_gap, score descending (ties: lower index first)."""
        if min_gap < 0:
            raise ValueError("min_gap must not be negative")
        end = len(self.vectors) - int(min_gap)
        if end <= 0:
            return []
        out = self.solver.bow_score(stack_vectors([vec]), stack_vectors(self.vectors), db_end=[end], top_k=top_k)
        return [(int(i), int(s)) for i, s in zip(out["top_idx"][0], out["top_score"][0]) if i >= 0]

    def score_against(self, vec, index):
        """The score of vec against entry `index` alone (ORB-SLAM's reference: the frame's own predecessor)."""
        if not 0 <= index < len(self.vectors):
            raise IndexError(f"no entry {index}")
        out = self.solver.bow_score(stack_vectors([vec]), stack_vectors([self.vectors[index]]), top_k=1, dense=True)
        return int(out["score"][0, 0])

    def loop_candidates(self, vec, ref_score, ratio=0.75, min_gap=0, top_k=10):
        """query() cut at ratio * ref_score in exact integer arithmetic (score * den >= ref_score * num for ratio = num / den
        with den = 2^20): the candidates that score at least `ratio` times what the frame scores against its own predecessor,
        which is ORB-SLAM's normalisation."""
        num = int(round(float(ratio) * (1 << 20)))
        return [(i, s) for i, s in self.query(vec, min_gap=min_gap, top_k=top_k) if (s << 20) >= int(ref_score) * num]


def pair_list(solver, vectors, top_k=10):
    """The image pairs an SfM run should match: every image scored against the earlier ones (db_end[q] = q), its top_k
    kept.  vectors: a CSR dict or a list of (words, values).  Returns a sorted list of (i, j), i < j, each pair once."""
    csr = vectors if isinstance(vectors, dict) else stack_vectors(list(vectors))
    n = len(csr["vec_off"]) - 1
    if n < 2:
        return []
    out = solver.bow_score(csr, csr, db_end=np.arange(n, dtype=np.int32), top_k=top_k)
    pairs = {(int(j), q) for q in range(n) for j in out["top_idx"][q] if j >= 0}
    return sorted(pairs)
