"""GPU: ba_vocab_train, ba_vocab_set / ba_vocab_get, ba_bow_transform and ba_bow_score against the numpy yardstick of
tests/bow_reference.py.  The arithmetic is integer: every comparison is exact equality on every output array.

Shapes.  T = 256 positions per tile of the training kernels; rows = 255, 256, 257 and 4 T + 1 put nodes across tile borders, and
(k, L) = (2, 8) on 600 rows reaches the deepest level with nodes of a few rows each.  The score's database chunk is
hip_backend.BOW_CHUNK vectors; BA_DEBUG_BOW_CHUNK=64 makes nd = 65 and 200 cross chunks."""
import os

import numpy as np
import pytest

from tests import bow_reference as B

pytestmark = pytest.mark.gpu
TREE = ("n_nodes", "n_words", "child0", "n_child", "node_desc", "word_of_node", "idf_q", "train_word")
CSR = ("vec_off", "vec_word", "vec_val")


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


@pytest.fixture(scope="module")
def planted():
    """The planted retrieval data (bow_reference.planted) and the yardstick's answers, computed once: 48 database images (the training
    sets) and 24 queries of 130 rows, vocabulary (k, L) = (10, 3), iters 10, min_split 2, seed 7."""
    db, db_place, qs, q_place = B.planted()
    opts = dict(branching=10, levels=3, iters=10, min_split=2, seed=7)
    vocab = B.train(db, **opts)
    vq, vd = B.transform(vocab, qs), B.transform(vocab, db)
    return dict(db=db, qs=qs, db_place=db_place, q_place=q_place, opts=opts, vocab=vocab, vq=vq, vd=vd, score=B.score(vq, vd, top_k=10))


def _rand(rng, n, width=32):
    return rng.integers(0, 256, (n, width), dtype=np.uint8)


def _split(rows, cuts):
    """rows cut into sets at the given row numbers (a repeated number gives a set with zero rows)."""
    edges = [0] + list(cuts) + [len(rows)]
    return [rows[a:b] for a, b in zip(edges[:-1], edges[1:])]


def _same(got, want, keys):
    for k in keys:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), k


def _train_check(solver, sets, **opts):
    got, want = solver.train_vocabulary(sets, **opts), B.train(sets, **opts)
    _same(got, want, TREE)
    assert (got["desc_bytes"], got["branching"], got["levels"]) == (want["desc_bytes"], want["branching"], want["levels"])
    return got, want


# ------------------------------------------------------------------------------------------------------------- 1: training
@pytest.mark.parametrize("min_split", [2, 0])
@pytest.mark.parametrize("iters", [1, 10])
@pytest.mark.parametrize("k,L,rows,width", [(3, 2, 200, 8), (3, 2, 200, 32), (3, 2, 200, 64), (2, 8, 600, 32)])
def test_training_equals_the_yardstick(solver, k, L, rows, width, iters, min_split):
    """Clustered rows (eight centres, 6 % of the bits flipped) so that the majority has something to find; five sets, one of
    them with zero rows."""
    rng = np.random.default_rng(10 + rows + width)
    centres = _rand(rng, 8, width)
    data = centres[rng.integers(0, 8, rows)] ^ np.packbits(rng.random((rows, width * 8)) < 0.06, axis=1)
    sets = _split(data, [rows // 5, rows // 2, rows // 2, rows - 7])
    assert any(len(s) == 0 for s in sets)
    got, want = _train_check(solver, sets, branching=k, levels=L, iters=iters, min_split=min_split, seed=3)
    assert want["n_words"] > k and B.depth_of(want["child0"], want["n_child"]).max() >= 2


def test_training_on_the_planted_data(solver, planted):
    got = solver.train_vocabulary(planted["db"], **planted["opts"])
    _same(got, planted["vocab"], TREE)
    assert got["n_words"] > 500


@pytest.mark.parametrize("rows", [1, 3, 255, 256, 257, 4 * 256 + 1])
def test_training_row_counts_across_tiles(solver, rows):
    """k = 4: rows = 1 and k - 1 = 3 cannot fill the slots; the others put the border between two nodes inside a tile."""
    rng = np.random.default_rng(rows)
    data = _rand(rng, 4, 32)[rng.integers(0, 4, rows)] ^ np.packbits(rng.random((rows, 256)) < 0.05, axis=1)
    _, want = _train_check(solver, _split(data, [rows // 3]), branching=4, levels=3, iters=10, min_split=2, seed=1)
    assert want["n_words"] == 1 if rows == 1 else want["n_words"] >= 2


def test_training_identical_rows_and_ties(solver):
    same = np.repeat(_rand(np.random.default_rng(4), 1, 32), 300, axis=0)
    got, _ = _train_check(solver, [same[:100], same[100:]], branching=5, levels=3, iters=10, min_split=2, seed=0)
    assert got["n_nodes"] == 1 and got["n_words"] == 1 and got["idf_q"].tolist() == [0]
    for w in ("tf_idf", "tf"):
        _same(solver.bow_transform([same[:7]], weighting=w), B.transform(got, [same[:7]], weighting=w), CSR + ("desc_word",))
    assert solver.bow_transform([same[:7]], weighting="tf")["vec_val"].tolist() == [1 << 30]
    assert len(solver.bow_transform([same[:7]])["vec_val"]) == 0
    rows, opts = B.majority_tie_case()
    got, _ = _train_check(solver, [rows], **opts)
    assert got["node_desc"][1].tolist() == [255] * 8 and np.array_equal(got["node_desc"][2], rows[0])
    rows, opts = B.assign_tie_case()
    got, _ = _train_check(solver, [rows], **opts)
    assert got["train_word"][2] == 0 and sorted(got["train_word"][:2].tolist()) == [0, 1]


def test_training_seeds_and_repeats(solver):
    data = _rand(np.random.default_rng(6), 500, 32)
    kw = dict(branching=4, levels=3, iters=10, min_split=2)
    a, _ = _train_check(solver, [data], seed=1, **kw)
    b, _ = _train_check(solver, [data], seed=2, **kw)
    again = solver.train_vocabulary([data], seed=1, **kw)
    _same(again, a, TREE)
    assert not np.array_equal(a["train_word"], b["train_word"])


def test_training_refusals(solver, hb):
    data = _rand(np.random.default_rng(7), 50, 32)
    for bad, name in ((dict(branching=1), "branching"), (dict(branching=33), "branching"), (dict(levels=0), "levels"), (dict(levels=9), "levels"),
                      (dict(iters=0), "iters"), (dict(min_split=1), "min_split")):
        with pytest.raises(hb.BAHipError, match=name):
            solver.train_vocabulary([data], **bad)
    with pytest.raises(hb.BAHipError, match="desc_bytes"):
        solver.train_vocabulary([data[:, :12]])


# ---------------------------------------------------------------------------------------------- 2: ba_vocab_set / ba_vocab_get
def _hand_tree():
    """Two levels over 8-byte descriptors: the root's children are all-zeros (a leaf, word 0) and all-ones (inner); the latter's
    are 0xff..f0 (word 1) and 0xff..ff (word 2)."""
    nd = np.zeros((5, 8), dtype=np.uint8)
    nd[2] = nd[3] = nd[4] = 255
    nd[3, 7] = 0xf0
    return dict(child0=np.array([1, -1, 3, -1, -1], np.int32), n_child=np.array([2, 0, 2, 0, 0], np.int32), node_desc=nd,
                idf_q=np.array([4096, 100, 300], np.int32))


def _chain(depth):
    """Two nodes per level, the first of them inner: 2 depth + 1 nodes, `depth` levels."""
    n = 2 * depth + 1
    child0, n_child = np.full(n, -1, np.int32), np.zeros(n, np.int32)
    for inner, first in [(0, 1)] + [(2 * d - 1, 2 * d + 1) for d in range(1, depth)]:
        child0[inner], n_child[inner] = first, 2
    return dict(child0=child0, n_child=n_child, node_desc=np.zeros((n, 8), np.uint8), idf_q=np.zeros(depth + 1, np.int32))


def test_vocabulary_round_trip_and_a_known_answer(solver):
    tree = _hand_tree()
    solver.set_vocabulary(tree)
    got = solver.vocabulary()
    _same(got, tree, ("child0", "n_child", "node_desc", "idf_q"))
    assert got["word_of_node"].tolist() == [-1, 0, -1, 1, 2] and (got["n_nodes"], got["n_words"], got["branching"], got["levels"]) == (5, 3, 2, 2)
    z, o, f0 = np.zeros(8, np.uint8), np.full(8, 255, np.uint8), np.array([255] * 7 + [0xf0], np.uint8)
    half = np.array([255] * 4 + [0] * 4, np.uint8)       # 32 bits from either child of the root: the tie goes to slot 0, word 0
    fa = np.array([255] * 7 + [0xfc], np.uint8)          # 2 bits from either leaf of the inner node: slot 0, word 1
    out = solver.bow_transform([np.stack([z, o, f0, half, fa, o])])
    assert out["desc_word"].tolist() == [0, 2, 1, 0, 1, 2]
    # counts 2, 2, 2 with idf 4096, 100, 300: a = 8192, 200, 600, A = 8992
    assert out["vec_word"].tolist() == [0, 1, 2] and out["vec_val"].tolist() == [(a << 30) // 8992 for a in (8192, 200, 600)]
    out = solver.bow_transform([np.stack([z, o, o])], weighting="tf")
    assert out["vec_word"].tolist() == [0, 2] and out["vec_val"].tolist() == [(1 << 30) // 3, (2 << 30) // 3]


def test_malformed_trees_are_refused_by_name(solver, hb):
    def broken(**kw):
        t = _hand_tree()
        for k, v in kw.items():
            t[k] = np.array(v, dtype=t[k].dtype)
        return t
    cases = [(broken(child0=[1, -1, 4, -1, -1]), "breadth-first contiguous"),
             (broken(child0=[2, -1, 3, -1, -1]), "breadth-first contiguous"),
             (broken(child0=[1, -1, -1, -1, -1], n_child=[2, 0, 0, 0, 0], idf_q=[1, 1, 1, 1]), "child of no node"),
             (broken(n_child=[2, 0, 1, 0, 0]), "n_child"),
             (broken(n_child=[2, 0, 33, 0, 0]), "n_child"),
             (broken(n_child=[2, 0, 3, 0, 0]), "reach past"),
             (broken(n_child=[2, 1, 2, 0, 0]), "n_child"),
             (broken(idf_q=[0, -1, 0]), "negative"),
             (broken(idf_q=[0, 1 << 17, 0]), "above")]
    cases.append((_chain(9), "depth"))
    solver.set_vocabulary(_hand_tree())
    for tree, name in cases:
        with pytest.raises(hb.BAHipError, match=name):
            solver.set_vocabulary(tree)
    assert solver.vocabulary_size()["n_nodes"] == 5           # a refused upload leaves the vocabulary as it was
    solver.set_vocabulary(_chain(8))                          # eight levels deep: accepted
    assert solver.vocabulary_size()["levels"] == 8 and solver.vocabulary_size()["n_nodes"] == 17


# ----------------------------------------------------------------------------------------------------------- 3: transform
@pytest.mark.parametrize("weighting", ["tf_idf", "tf"])
def test_transform_set_sizes_in_one_call_and_alone(solver, hb, weighting):
    rng = np.random.default_rng(11)
    centres = _rand(rng, 30, 32)
    sizes = (0, 1, 63, 64, 65, 257, hb.BOW_MAX_SET)
    sets = [centres[rng.integers(0, 30, n)] ^ np.packbits(rng.random((n, 256)) < 0.05, axis=1) for n in sizes]
    vocab = B.train(sets[2:6], branching=3, levels=3, iters=5, min_split=2, seed=5)
    solver.set_vocabulary(vocab)
    want = B.transform(vocab, sets, weighting=weighting)
    got = solver.bow_transform(sets, weighting=weighting)
    _same(got, want, CSR + ("desc_word",))
    assert np.diff(want["vec_off"])[0] == 0 and np.diff(want["vec_off"])[-1] > 1
    for i, s in enumerate(sets):
        one = solver.bow_transform([s], weighting=weighting)
        w, v = B.vector(want, i)
        assert np.array_equal(one["vec_word"], w) and np.array_equal(one["vec_val"], v), sizes[i]


def test_transform_refusals(solver, hb):
    with hb.Solver(0) as fresh:
        with pytest.raises(hb.BAHipError, match="no vocabulary"):
            fresh.bow_transform([_rand(np.random.default_rng(0), 5, 32)])
        with pytest.raises(hb.BAHipError, match="no vocabulary"):
            fresh.vocabulary()
    solver.set_vocabulary(_hand_tree())
    with pytest.raises(hb.BAHipError, match="not the vocabulary's"):
        solver.bow_transform([_rand(np.random.default_rng(0), 5, 32)])
    with pytest.raises(hb.BAHipError, match="more than"):
        solver.bow_transform([np.zeros((hb.BOW_MAX_SET + 1, 8), np.uint8)])


# ---------------------------------------------------------------------------------------------------------------- 4: score
def _score_check(solver, q, d, db_end=None, top_k=10):
    got, want = solver.bow_score(q, d, db_end=db_end, top_k=top_k, dense=True), B.score(q, d, db_end=db_end, top_k=top_k)
    _same(got, want, ("top_idx", "top_score", "score"))
    return got


@pytest.fixture(scope="module")
def vectors():
    """200 database vectors (entries 40 and 41 empty; 90, 150 and 199 copies of 17, 17 and 63) and 9 queries (query 4 empty, query 5 a copy of
    database vector 17, so that three database entries tie at the full score)."""
    rng = np.random.default_rng(12)
    d = B.random_vectors(rng, 200, empty=(40, 41))
    d = B.take_vectors(d, [17 if i in (90, 150) else 63 if i == 199 else i for i in range(200)])
    q = B.random_vectors(rng, 9, empty=(4,))
    qs = [B.vector(q, i) for i in range(9)]
    qs[5] = B.vector(d, 17)
    return B.join_vectors(qs), d


@pytest.mark.parametrize("nd", [1, 2, 65])
def test_score_equals_the_yardstick(solver, vectors, nd):
    q, d = vectors
    d = B.take_vectors(d, range(nd))
    for top_k in (1, 10, 64):                    # (64 > nd for nd = 1 and 2: padding)
        _score_check(solver, q, d, top_k=top_k)
    nq = len(q["vec_off"]) - 1
    _score_check(solver, q, d, db_end=np.zeros(nq, np.int32))
    _score_check(solver, q, d, db_end=np.arange(nq, dtype=np.int32))
    _score_check(solver, q, d, db_end=np.array([nd + 5, -3] + [nd] * (nq - 2), np.int32))     # clamped to 0 .. nd


def test_score_ties_empty_vectors_and_chunks(hb, solver, vectors, monkeypatch):
    q, d = vectors
    full = _score_check(solver, q, d, top_k=10)
    assert full["top_idx"][5, :3].tolist() == [17, 90, 150] and len(set(full["top_score"][5, :3].tolist())) == 1       # ties: the lower index first
    assert full["top_score"][5, 0] == B.vector(d, 17)[1].sum()
    assert (full["top_idx"][4] == -1).all() and (full["score"][:, 40:42] == 0).all()
    empty = B.take_vectors(d, [40, 41])
    _score_check(solver, q, empty)
    _score_check(solver, empty, d)
    _score_check(solver, B.take_vectors(d, []), d)
    _score_check(solver, q, B.take_vectors(d, []))
    monkeypatch.setenv("BA_DEBUG_BOW_CHUNK", "64")
    with hb.Solver(0) as small:
        for nd in (64, 65, 200):
            sub = B.take_vectors(d, range(nd))
            nq = len(q["vec_off"]) - 1
            for end in (None, np.arange(nq, dtype=np.int32) * 30):
                for top_k in (1, 10, 64):
                    got = _score_check(small, q, sub, db_end=end, top_k=top_k)
                    _same(got, solver.bow_score(q, sub, db_end=end, top_k=top_k, dense=True), ("top_idx", "top_score", "score"))


def test_score_refusals(solver, hb, vectors):
    q, d = vectors
    bad = dict(q, vec_word=q["vec_word"][::-1].copy())
    with pytest.raises(hb.BAHipError, match="ascending"):
        solver.bow_score(bad, d)
    with pytest.raises(hb.BAHipError, match="negative value"):
        solver.bow_score(dict(q, vec_val=-q["vec_val"]), d)
    with pytest.raises(hb.BAHipError, match="2\\^30"):
        solver.bow_score(dict(q, vec_val=q["vec_val"] * 2), d)


def test_planted_retrieval_equals_the_yardstick(solver, planted):
    """The (10, 3) vocabulary on the planted data (yardstick: 24 of 24, worst same-place / other-place ratio 1.55)."""
    solver.set_vocabulary(planted["vocab"])
    vq, vd = solver.bow_transform(planted["qs"]), solver.bow_transform(planted["db"])
    _same(vq, planted["vq"], CSR + ("desc_word",))
    _same(vd, planted["vd"], CSR + ("desc_word",))
    assert np.array_equal(vd["desc_word"], planted["vocab"]["train_word"])
    got = solver.bow_score(vq, vd, top_k=10, dense=True)
    _same(got, planted["score"], ("top_idx", "top_score", "score"))
    assert (planted["db_place"][got["top_idx"][:, 0]] == planted["q_place"]).all()


# ----------------------------------------------------------------------------------------------------------- 5: end to end
def test_end_to_end_on_the_desk_crop(solver, golden_dir):
    img = np.load(os.path.join(golden_dir, "orb_desk_crop.npy"))
    descs = [solver.extract_orb(np.ascontiguousarray(im), n_levels=4, n_features=500)["desc"] for im in (img, img[8:, 16:], img[:200, :230])]
    assert all(len(x) > 100 for x in descs)
    voc = solver.train_vocabulary(descs, branching=4, levels=3)
    _same(voc, B.train(descs, branching=4, levels=3), TREE)
    vec = solver.bow_transform(descs, weighting="tf")
    _same(vec, B.transform(voc, descs, weighting="tf"), CSR + ("desc_word",))
    assert np.array_equal(vec["desc_word"], voc["train_word"])
    s = solver.bow_score(vec, vec, top_k=3, dense=True)
    for i in range(3):
        w, v = B.vector(vec, i)
        assert s["score"][i, i] == v.sum() and v.sum() >= (1 << 30) - len(w)
