"""CPU: the place recognition yardstick (tests/bow_reference.py) against itself -- tree invariants, the score identity,
hand-made ties, the planted retrieval case -- and the host side: place.Vocabulary / KeyframeDatabase / pair_list against the
yardstick-backed stand-in, and the input checks of hip_backend.Solver that run before any device call."""
import ctypes as C

import numpy as np
import pytest

from tests import bow_reference as B
from tests import ransac_reference as RR


@pytest.fixture(scope="module")
def planted():
    return B.planted()


def _rand(rng, n, width=32):
    return rng.integers(0, 256, (n, width), dtype=np.uint8)


def test_draws_are_the_ransac_generator():
    got = B.draw_rows(7, 2, 3, [0, 5, 1000, (1 << 24) - 1])
    assert [int(g) for g in got] == [RR.draw(7, 2, 3, x) for x in (0, 5, 1000, (1 << 24) - 1)]
    assert int(B.draw_rows((1 << 64) - 1, 0, 0, [1])[0]) == RR.draw((1 << 64) - 1, 0, 0, 1)


def check_tree(v, sets, levels):
    child0, n_child, rows = v["child0"], v["n_child"], sum(len(s) for s in sets)
    assert child0[0] in (-1, 1) and len(child0) == v["n_nodes"] == len(n_child) == len(v["node_desc"])
    nxt, parent = 1, np.full(v["n_nodes"], -1)
    for n in range(v["n_nodes"]):                          # breadth-first numbering, contiguous children, >= 2 of them
        if child0[n] < 0:
            assert n_child[n] == 0
            continue
        assert child0[n] == nxt and n_child[n] >= 2 and n_child[n] <= v["branching"]
        parent[nxt:nxt + n_child[n]] = n
        nxt += n_child[n]
    assert nxt == v["n_nodes"] and (parent[1:] >= 0).all() and (np.diff(parent[1:]) >= 0).all()
    depth = B.depth_of(child0, n_child)
    assert depth.max() <= levels and (np.diff(depth) >= 0).all()
    leaves = np.flatnonzero(child0 < 0)
    assert np.array_equal(v["word_of_node"][leaves], np.arange(len(leaves))) and (v["word_of_node"][child0 >= 0] == -1).all()
    assert v["n_words"] == len(leaves) == len(v["idf_q"])
    # the members of the children partition the parent's: every row is in one leaf, and a node's members are its subtree's
    members = np.zeros(v["n_nodes"], dtype=np.int64)
    np.add.at(members, leaves[v["train_word"]], 1)
    assert (members[child0 >= 0] == 0).all()
    for n in range(v["n_nodes"] - 1, 0, -1):               # (children are numbered after their parent)
        assert members[n] > 0                              # a child is a non-empty slot
        members[parent[n]] += members[n]
    assert members[0] == rows
    desc, _ = B.stack(sets)
    assert len(v["train_word"]) == rows and np.array_equal(B.descend(v, desc), v["train_word"])


@pytest.mark.parametrize("k,L,min_split", [(3, 2, 2), (10, 3, 0), (2, 8, 2), (4, 5, 0)])
def test_tree_invariants(planted, k, L, min_split):
    rng = np.random.default_rng(k * 10 + L)
    sets = [_rand(rng, n) for n in (120, 0, 77, 203)]
    check_tree(B.train(sets, branching=k, levels=L, iters=4, min_split=min_split, seed=2), sets, L)
    sets = planted[0][:12]
    check_tree(B.train(sets, branching=k, levels=L, iters=10, min_split=min_split, seed=7), sets, L)


def test_score_identity():
    """2 * score == sum vq + sum vd - sum |vq - vd| over the union of the words, exactly."""
    rng = np.random.default_rng(3)
    v = B.random_vectors(rng, 12, n_words=80, nnz=30, empty=(5,))
    s = B.score(v, v, top_k=3)["score"]
    for a in range(12):
        for b in range(12):
            (wa, va), (wb, vb) = B.vector(v, a), B.vector(v, b)
            da, db = np.zeros(80, np.int64), np.zeros(80, np.int64)
            da[wa], db[wb] = va, vb
            assert 2 * int(s[a, b]) == int(da.sum() + db.sum() - np.abs(da - db).sum())
    assert (np.diag(s) == [B.vector(v, i)[1].sum() for i in range(12)]).all() and s[5].max() == 0


def test_top_k_order_padding_and_db_end():
    rng = np.random.default_rng(4)
    d = B.random_vectors(rng, 6, n_words=40, nnz=15)
    d = B.take_vectors(d, [0, 1, 2, 1, 4, 1])
    out = B.score(B.take_vectors(d, [1]), d, top_k=8)
    assert out["top_idx"][0, :3].tolist() == [1, 3, 5] and out["top_idx"][0, 6:].tolist() == [-1, -1] and out["top_score"][0, 7] == 0
    assert (np.diff(out["top_score"][0]) <= 0).all()
    out = B.score(B.take_vectors(d, [1]), d, db_end=[3], top_k=8)
    assert set(out["top_idx"][0].tolist()) <= {-1, 0, 1, 2} and (out["score"][0, 3:] == 0).all()


def test_majority_tie_assignment_tie_and_identical_rows():
    rows, opts = B.majority_tie_case()
    v = B.train([rows], **opts)
    assert sorted(B.seed_rows(opts["seed"], 0, 2, np.arange(4))) == [0, 1]
    assert v["n_nodes"] == 3 and v["node_desc"][1].tolist() == [255] * 8 and np.array_equal(v["node_desc"][2], rows[0])
    assert v["train_word"].tolist() == [1, 1, 0, 0]
    assert B.majority(rows).tolist() == [255] * 8 and B.majority(rows[:3]).tolist() == rows[0].tolist()
    rows, opts = B.assign_tie_case()
    v = B.train([rows], **opts)
    first = B.seed_rows(opts["seed"], 0, 2, np.arange(3))[0]
    assert v["train_word"][2] == 0 == v["train_word"][first] and v["train_word"][1 - first] == 1
    assert B.assign(rows[2:], rows[:2], np.ones(2, bool)).tolist() == [0] and B.assign(rows[2:], rows[1::-1], np.ones(2, bool)).tolist() == [0]
    same = np.repeat(_rand(np.random.default_rng(4), 1), 50, axis=0)
    v = B.train([same[:20], same[20:]], branching=5, levels=3, min_split=2)
    assert v["n_nodes"] == 1 and v["n_words"] == 1 and v["idf_q"].tolist() == [0] and (v["train_word"] == 0).all()
    assert len(B.transform(v, [same[:7]])["vec_val"]) == 0
    t = B.transform(v, [same[:7], same[:0]], weighting="tf")
    assert t["vec_off"].tolist() == [0, 1, 1] and t["vec_word"].tolist() == [0] and t["vec_val"].tolist() == [1 << 30]


def test_a_slot_that_draws_an_earlier_slots_row_stays_empty():
    rows = _rand(np.random.default_rng(8), 3)
    seen = set()
    for seed in range(8):                    # four slots, three rows: at least one repeat, and the repeats stay empty
        distinct = len(set(B.seed_rows(seed, 0, 4, np.arange(3))))
        v = B.train([rows], branching=4, levels=1, min_split=2, seed=seed)
        assert v["n_child"][0] == (distinct if distinct >= 2 else 0) and v["n_words"] == max(distinct, 1)
        seen.add(distinct)
    assert seen == {1, 2, 3}


@pytest.mark.parametrize("k,L,ratio", [(8, 3, 1.12), (10, 3, 1.55), (4, 5, 1.38)])
def test_planted_retrieval(planted, k, L, ratio):
    """12 places, 4 database images (the training sets) and 2 queries each; iters 10, min_split 2, seed 7, default_rng(0).  The
    top-1 of all 24 queries is an image of its own place.  Worst ratio of the lowest same-place score to the highest
    other-place score on this yardstick: 1.126 (k / L = 8 / 3, 493 words), 1.551 (10 / 3, 899 words), 1.381 (4 / 5, 910 words)."""
    db, db_place, qs, q_place = planted
    v = B.train(db, branching=k, levels=L, iters=10, min_split=2, seed=7)
    vd = B.transform(v, db)
    assert np.array_equal(vd["desc_word"], v["train_word"])
    r = B.score(B.transform(v, qs), vd, top_k=4)
    assert (db_place[r["top_idx"][:, 0]] == q_place).all()
    worst = min(r["score"][q][db_place == q_place[q]].min() / r["score"][q][db_place != q_place[q]].max() for q in range(len(qs)))
    assert worst > 1.1 and abs(worst - ratio) < 0.01


def test_idf_is_the_formula(planted):
    db = planted[0][:16]
    v = B.train(db, branching=6, levels=2, min_split=2, seed=1)
    _, off = B.stack(db)
    set_of_row = np.searchsorted(off, np.arange(off[-1]), side="right") - 1
    n_with = np.array([len(np.unique(set_of_row[v["train_word"] == w])) for w in range(v["n_words"])])
    want = np.floor(np.log(len(db) / n_with) * 4096 + 0.5)
    assert np.abs(v["idf_q"] - want).max() <= 1 and v["idf_q"].min() >= 0 and v["idf_q"].max() > 0


# ------------------------------------------------------------------------------------------------------------------ place.py
def _tree():
    nd = np.zeros((5, 8), dtype=np.uint8)
    nd[2:] = 255
    return dict(child0=[1, -1, 3, -1, -1], n_child=[2, 0, 2, 0, 0], node_desc=nd, idf_q=[4096, 100, 300])


def test_vocabulary_save_load_round_trip(tmp_path, planted):
    from bundle_adjustment_amd.place import Vocabulary
    s = B.YardstickSolver()
    voc = Vocabulary.train(s, planted[0][:8], branching=4, levels=2, min_split=2)
    path = tmp_path / "voc.npz"
    voc.save(path)
    back = Vocabulary.load(path)
    for k in ("child0", "n_child", "node_desc", "idf_q"):
        a, b = getattr(voc, k), getattr(back, k)
        assert a.dtype == b.dtype and np.array_equal(a, b), k
    assert np.array_equal(back.word_of_node, s.vocab["word_of_node"]) and (back.n_nodes, back.n_words, back.desc_bytes) == (s.vocab["n_nodes"], s.vocab["n_words"], 32)
    other = B.YardstickSolver()
    back.upload(other)
    assert np.array_equal(other.bow_transform(planted[2][:2])["vec_val"], s.bow_transform(planted[2][:2])["vec_val"])
    np.savez(tmp_path / "bad.npz", child0=voc.child0)
    with pytest.raises(ValueError, match="not a vocabulary file"):
        Vocabulary.load(tmp_path / "bad.npz")


def test_vocabulary_validation_refusals():
    from bundle_adjustment_amd.place import Vocabulary
    Vocabulary.from_dict(_tree())

    def bad(match, **kw):
        with pytest.raises(ValueError, match=match):
            Vocabulary.from_dict(dict(_tree(), **kw))
    bad("breadth-first contiguous", child0=[1, -1, 4, -1, -1])
    bad("breadth-first contiguous", child0=[2, -1, 3, -1, -1])
    bad("child of no node", child0=[1, -1, -1, -1, -1], n_child=[2, 0, 0, 0, 0], idf_q=[1, 1, 1, 1])
    bad("n_child", n_child=[2, 0, 1, 0, 0])
    bad("n_child", n_child=[2, 0, 33, 0, 0])
    bad("at a leaf", n_child=[2, 1, 2, 0, 0])
    bad("reach past", n_child=[2, 0, 3, 0, 0])
    bad("idf_q must lie", idf_q=[0, -1, 0])
    bad("idf_q must lie", idf_q=[0, 1 << 17, 0])
    bad("one entry per word", idf_q=[0, 0])
    bad("2-D uint8", node_desc=np.zeros((5, 8), np.int32))
    bad("multiple of 8", node_desc=np.zeros((5, 12), np.uint8))
    bad("one entry per node", node_desc=np.zeros((4, 8), np.uint8))
    n = 19
    child0, n_child = np.full(n, -1), np.zeros(n, int)
    for inner, first in [(0, 1)] + [(2 * d - 1, 2 * d + 1) for d in range(1, 9)]:
        child0[inner], n_child[inner] = first, 2
    with pytest.raises(ValueError, match="depth"):
        Vocabulary(child0, n_child, np.zeros((n, 8), np.uint8), np.zeros(10, int))
    Vocabulary(np.where(np.arange(17) == 15, -1, child0[:17]), np.where(np.arange(17) == 15, 0, n_child[:17]), np.zeros((17, 8), np.uint8), np.zeros(9, int))


def test_keyframe_database_and_pair_list(planted):
    from bundle_adjustment_amd import place
    db, db_place, qs, q_place = planted
    s = B.YardstickSolver()
    place.Vocabulary.train(s, db, branching=10, levels=3, iters=10, min_split=2, seed=7)
    csr = s.bow_transform(db)
    vecs = place.split_vectors(csr)
    assert all(np.array_equal(a, b) for x, y in zip(vecs, (B.vector(csr, i) for i in range(len(db)))) for a, b in zip(x, y))
    back = place.stack_vectors(vecs)
    assert all(np.array_equal(back[k], csr[k]) for k in ("vec_off", "vec_word", "vec_val"))
    kdb = place.KeyframeDatabase(s)
    assert kdb.query(vecs[0]) == [] and len(kdb) == 0
    for i, v in enumerate(vecs):
        assert kdb.add(v) == i
    q = place.bow_vector(s, qs[0])
    full = B.score(s.bow_transform(qs[:1]), csr, top_k=5)
    assert kdb.query(q, top_k=5) == [(int(i), int(sc)) for i, sc in zip(full["top_idx"][0], full["top_score"][0]) if i >= 0]
    assert db_place[kdb.query(q, top_k=1)[0][0]] == q_place[0]
    # min_gap hides the newest entries through db_end
    s.score_calls.clear()
    got = kdb.query(q, min_gap=46, top_k=5)
    assert s.score_calls[-1]["db_end"] == [2] and s.score_calls[-1]["nd"] == 48 and all(i < 2 for i, _ in got)
    assert kdb.query(q, min_gap=48) == [] and kdb.query(q, min_gap=100) == []
    with pytest.raises(ValueError):
        kdb.query(q, min_gap=-1)
    with pytest.raises(ValueError):
        kdb.add((np.arange(3), np.arange(4)))
    # ORB-SLAM's normalisation: candidates scoring at least ratio * (the score against the predecessor)
    ref = kdb.score_against(q, 1)
    assert ref == int(full["score"][0, 1])
    cands = kdb.loop_candidates(q, ref_score=ref, ratio=0.75, top_k=10)
    all10 = kdb.query(q, top_k=10)
    assert cands == [(i, sc) for i, sc in all10 if sc * (1 << 20) >= ref * round(0.75 * (1 << 20))] and 1 <= len(cands) <= len(all10)
    assert kdb.loop_candidates(q, ref_score=1 << 30, ratio=1.0) == []
    with pytest.raises(IndexError):
        kdb.score_against(q, 48)
    # pair_list: every image against the earlier ones, each pair once, i < j
    sub = B.take_vectors(csr, range(12))
    s.score_calls.clear()
    pairs = place.pair_list(s, sub, top_k=2)
    assert s.score_calls[-1]["db_end"] == list(range(12)) and len(set(pairs)) == len(pairs) and all(i < j for i, j in pairs)
    ref = B.score(sub, sub, db_end=np.arange(12), top_k=2)
    assert pairs == sorted({(int(j), q_) for q_ in range(12) for j in ref["top_idx"][q_] if j >= 0})
    assert sum(db_place[i] == db_place[j] for i, j in pairs) >= 12 and place.pair_list(s, place.split_vectors(sub), top_k=2) == pairs
    assert place.pair_list(s, B.take_vectors(csr, [0])) == [] and place.pair_list(s, []) == []


def test_names_are_exported():
    import bundle_adjustment_amd as pkg
    from bundle_adjustment_amd import place
    assert pkg.KeyframeDatabase is place.KeyframeDatabase and pkg.Vocabulary is place.Vocabulary and pkg.pair_list is place.pair_list
    assert place.BOW_ONE == B.BOW_ONE


# ------------------------------------------------------------------------------------------------------- hip_backend, no device
@pytest.fixture(scope="module")
def hb():
    import __graft_entry__ as g
    g.build()
    from bundle_adjustment_amd import hip_backend
    return hip_backend


def test_vocab_options_and_constants(hb):
    o = hb.vocab_options()
    assert (o.branching, o.levels, o.iters, o.min_split, o.seed) == (10, 6, 10, 0, 0) and C.sizeof(hb.BAVocabOptions) == 24
    assert hb.vocab_options(seed=(1 << 64) - 1, branching=4).seed == (1 << 64) - 1
    with pytest.raises(TypeError):
        hb.vocab_options(depth=3)
    assert hb.BOW_ONE == B.BOW_ONE and hb.BOW_IDF_ONE == B.IDF_ONE and hb.BOW_MAX_SET >= hb.ORB_MAX_FEATURES and hb.BOW_MAX_TRAIN_ROWS == 1 << B.ROW_BITS


def test_solver_input_checks_run_before_any_device_call(hb):
    s = object.__new__(hb.Solver)            # no handle: anything that reached the library would fail differently
    s._lib, s._h = hb.load_library(), None
    a, b = np.zeros((3, 32), np.uint8), np.zeros((3, 64), np.uint8)
    for call in (s.train_vocabulary, s.bow_transform):
        with pytest.raises(ValueError, match="different widths"):
            call([a, b])
        with pytest.raises(ValueError, match="2-D uint8"):
            call([a.astype(np.float32)])
        with pytest.raises(ValueError, match="2-D uint8"):
            call([a[0]])
    with pytest.raises(ValueError, match="unknown weighting"):
        s.bow_transform([a], weighting="l2")
    with pytest.raises(TypeError):
        s.train_vocabulary([a], depth=3)
    v = B.random_vectors(np.random.default_rng(0), 3)
    with pytest.raises(ValueError, match="vec_off, vec_word and vec_val"):
        s.bow_score(dict(vec_off=v["vec_off"]), v)
    with pytest.raises(ValueError, match="integer array"):
        s.bow_score(dict(v, vec_val=v["vec_val"].astype(np.float64)), v)
    with pytest.raises(ValueError, match="must end at"):
        s.bow_score(v, dict(v, vec_word=v["vec_word"][:-1]))
    with pytest.raises(ValueError, match="one entry per query"):
        s.bow_score(v, v, db_end=[1, 2])
    for k in (0, 65):
        with pytest.raises(ValueError, match="top_k"):
            s.bow_score(v, v, top_k=k)
    t = _tree()
    with pytest.raises(ValueError, match="2-D uint8"):
        s.set_vocabulary(dict(t, node_desc=t["node_desc"].astype(np.int16)))
    with pytest.raises(ValueError, match="one entry per node"):
        s.set_vocabulary(dict(t, n_child=[2, 0, 2, 0]))
    with pytest.raises(ValueError, match="one entry per leaf"):
        s.set_vocabulary(dict(t, idf_q=[1, 2]))
    s._h = None                              # (nothing for __del__ to destroy)
