"""Times of the place recognition calls (output kept in profiles/bow_times.txt).

    python tools/bow_times.py [--out FILE] [--stage NAME] [--rows N]

Host wall time of each call with every output copied back, measured as tools/match_times.py does (median, min and max of REPS
calls after WARM warm-up calls); a stage is one call:
  train      ba_vocab_train on --rows (default 1 000 000) 32-byte rows in 2000 sets, k = 10, L = 5, iters = 10: three quarters of the
             rows are copies of 20 000 planted descriptors with 4 % of the bits flipped, the rest random bytes (1 + 2 calls);
  transform  ba_bow_transform of 16 sets of 3000 rows under that vocabulary;
  score      ba_bow_score of 10 000 x 10 000 vectors of about 2000 words out of 100 000, top_k = 10 (synthetic L1-normalised vectors);
  match      the one ba_match_descriptors call behind features.match_to_keyframes, for one frame of 3000 descriptors against 1000
             keyframes of 3000: the exhaustive loop that retrieval replaces.
--stage runs one stage alone (transform trains a small vocabulary of its own then).  Recorded, not gated."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS, WARM = 7, 2


def timed(fn, reps=REPS, warm=WARM):
    for _ in range(warm):
        out = fn()
    w = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        w.append(time.perf_counter() - t0)
    return out, f"{1e3 * float(np.median(w)):.3f} ms (min {1e3 * min(w):.3f}, max {1e3 * max(w):.3f})"


def training_rows(rng, rows, n_sets=2000):
    planted = rng.integers(0, 256, (20000, 32), dtype=np.uint8)
    n_copy = rows * 3 // 4
    data = np.concatenate([planted[rng.integers(0, len(planted), n_copy)] ^ np.packbits(rng.random((n_copy, 256)) < 0.04, axis=1),
                           rng.integers(0, 256, (rows - n_copy, 32), dtype=np.uint8)])
    data = data[rng.permutation(rows)]
    return np.array_split(data, n_sets)


def vectors(rng, n, n_words=100000, nnz=2000):
    off, vw, vv = np.zeros(n + 1, dtype=np.int64), [], []
    for i in range(n):
        w = np.unique(rng.integers(0, n_words, nnz))
        a = rng.integers(1, 100, len(w)).astype(np.int64)
        v = (a << 30) // int(a.sum())
        vw.append(w[v > 0].astype(np.int32))
        vv.append(v[v > 0].astype(np.int32))
        off[i + 1] = off[i] + len(vw[-1])
    return dict(vec_off=off, vec_word=np.concatenate(vw), vec_val=np.concatenate(vv))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bow_times.txt"))
    ap.add_argument("--stage", default="")
    ap.add_argument("--rows", type=int, default=1000000)
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from bundle_adjustment_amd import hip_backend as hb
    rng = np.random.default_rng(0)
    lines = []

    def note(line):
        lines.append(line)
        print(line, flush=True)
    with hb.Solver(0) as s:
        if a.stage in ("", "train"):
            sets = training_rows(rng, a.rows)
            voc, t = timed(lambda: s.train_vocabulary(sets, branching=10, levels=5, iters=10), reps=2, warm=1)
            note(f"train: {a.rows} rows of 32 bytes in {len(sets)} sets, k 10, L 5, iters 10: {voc['n_nodes']} nodes, {voc['n_words']} words: wall {t}")
        if a.stage in ("", "transform"):
            if a.stage:
                s.train_vocabulary(training_rows(rng, 100000, 200), branching=10, levels=4, iters=5)
            sets = [rng.integers(0, 256, (3000, 32), dtype=np.uint8) for _ in range(16)]
            out, t = timed(lambda: s.bow_transform(sets))
            note(f"transform: 16 sets of 3000 rows, {s.vocabulary_size()['n_words']} words: {len(out['vec_word'])} entries: wall {t}")
        if a.stage in ("", "score"):
            v = vectors(rng, 10000)
            out, t = timed(lambda: s.bow_score(v, v, top_k=10), reps=3, warm=1)
            note(f"score: 10000 x 10000 vectors of {len(v['vec_word']) / 10000:.0f} words out of 100000, top_k 10: wall {t}; "
                 f"self first for {(out['top_idx'][:, 0] == np.arange(10000)).mean():.3f} of the queries")
            sub = {k: (x[:101] if k == "vec_off" else x[:int(v["vec_off"][100])]) for k, x in v.items()}
            _, t = timed(lambda: s.bow_score(sub, v, top_k=10))
            note(f"score: 100 x 10000 of the same vectors: wall {t}")
        if a.stage in ("", "match"):
            new = rng.integers(0, 256, (3000, 32), dtype=np.uint8)
            kfs = [rng.integers(0, 256, (3000, 32), dtype=np.uint8) for _ in range(1000)]
            pairs = np.array([(1 + n, 0) for n in range(len(kfs))], dtype=np.int32)
            _, t = timed(lambda: s.match_descriptors([new] + kfs, pairs), reps=3, warm=1)
            note(f"match_to_keyframes' one call (match_descriptors, without building the Match lists): one frame of 3000 descriptors against "
                 f"1000 keyframes of 3000: wall {t}")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
