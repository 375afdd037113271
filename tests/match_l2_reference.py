"""The numpy yardstick of ba_match_l2 (include/ba_hip.h): squared distances from int64 products of the unsigned bytes (the plain
formula sum (q - t)^2, not the shifted one the kernel uses), the order (d, j) from a STABLE argsort of the distances, `good` by the
header's definition taken literally, the ratio comparison in Python floats."""
import numpy as np

from tests.match_reference import KEYS, assert_equal  # noqa: F401  (the same seven outputs, compared the same way)


def distances(q, t):
    """(nq, nt) int32 squared Euclidean distances of the rows of two uint8 arrays, by blocks of queries."""
    q, t = np.asarray(q, dtype=np.uint8), np.asarray(t, dtype=np.uint8)
    d = np.zeros((q.shape[0], t.shape[0]), dtype=np.int32)
    t64 = t.astype(np.int64)
    step = max(1, (1 << 22) // max(1, t.shape[0] * max(1, q.shape[1])))
    for lo in range(0, q.shape[0], step):
        diff = q[lo:lo + step, None, :].astype(np.int64) - t64[None, :, :]
        d[lo:lo + step] = (diff * diff).sum(axis=2)
    return d


def match_pair(q, t, ratio=0.75, max_distance=-1, mutual=0):
    """One pair -> dict(best, second, dist1, dist2 int32 (nq,), good bool (nq,), n_good)."""
    nq, nt = len(q), len(t)
    d = distances(q, t)
    best = np.full(nq, -1, dtype=np.int32)
    second, dist1, dist2 = best.copy(), best.copy(), best.copy()
    if nt >= 1:
        order = np.argsort(d, axis=1, kind="stable")
        best[:] = order[:, 0]
        dist1[:] = d[np.arange(nq), best]
    if nt >= 2:
        second[:] = order[:, 1]
        dist2[:] = d[np.arange(nq), second]
    first_query = np.argsort(d, axis=0, kind="stable")[0] if nq and nt else np.zeros(nt, dtype=np.int64)   # per train: lowest (d, i)
    good = np.zeros(nq, dtype=bool)
    for i in range(nq):
        g = best[i] >= 0
        g = g and (ratio <= 0 or (second[i] >= 0 and float(dist1[i]) < (ratio * ratio) * float(dist2[i])))
        g = g and (max_distance < 0 or dist1[i] <= max_distance)
        g = g and (mutual == 0 or first_query[best[i]] == i)
        good[i] = g
    return dict(best=best, second=second, dist1=dist1, dist2=dist2, good=good, n_good=int(good.sum()))


def match_l2(sets, pairs=None, **opts):
    """What hip_backend.Solver.match_l2 returns, from match_pair."""
    if pairs is None:
        pairs = [(0, 1)] if len(sets) else []
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    res = [match_pair(sets[a], sets[b], **opts) for a, b in pairs]
    out = {k: (np.concatenate([r[k] for r in res]) if res else np.zeros(0, dtype=bool if k == "good" else np.int32))
           for k in ("best", "second", "dist1", "dist2", "good")}
    out["row_off"] = np.r_[0, np.cumsum([len(sets[a]) for a, _ in pairs])].astype(np.int64)
    out["n_good"] = np.array([r["n_good"] for r in res], dtype=np.int32)
    return out
