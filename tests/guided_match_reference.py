"""The numpy yardstick of ba_match_guided (include/ba_hip.h): the two gates written as the header's expressions, float64 arrays and
one numpy operation per device operation (numpy rounds every operation on its own, as the kernels do), then
tests/match_reference.py's stable-argsort order over the admitted train rows of each query, mapped back to train indices."""
import numpy as np

from tests import match_reference as M


def gate_window(window, xy_train):
    """(nq, nt) bool.  window (nq, 3) float32 (px, py, r) per query, xy_train (nt, 2) float32."""
    w = np.asarray(window, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    t = np.asarray(xy_train, dtype=np.float32).reshape(-1, 2).astype(np.float64)
    px, py, r = w[:, 0, None], w[:, 1, None], w[:, 2, None]
    x, y = t[None, :, 0], t[None, :, 1]
    with np.errstate(invalid="ignore", over="ignore"):
        dx = x - px
        dy = y - py
        a = dx * dx
        b = dy * dy
        d2 = a + b
        rr = r * r
        return (r >= 0) & (d2 <= rr)


def gate_epipolar(F, xy_query, xy_train, max_epi_px):
    """(nq, nt) bool.  F (3, 3) float64 with x_train^T F x_query = 0; the train keypoint against the query's line."""
    F = np.asarray(F, dtype=np.float64).reshape(3, 3)
    q = np.asarray(xy_query, dtype=np.float32).reshape(-1, 2).astype(np.float64)
    t = np.asarray(xy_train, dtype=np.float32).reshape(-1, 2).astype(np.float64)
    x1, y1 = q[:, 0], q[:, 1]
    x, y = t[None, :, 0], t[None, :, 1]
    m = np.float64(max_epi_px)
    with np.errstate(invalid="ignore", over="ignore"):
        l0 = (F[0, 0] * x1 + F[0, 1] * y1) + F[0, 2]
        l1 = (F[1, 0] * x1 + F[1, 1] * y1) + F[1, 2]
        l2 = (F[2, 0] * x1 + F[2, 1] * y1) + F[2, 2]
        n = l0 * l0 + l1 * l1
        thr = (m * m) * n
        e = (l0[:, None] * x + l1[:, None] * y) + l2[:, None]
        return (n > 0)[:, None] & (e * e <= thr[:, None])


def match_pair_guided(q, t, gate, ratio=0.75, max_distance=-1, mutual=0, single=1):
    """One pair under the (nq, nt) bool gate -> dict(best, second, dist1, dist2, n_cand int32 (nq,), good bool (nq,), n_good)."""
    nq, nt = len(q), len(t)
    gate = np.asarray(gate, dtype=bool).reshape(nq, nt)
    d = M.distances(q, t)
    best = np.full(nq, -1, dtype=np.int32)
    second, dist1, dist2 = best.copy(), best.copy(), best.copy()
    for i in range(nq):
        adm = np.nonzero(gate[i])[0]
        order = adm[np.argsort(d[i, adm], kind="stable")]
        if len(order) >= 1:
            best[i], dist1[i] = order[0], d[i, order[0]]
        if len(order) >= 2:
            second[i], dist2[i] = order[1], d[i, order[1]]
    first_query = np.full(nt, -1, dtype=np.int64)          # per train row: the lowest (d, i) among the queries that admit it
    for j in range(nt):
        adm = np.nonzero(gate[:, j])[0]
        if len(adm):
            first_query[j] = adm[np.argsort(d[adm, j], kind="stable")[0]]
    good = np.zeros(nq, dtype=bool)
    for i in range(nq):
        g = best[i] >= 0
        if ratio > 0:
            g = g and ((second[i] >= 0 and float(dist1[i]) < ratio * float(dist2[i])) or (single == 1 and second[i] < 0))
        g = g and (max_distance < 0 or dist1[i] <= max_distance)
        g = g and (mutual == 0 or first_query[best[i]] == i)
        good[i] = g
    return dict(best=best, second=second, dist1=dist1, dist2=dist2, good=good, n_good=int(good.sum()),
                n_cand=gate.sum(axis=1).astype(np.int32))


def gates_of(sets, keypoints, pairs, window=None, fundamental=None, max_epi_px=3.0):
    """The (nq, nt) gate of every pair, from what hip_backend.Solver.match_guided is given."""
    gates, row = [], 0
    for p, (a, b) in enumerate(pairs):
        if window is not None:
            w = np.asarray(window, dtype=np.float32).reshape(-1, 3)[row:row + len(sets[a])]
            gates.append(gate_window(w, keypoints[b]))
        else:
            gates.append(gate_epipolar(np.asarray(fundamental, dtype=np.float64).reshape(-1, 3, 3)[p], keypoints[a], keypoints[b], max_epi_px))
        row += len(sets[a])
    return gates


def match_guided(sets, keypoints, pairs=None, *, window=None, fundamental=None, max_epi_px=3.0, **opts):
    """What hip_backend.Solver.match_guided returns, from match_pair_guided."""
    if pairs is None:
        pairs = [(0, 1)] if len(sets) else []
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    gates = gates_of(sets, keypoints, pairs, window, fundamental, max_epi_px)
    res = [match_pair_guided(sets[a], sets[b], g, **opts) for (a, b), g in zip(pairs, gates)]
    out = {k: (np.concatenate([r[k] for r in res]) if res else np.zeros(0, dtype=bool if k == "good" else np.int32))
           for k in ("best", "second", "dist1", "dist2", "good", "n_cand")}
    out["row_off"] = np.r_[0, np.cumsum([len(sets[a]) for a, _ in pairs])].astype(np.int64)
    out["n_good"] = np.array([r["n_good"] for r in res], dtype=np.int32)
    return out


KEYS = M.KEYS + ("n_cand",)


def assert_equal(got, ref):
    for k in KEYS:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, (k, got[k].dtype, got[k].shape, ref[k].dtype, ref[k].shape)
        assert np.array_equal(got[k], ref[k]), (k, np.nonzero(np.asarray(got[k]) != np.asarray(ref[k]))[0][:10])
