"""CPU: the numpy statement of ba_set_problem's layout (tests/layout_reference.py) against a layout built by a plain-Python
loop on tiny problems -- camera table in LDS and past it, 2 and 16 lanes per point, duplicated pairs, points and cameras
nobody sees -- and against mutants of that layout, each of which it must reject by the name of the array that is wrong."""
import numpy as np
import pytest

from tests.layout_reference import NPART, check_layout, table_fits


def _problem(n_cams, n_pts, seed, n_obs=60):
    """random visibility with duplicated (camera, point) pairs (own pixels each), a point and cameras nobody sees,
    shuffled; every camera that sees anything sees one point twice at least"""
    rng = np.random.default_rng(seed)
    cams_used = rng.choice(np.arange(1, n_cams - 1), 5, replace=False)      # camera 0 and the last one see nothing
    ci = rng.choice(cams_used, n_obs)
    pi = rng.integers(0, n_pts - 1, n_obs)                                   # the last point is seen by nobody
    pi[pi == 3] = 4                                                          # ... and point 3
    ci = np.concatenate([ci, ci[:12], ci[:6]])
    pi = np.concatenate([pi, pi[:12], pi[:6]])                               # pairs given twice and three times
    perm = rng.permutation(ci.size)
    uv = rng.uniform(0, 1000, (ci.size, 2))
    return ci[perm].astype(np.int32), pi[perm].astype(np.int32), uv


def _loop_build(ci, pi, uv, n_cams, n_pts, lanes, nblkP, long_spb):
    """the layout by loops over observations, points and cameras; nothing shared with layout_reference"""
    n_obs = len(ci)
    if table_fits(n_cams):
        slot = list(range(n_pts))
    else:
        keys = []
        for p in range(n_pts):
            mine = [int(ci[i]) for i in range(n_obs) if pi[i] == p]
            keys.append((sum(mine) / len(mine) if mine else float(n_cams), p))
        slot = [0] * n_pts
        for r, (_, p) in enumerate(sorted(keys)):                 # (ties: by caller's index = stable)
            slot[p] = r
    segs = [[] for _ in range(n_pts)]
    for i in range(n_obs):
        segs[slot[pi[i]]].append(i)
    if lanes == 2 and table_fits(n_cams):                         # any visiting order inside a point will do
        segs = [s[1:] + s[:1] for s in segs]
    pt_off, p_src = [0], []
    for s in segs:
        p_src += s
        pt_off.append(len(p_src))
    per_cam = [[] for _ in range(n_cams)]
    for j, i in enumerate(p_src):                                 # walking the point-ordered list: ascending point, ties in list order
        per_cam[ci[i]].append(i)
    c_orig, offk = [], []
    for c in range(n_cams):
        n = len(per_cam[c])
        offk += [len(c_orig) + (n * k) // NPART for k in range(NPART + 1)]
        c_orig += per_cam[c]
    lens = [len(s) for s in segs]
    med = sorted(lens)[n_pts // 2]
    long_thr = max(8, 2 * med) if lanes == 2 else 0x7fffffff
    long_pts = [p for p in range(n_pts) if lens[p] > long_thr]
    nblkL = (len(long_pts) + long_spb - 1) // long_spb
    ppb = max(1, (n_pts + nblkP - 1) // nblkP)
    groups = [[p for p in range(b * ppb, min(n_pts, (b + 1) * ppb))] for b in range(nblkP)]
    groups += [long_pts[w * long_spb:(w + 1) * long_spb] for w in range(nblkL)]
    win = []
    for g in groups:
        cams = [int(ci[i]) for p in g for i in segs[p]]
        win += [min(cams), max(cams) - min(cams) + 1] if cams else [0, 0]
    widths = win[1::2]
    spans = [max(ci[i] for i in s) - min(ci[i] for i in s) for s in segs if s]
    in_part = in_band = 0
    for c in range(n_cams):
        for k in range(NPART):
            for a in range(offk[c * (NPART + 1) + k], offk[c * (NPART + 1) + k + 1]):
                q = slot[pi[c_orig[a]]]
                s = next(t for t in range(NPART) if -(-t * n_pts // NPART) <= q < -(-(t + 1) * n_pts // NPART))
                in_part += s == k
                in_band += s == (c * NPART) // n_cams
    sc = dict(lanes=lanes, nblkP=nblkP, ppb=ppb, nblkL=nblkL, long_spb=long_spb, long_thr=long_thr, n_long=len(long_pts),
              cam_band=int(in_band > in_part), banded=int(bool(spans) and sum(spans) / len(spans) <= n_cams / 8.0),
              cam_segl=16 if n_obs // n_cams // NPART < 64 else 64, build_path=0, mw_ok=0)
    for name, row in (("pinhole", 144), ("bal", 208)):
        ok = [w * row <= 150 * 1024 for w in widths]
        sc["all_lds_" + name] = int(all(ok))
        sc["lds_bytes_" + name] = max([w * row for w, o in zip(widths, ok) if o], default=0)
    lay = dict(pt_off=np.array(pt_off, np.int32), p_cam=np.array([ci[i] for i in p_src], np.int32),
               c_pt=np.array([slot[pi[i]] for i in c_orig], np.int32), c_orig=np.array(c_orig, np.int32),
               offk=np.array(offk, np.int32), long_pts=np.array(long_pts, np.int32), blk_win=np.array(win, np.int32),
               slot=np.array(slot, np.int32), p_uv=uv[p_src].reshape(-1).copy(), c_uv=uv[c_orig].reshape(-1).copy())
    return lay, sc


CASES = {   # n_cams, n_pts, lanes, nblkP, long_spb
    "fits_16_lanes": (9, 20, 16, 3, 64),
    "fits_2_lanes": (9, 20, 2, 3, 2),
    "fits_2_lanes_one_range": (12, 7, 2, 1, 64),
    "past_lds_16_lanes": (1100, 20, 16, 4, 64),
    "past_lds_2_lanes": (1100, 20, 2, 6, 1),
}


def _case(name):
    n_cams, n_pts, lanes, nblkP, long_spb = CASES[name]
    ci, pi, uv = _problem(n_cams, n_pts, seed=len(name))
    if lanes == 2:              # long tracks (more than max(8, 2 med) = 8 views): points 0 .. 2 get ten views each and more,
        pi[:30] = np.arange(30) % 3                               # most other points lose all but one (median 1)
        keep = np.ones(ci.size, bool)
        for p in range(4, n_pts):
            keep[np.flatnonzero(pi == p)[1:]] = False
        ci, pi, uv = ci[keep], pi[keep], uv[keep]
    lay, sc = _loop_build(ci, pi, uv, n_cams, n_pts, lanes, nblkP, long_spb)
    return ci, pi, uv, n_cams, n_pts, lay, sc


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_accepts_the_loop_built_layout(name):
    ci, pi, uv, n_cams, n_pts, lay, sc = _case(name)
    assert np.bincount(pi, minlength=n_pts).min() == 0 and np.bincount(ci, minlength=n_cams).min() == 0
    if sc["lanes"] == 2:
        assert sc["n_long"] > 0 and sc["nblkL"] > 0
    if not table_fits(n_cams):
        assert not np.array_equal(lay["slot"], np.arange(n_pts))
    check_layout(ci, pi, uv, n_cams, n_pts, lay, sc)


def test_reference_states_its_precondition():
    ci, pi, uv, n_cams, n_pts, lay, sc = _case("fits_16_lanes")
    uv = uv.copy()
    uv[7] = uv[2]
    with pytest.raises(AssertionError, match="precondition"):
        check_layout(ci, pi, uv, n_cams, n_pts, lay, sc)


def _camera_with_a_repeated_point(lay, sc, n_cams):
    """(a, a + 1): neighbouring entries of one camera's list with the same point"""
    offk = lay["offk"].reshape(n_cams, NPART + 1)
    for c in range(n_cams):
        for a in range(offk[c, 0], offk[c, NPART] - 1):
            if lay["c_pt"][a] == lay["c_pt"][a + 1]:
                return a
    raise AssertionError("the problem has no repeated pair")


def _camera_out_of_caller_order(lay, n_cams):
    """a camera whose list, put into the caller's order, is not ascending in point"""
    offk = lay["offk"].reshape(n_cams, NPART + 1)
    for c in range(n_cams):
        a, b = offk[c, 0], offk[c, NPART]
        order = np.argsort(lay["c_orig"][a:b], kind="stable")
        if np.any(np.diff(lay["c_pt"][a:b][order]) < 0):
            return a, b, order
    raise AssertionError("every camera's caller order is ascending in point")


def _mutate(kind, lay, sc, n_cams, n_pts):
    lay = {k: v.copy() for k, v in lay.items()}
    c_uv = lay["c_uv"].reshape(-1, 2)
    if kind == "c_orig_swap_of_a_repeated_point":      # the pair's pixels go along: only the tie rule can tell
        a = _camera_with_a_repeated_point(lay, sc, n_cams)
        lay["c_orig"][[a, a + 1]] = lay["c_orig"][[a + 1, a]]
        c_uv[[a, a + 1]] = c_uv[[a + 1, a]]
        return lay, "c_orig"
    if kind == "c_orig_swap":                          # two entries of one camera with different points, c_orig alone:
        offk = lay["offk"].reshape(n_cams, NPART + 1)  # the first array that disagrees with c_orig is c_pt
        c = next(c for c in range(n_cams) if offk[c, NPART] > offk[c, 0] and lay["c_pt"][offk[c, 0]] != lay["c_pt"][offk[c, NPART] - 1])
        a, b = offk[c, 0], offk[c, NPART] - 1
        lay["c_orig"][[a, b]] = lay["c_orig"][[b, a]]
        return lay, "c_pt"
    if kind == "c_pt_in_caller_order":                 # the whole camera consistently in caller order
        a, b, order = _camera_out_of_caller_order(lay, n_cams)
        for k in ("c_pt", "c_orig"):
            lay[k][a:b] = lay[k][a:b][order]
        c_uv[a:b] = c_uv[a:b][order]
        return lay, "c_pt"
    if kind == "offk_off_by_one":
        offk = lay["offk"].reshape(n_cams, NPART + 1)
        c = int(np.argmax(offk[:, NPART] - offk[:, 0]))
        offk[c, 3] += 1
        return lay, "offk"
    if kind in ("window_short_at_the_low_end", "window_short_at_the_high_end"):
        win = lay["blk_win"].reshape(-1, 2)
        b = int(np.argmax(win[:, 1]))
        assert win[b, 1] >= 2
        win[b, 1] -= 1
        if kind == "window_short_at_the_low_end":
            win[b, 0] += 1
        return lay, "blk_win"
    if kind == "long_window_short":
        win = lay["blk_win"].reshape(-1, 2)
        assert sc["nblkL"] > 0 and win[-1, 1] >= 2
        win[-1, 1] -= 1
        return lay, "blk_win"
    if kind == "long_pts_misses_a_point":
        assert lay["long_pts"].size >= 2
        lay["long_pts"] = np.delete(lay["long_pts"], 1)
        return lay, "long_pts"
    if kind == "pt_off_shifted":
        lay["pt_off"][n_pts // 2:n_pts] += 1
        return lay, "pt_off"
    if kind == "c_uv_from_the_neighbour":
        a = c_uv.shape[0] // 2
        c_uv[a] = c_uv[a + 1]
        return lay, "c_uv"
    if kind == "p_cam_of_the_neighbour":
        j = next(j for j in range(lay["p_cam"].size - 1) if lay["p_cam"][j] != lay["p_cam"][j + 1])
        lay["p_cam"][j] = lay["p_cam"][j + 1]
        return lay, "p_cam"
    if kind == "point_order_not_stable":               # two observations of a point swapped (pixels along): only for >2 lanes
        off = lay["pt_off"]
        p = int(np.argmax(np.diff(off)))
        j = off[p]
        p_uv = lay["p_uv"].reshape(-1, 2)
        lay["p_cam"][[j, j + 1]] = lay["p_cam"][[j + 1, j]]
        p_uv[[j, j + 1]] = p_uv[[j + 1, j]]
        return lay, "p_uv"
    raise KeyError(kind)


MUTANTS = ["c_orig_swap_of_a_repeated_point", "c_orig_swap", "c_pt_in_caller_order", "offk_off_by_one",
           "window_short_at_the_low_end", "window_short_at_the_high_end", "pt_off_shifted", "c_uv_from_the_neighbour",
           "p_cam_of_the_neighbour"]


@pytest.mark.parametrize("kind", MUTANTS + ["point_order_not_stable"])
@pytest.mark.parametrize("name", ["fits_16_lanes", "past_lds_16_lanes"])
def test_reference_rejects_mutants_by_name(name, kind):
    ci, pi, uv, n_cams, n_pts, lay, sc = _case(name)
    bad, array = _mutate(kind, lay, sc, n_cams, n_pts)
    with pytest.raises(AssertionError, match="^" + array + r"[\[ ]"):
        check_layout(ci, pi, uv, n_cams, n_pts, bad, sc)


@pytest.mark.parametrize("kind", MUTANTS + ["long_pts_misses_a_point", "long_window_short"])
@pytest.mark.parametrize("name", ["fits_2_lanes", "past_lds_2_lanes"])
def test_reference_rejects_mutants_by_name_with_long_tracks(name, kind):
    ci, pi, uv, n_cams, n_pts, lay, sc = _case(name)
    bad, array = _mutate(kind, lay, sc, n_cams, n_pts)
    with pytest.raises(AssertionError, match="^" + array + r"[\[ ]"):
        check_layout(ci, pi, uv, n_cams, n_pts, bad, sc)


def test_a_wrong_scalar_is_named():
    ci, pi, uv, n_cams, n_pts, lay, sc = _case("fits_2_lanes")
    for key, wrong in (("long_thr", sc["long_thr"] + 1), ("n_long", sc["n_long"] - 1), ("nblkL", sc["nblkL"] + 1), ("ppb", sc["ppb"] + 1),
                       ("cam_segl", 64), ("banded", 1 - sc["banded"]), ("cam_band", 1 - sc["cam_band"]),
                       ("lds_bytes_pinhole", sc["lds_bytes_pinhole"] + 144), ("all_lds_bal", 0)):
        with pytest.raises(AssertionError, match="^" + key + " = "):
            check_layout(ci, pi, uv, n_cams, n_pts, lay, dict(sc, **{key: wrong}))
