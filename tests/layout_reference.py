"""The layout ba_set_problem builds, stated in numpy -- independent of both builds (the host counting sorts of
csrc/ba_hip.hip and the device kernels of csrc/ba_setup.hpp, which share their grid helpers and were written to reproduce
one another).  check_layout takes the caller's arrays and what Solver.debug_layout returns and asserts what every array
and scalar must be; each assertion names the array (or scalar) and the first offending index.

What is NOT restated: the number of lanes per point and of point ranges (they follow from the chip's compute units; the
layout is checked FOR the lanes / nblkP / long_spb it reports), and the greedy bank rule of the 2-lane visiting order
(inside a point the order is then only required to be a permutation; bit-equality of the two builds covers the rule)."""
import numpy as np

ARRAYS = ("pt_off", "p_cam", "c_pt", "c_orig", "offk", "long_pts", "blk_win", "slot", "p_uv", "c_uv")
NPART = 8                                   # partitions per camera (ba_kernels.hpp)
ROW_BYTES = {"pinhole": 18 * 8, "bal": 26 * 8}   # one camera's row of the point passes' LDS table
LDS_TAB_BYTES = 150 * 1024                  # the table's budget
NO_LONG_ROWS = 0x7fffffff                   # long_thr when points have more than two lanes anyway


def table_fits(n_cams):
    return n_cams * ROW_BYTES["pinhole"] <= LDS_TAB_BYTES


def _same(name, got, want):
    """got == want element for element; names the array and the first index that differs"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape[1:] == want.shape[1:], f"{name}: shape {got.shape}, expected {want.shape}"
    n = min(got.shape[0], want.shape[0])
    bad = np.flatnonzero((got[:n] != want[:n]).reshape(n, -1).any(axis=1)) if n else np.empty(0, int)
    assert bad.size == 0, f"{name}[{bad[0]}] = {got[bad[0]]}, expected {want[bad[0]]}"
    assert got.shape[0] == want.shape[0], f"{name}[{n}]: {got.shape[0]} entries, expected {want.shape[0]}"


def _scalar(name, got, want):
    assert int(got) == int(want), f"{name} = {got}, expected {want}"


def _bits(uv, n):
    return np.ascontiguousarray(np.asarray(uv, dtype=np.float64).reshape(n, 2)).view(np.uint64)


def reference_slot(cam_idx, pt_idx, n_cams, n_pts):
    """internal point numbering: the caller's when the camera table fits in LDS, otherwise the rank of the point in a
    stable sort by the mean index of its cameras (float64; n_cams for a point nobody sees)"""
    if table_fits(n_cams):
        return np.arange(n_pts, dtype=np.int64)
    cnt = np.bincount(pt_idx, minlength=n_pts)
    total = np.bincount(pt_idx, weights=cam_idx.astype(np.float64), minlength=n_pts)   # (sums of small integers: exact)
    key = np.where(cnt > 0, total / np.maximum(cnt, 1), float(n_cams))
    slot = np.empty(n_pts, dtype=np.int64)
    slot[np.argsort(key, kind="stable")] = np.arange(n_pts)
    return slot


def check_layout(cam_idx, pt_idx, uv, n_cams, n_pts, lay, scalars):
    cam_idx = np.asarray(cam_idx, dtype=np.int64)
    pt_idx = np.asarray(pt_idx, dtype=np.int64)
    n_obs = cam_idx.size
    fits = table_fits(n_cams)
    lanes = scalars["lanes"]

    # ---- precondition: pairwise distinct pixel rows (p_src is not exposed; the pixels say which observation sits where)
    uvb = _bits(uv, n_obs)
    row_of = {}
    for i, key in enumerate(zip(uvb[:, 0].tolist(), uvb[:, 1].tolist())):
        assert key not in row_of, f"precondition: uv[{i}] repeats uv[{row_of[key]}]"
        row_of[key] = i

    # ---- slot
    slot = reference_slot(cam_idx, pt_idx, n_cams, n_pts)
    _same("slot", lay["slot"], slot)
    pt = slot[pt_idx]                                           # internal point of every caller's observation

    # ---- pt_off
    length = np.bincount(pt, minlength=n_pts)
    pt_off = np.concatenate([[0], np.cumsum(length)])
    _same("pt_off", lay["pt_off"], pt_off)
    assert pt_off[n_pts] == n_obs

    # ---- point order: position j holds the caller's observation src[j]
    p_uvb = _bits(lay["p_uv"], n_obs)
    assert np.asarray(lay["p_cam"]).shape == (n_obs,), f"p_cam: shape {np.asarray(lay['p_cam']).shape}"
    src = np.empty(n_obs, dtype=np.int64)
    for j, key in enumerate(zip(p_uvb[:, 0].tolist(), p_uvb[:, 1].tolist())):
        assert key in row_of, f"p_uv[{j}] = {np.asarray(lay['p_uv']).reshape(-1, 2)[j]} is nobody's pixel"
        src[j] = row_of[key]
    seen = np.bincount(src, minlength=n_obs)
    twice = np.flatnonzero(seen[src] > 1)
    assert twice.size == 0, f"p_uv[{twice[0]}]: observation {src[twice[0]]} sits at two positions"
    point_of_pos = np.repeat(np.arange(n_pts), length)
    # (src is a permutation by now: with the next two lines every segment holds exactly its point's observations)
    _same("p_uv (point of the observation at a position)", pt[src], point_of_pos)
    _same("p_cam", lay["p_cam"], cam_idx[src])
    if lanes != 2 or not fits:
        # the caller's order inside a point (stable); with 2 lanes and the table in LDS the visiting order is free
        _same("p_uv (caller's order inside a point)", src, np.argsort(pt, kind="stable"))
    pos_of = np.empty(n_obs, dtype=np.int64)
    pos_of[src] = np.arange(n_obs)

    # ---- camera order
    c_orig = np.asarray(lay["c_orig"], dtype=np.int64)
    assert c_orig.shape == (n_obs,), f"c_orig: shape {c_orig.shape}"
    out = np.flatnonzero((c_orig < 0) | (c_orig >= n_obs))
    assert out.size == 0, f"c_orig[{out[0]}] out of range"
    seen = np.bincount(c_orig, minlength=n_obs)
    twice = np.flatnonzero(seen[c_orig] > 1)
    assert twice.size == 0, f"c_orig[{twice[0]}] appears twice: not a permutation"
    n_of_cam = np.bincount(cam_idx, minlength=n_cams)
    cam_of_pos = np.repeat(np.arange(n_cams), n_of_cam)
    _same("c_orig (camera of the observation at a position)", cam_idx[c_orig], cam_of_pos)
    _same("c_pt", lay["c_pt"], pt[c_orig])
    c_pt = pt[c_orig]
    inside = cam_of_pos[1:] == cam_of_pos[:-1]                     # a and a + 1 belong to one camera
    down = np.flatnonzero(inside & (c_pt[1:] < c_pt[:-1]))
    assert down.size == 0, f"c_pt[{down[0] + 1}] descends inside camera {cam_of_pos[down[0]]}"
    # a point seen more than once by a camera: in the order of the positions in the point-ordered list
    tie = np.flatnonzero(inside & (c_pt[1:] == c_pt[:-1]) & (pos_of[c_orig[1:]] < pos_of[c_orig[:-1]]))
    assert tie.size == 0, f"c_orig[{tie[0] + 1}]: repeated point not in the order of the point-ordered list"
    _same("c_uv", _bits(lay["c_uv"], n_obs), uvb[c_orig])

    # ---- offk: every camera's list cut into NPART equal-count chunks
    cam_off = np.concatenate([[0], np.cumsum(n_of_cam)])
    offk = cam_off[:-1, None] + (n_of_cam[:, None] * np.arange(NPART + 1)[None, :]) // NPART
    _same("offk", np.asarray(lay["offk"]).reshape(-1), offk.reshape(-1))

    # ---- long tracks
    med = int(np.sort(length)[n_pts // 2]) if n_pts else 0
    long_thr = max(8, 2 * med) if lanes == 2 else NO_LONG_ROWS
    _scalar("long_thr", scalars["long_thr"], long_thr)
    long_pts = np.flatnonzero(length > long_thr)
    _same("long_pts", lay["long_pts"], long_pts)
    _scalar("n_long", scalars["n_long"], long_pts.size)
    long_spb = scalars["long_spb"]
    assert long_spb >= 1, f"long_spb = {long_spb}"
    _scalar("nblkL", scalars["nblkL"], -(-long_pts.size // long_spb))

    # ---- grid and windows
    nblkP, nblkL = scalars["nblkP"], scalars["nblkL"]
    assert nblkP >= 1, f"nblkP = {nblkP}"
    ppb = max(1, -(-n_pts // nblkP))
    _scalar("ppb", scalars["ppb"], ppb)
    _scalar("cam_segl", scalars["cam_segl"], 16 if n_obs // n_cams // NPART < 64 else 64)
    p_cam = cam_idx[src]

    def window(positions):
        if positions.size == 0:
            return (0, 0)
        lo, hi = int(p_cam[positions].min()), int(p_cam[positions].max())
        return (lo, hi - lo + 1)

    win = []
    for b in range(nblkP):
        p0, p1 = min(n_pts, b * ppb), min(n_pts, (b + 1) * ppb)
        win.append(window(np.arange(pt_off[p0], pt_off[p1])))
    for w in range(nblkL):
        mine = long_pts[w * long_spb:(w + 1) * long_spb]
        win.append(window(np.concatenate([np.arange(pt_off[p], pt_off[p + 1]) for p in mine]) if mine.size else np.empty(0, int)))
    win = np.array(win, dtype=np.int64).reshape(-1, 2)
    got_win = np.asarray(lay["blk_win"])
    assert got_win.size == 2 * (nblkP + nblkL), f"blk_win: {got_win.size} ints, expected {2 * (nblkP + nblkL)}"
    _same("blk_win", got_win.reshape(-1, 2), win)

    # ---- the point passes' dynamic LDS, per camera model
    for model, row in ROW_BYTES.items():
        need = win[:, 1] * row
        ok = need <= LDS_TAB_BYTES
        _scalar(f"all_lds_{model}", scalars[f"all_lds_{model}"], int(ok.all()))
        _scalar(f"lds_bytes_{model}", scalars[f"lds_bytes_{model}"], int(need[ok].max()) if ok.any() else 0)

    # ---- band statistic: mean camera span of the non-empty tracks
    span_sum, tracks = 0, 0
    if n_obs:
        order = np.argsort(pt, kind="stable")
        first = pt_off[:-1][length > 0]
        cams_by_pt = cam_idx[order]
        span_sum = int((np.maximum.reduceat(cams_by_pt, first) - np.minimum.reduceat(cams_by_pt, first)).sum())
        tracks = int((length > 0).sum())
    _scalar("banded", scalars["banded"], int(tracks > 0 and span_sum / tracks <= n_cams / 8.0))

    # ---- XCD decision: observations whose point lies in the table slice of their partition / of their camera's range;
    #      slice k of the point table is [ceil(k Np / 8), ceil((k + 1) Np / 8))
    cuts = -(-(np.arange(1, NPART + 1) * n_pts) // NPART)          # upper ends of the slices
    slice_of = np.searchsorted(cuts, c_pt, side="right")
    part_of = np.repeat(np.tile(np.arange(NPART), n_cams), np.diff(offk, axis=1).reshape(-1))
    in_partition = int((slice_of == part_of).sum())
    in_band = int((slice_of == (cam_of_pos * NPART) // n_cams).sum())
    _scalar("cam_band", scalars["cam_band"], int(in_band > in_partition))
