"""GPU: the layout ba_set_problem builds -- by the host (BA_SETUP=host) and by the device (BA_SETUP=device, csrc/ba_setup.hpp)
-- against the numpy statement of it (tests/layout_reference.py) and against one another, bit for bit, at the edges of the
device build: scans and camera tiles at whole blocks, the ends of the three segment-sort paths of a point (16 | 17, 64 | 65)
and of the two of a camera (12 288 | 12 289 keys), cameras and points nobody sees, repeated pairs, one point; the hand-back
to the host build, the automatic choice at 50 000 observations, and a handle that builds one problem after another.

Integers and pixel bits only: no tolerance anywhere.  Every problem takes its cameras and points from make_problem (pixels:
the true projections plus noise, float32-valued, pairwise distinct) so that the two-iteration solve that follows stays finite."""
import functools

import numpy as np
import pytest

from bundle_adjustment_amd import hip_backend
from bundle_adjustment_amd.problem import BAProblem
from bundle_adjustment_amd.rotations import rvecs_to_matrices
from bundle_adjustment_amd.synthetic import make_problem
from tests.layout_reference import ARRAYS, check_layout, table_fits

pytestmark = pytest.mark.gpu

RANK_LDS = 12288                  # SETUP_RANK_LDS: keys of a camera the workgroup rank sort stages in LDS
TRACK_LENGTHS = (0, 1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 300)


# ------------------------------------------------------------------------------------------------------------- problems
def _pixels(cams, pts, K4, ci, pi, rng):
    """projections of the true scene plus N(0, 0.5), rounded to float32, rows made pairwise distinct"""
    R = rvecs_to_matrices(cams[:, :3])
    Xc = np.einsum('nij,nj->ni', R[ci], pts[pi]) + cams[ci, 3:]
    assert Xc[:, 2].min() > 0.5
    uv = np.stack([K4[0] * Xc[:, 0] / Xc[:, 2] + K4[2], K4[1] * Xc[:, 1] / Xc[:, 2] + K4[3]], axis=1)
    uv = (uv + rng.normal(0.0, 0.5, uv.shape)).astype(np.float32)
    while True:
        _, first = np.unique(uv, axis=0, return_index=True)
        if first.size == uv.shape[0]:
            return uv.astype(np.float64)
        again = np.setdiff1d(np.arange(uv.shape[0]), first)
        uv[again, 0] += (rng.integers(1, 4096, again.size) / 64.0).astype(np.float32)


def _build(n_cams, n_pts, ci, pi, seed, n_obs=None):
    """the observations (ci, pi) of make_problem's scene, shuffled, trimmed to n_obs when given"""
    rng = np.random.default_rng(seed)
    base, cams_true, pts_true = make_problem(n_cams, n_pts, 1, seed=seed, return_truth=True)
    ci, pi = np.asarray(ci, dtype=np.int32), np.asarray(pi, dtype=np.int32)
    perm = rng.permutation(ci.size)[:n_obs]
    ci, pi = np.ascontiguousarray(ci[perm]), np.ascontiguousarray(pi[perm])
    return BAProblem(base.cams, base.pts, ci, pi, _pixels(cams_true, pts_true, base.K4, ci, pi, rng), base.K4, 0).validate()


def _distinct_cameras(rng, n_pts, cams, k):
    """(n_pts, k): k distinct cameras of `cams` per point"""
    cams = np.asarray(cams)
    return cams[np.argsort(rng.random((n_pts, cams.size)), axis=1)[:, :k]]


def _tracks(per_point):
    """observation lists of a list of per-point camera arrays"""
    pi = np.repeat(np.arange(len(per_point)), [len(t) for t in per_point])
    return np.concatenate([np.asarray(t, dtype=np.int64) for t in per_point]), pi


def _scan_edge(n_pts, n_cams):
    rng = np.random.default_rng(n_pts + n_cams)
    return _build(n_cams, n_pts, _distinct_cameras(rng, n_pts, np.arange(n_cams), 3).reshape(-1), np.repeat(np.arange(n_pts), 3), seed=n_pts)


def _tile_edge(n_obs):
    rng = np.random.default_rng(77)
    return _build(9, 3000, _distinct_cameras(rng, 3000, np.arange(9), 3).reshape(-1), np.repeat(np.arange(3000), 3), seed=77, n_obs=n_obs)


def _track_lengths():
    n_cams, n_pts = 320, 1500
    rng = np.random.default_rng(31)
    lens = np.full(n_pts, 3)
    special = np.repeat(TRACK_LENGTHS, 3)
    where = rng.choice(np.arange(1, n_pts - 1), special.size - 2, replace=False)
    lens[0] = lens[n_pts - 1] = 0                       # nobody sees the first point or the last
    lens[where] = special[2:]                           # (the third 0-length point and everything else: anywhere between)
    return _build(n_cams, n_pts, *_tracks([rng.choice(n_cams, n, replace=False) for n in lens]), seed=31)


def _empty_cameras():
    n_cams, n_pts = 12, 2000                            # cameras 0, 5 and 11 see nothing, camera 3 sees one point once
    rng = np.random.default_rng(41)
    ci = _distinct_cameras(rng, n_pts, [1, 2, 4, 6, 7, 8, 9, 10], 3).reshape(-1)
    pi = np.repeat(np.arange(n_pts), 3)
    return _build(n_cams, n_pts, np.append(ci, 3), np.append(pi, 1234), seed=41)


HEAVY = {1: RANK_LDS, 2: RANK_LDS + 1, 3: 13000}        # camera: observations


def _heavy_cameras():
    n_cams, n_pts = 12, 13000
    rng = np.random.default_rng(51)
    ci, pi = [], []
    for c in range(n_cams):
        n = HEAVY.get(c, 200 + 37 * c)
        ci.append(np.full(n, c)); pi.append(rng.choice(n_pts, n, replace=False))
    return _build(n_cams, n_pts, np.concatenate(ci), np.concatenate(pi), seed=51)


def _duplicates():
    n_pts = 3000
    rng = np.random.default_rng(61)
    ci = _distinct_cameras(rng, n_pts, np.arange(9), 3).reshape(-1)
    pi = np.repeat(np.arange(n_pts), 3)
    again = rng.choice(ci.size, 400, replace=False)     # these pairs are given three times (own pixels each: _pixels)
    return _build(9, n_pts, np.concatenate([ci, ci[again], ci[again]]), np.concatenate([pi, pi[again], pi[again]]), seed=61)


def _hand_back():
    """12 points, each seen 2 100 times by 9 cameras: median track length 2 100, long_thr 4 200 -- past what the device
    build's capped track-length histogram can count"""
    rng = np.random.default_rng(71)
    return _build(9, 12, rng.integers(0, 9, 12 * 2100), np.repeat(np.arange(12), 2100), seed=71)


def _auto(n_cams, n_obs):
    rng = np.random.default_rng(n_cams)
    if n_cams < 1000:
        n_pts = 20400
        ci, pi = _distinct_cameras(rng, n_pts, np.arange(n_cams), 3).reshape(-1), np.repeat(np.arange(n_pts), 3)
    else:
        # camera table past LDS: the points are renumbered by the mean index of their cameras.  Half of the tracks lie in a
        # band of 30 cameras, half anywhere; points 10 .. 19 repeat the cameras of point 5 (equal keys: the sort is stable)
        # and three points are seen by nobody (key n_cams: they come last, in the caller's order)
        n_pts = 6100
        per_point = []
        for p in range(n_pts):
            if p % 2:
                per_point.append(rng.integers(0, n_cams - 30) + rng.choice(30, 10, replace=False))
            else:
                per_point.append(rng.choice(n_cams, 10, replace=False))
        for p in range(10, 20):
            per_point[p] = rng.permutation(per_point[5])
        for p in (100, 2000, n_pts - 1):
            per_point[p] = np.empty(0, dtype=np.int64)
        for p in range(3000, 3000 + 2 * (sum(len(t) for t in per_point) - n_obs), 2):   # down to n_obs: these lose a view each
            per_point[p] = per_point[p][:-1]
        ci, pi = _tracks(per_point)
        assert ci.size == n_obs
    return _build(n_cams, n_pts, ci, pi, seed=n_cams, n_obs=n_obs)


BUILDERS = {
    **{f"scan_{n_pts}_pts_{n_cams}_cams": functools.partial(_scan_edge, n_pts, n_cams)
       for n_pts in (4095, 4096, 4097, 8192, 8193) for n_cams in (9, 257)},
    **{f"tile_{n_obs}_obs": functools.partial(_tile_edge, n_obs) for n_obs in (4095, 4096, 4097, 8192)},
    "track_lengths": _track_lengths,
    "empty_cameras": _empty_cameras,
    "heavy_cameras": _heavy_cameras,
    "duplicates": _duplicates,
    "single_seen_once": lambda: _build(9, 1, [4], [0], seed=81),
    "single_seen_by_all": lambda: _build(9, 1, np.arange(9), np.zeros(9, int), seed=82),
    "hand_back": _hand_back,
}


@functools.lru_cache(maxsize=None)
def _problem(case):
    p = BUILDERS[case]()
    for a in (p.cams, p.pts, p.cam_idx, p.pt_idx, p.uv):
        a.setflags(write=False)
    return p


# ------------------------------------------------------------------------------------------------------------- builds
def _environment(monkeypatch, mode, lanes):
    for name in ("BA_SETUP", "BA_PT_LANES", "BA_PT_BLOCKS", "BA_LONG_SLOTS", "BA_PIXELS"):
        monkeypatch.delenv(name, raising=False)
    if mode:
        monkeypatch.setenv("BA_SETUP", mode)
    if lanes:
        monkeypatch.setenv("BA_PT_LANES", str(lanes))


def _read(s):
    return {k: s.debug_layout(k) for k in ARRAYS}, s.debug_layout("scalars")


def _solve(s):
    out = s.solve(loss="huber", max_iters=2, ftol=0.0, xtol=0.0, gtol=0.0)
    return out, s.get_params()


_FRESH = {}


def _fresh(monkeypatch, case, mode, lanes):
    """layout, scalars, solve result and parameters of `case` built on a handle of its own (computed once)"""
    key = (case, mode, lanes)
    if key not in _FRESH:
        _environment(monkeypatch, mode, lanes)
        with hip_backend.Solver(0) as s:
            s.set_problem(_problem(case))
            _FRESH[key] = _read(s) + _solve(s)
    return _FRESH[key]


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)


def _same_layout(a, b, what):
    (lay_a, sc_a), (lay_b, sc_b) = a, b
    for k in sc_a:
        if k != "build_path":
            assert sc_a[k] == sc_b[k], (what, k, sc_a[k], sc_b[k])
    for k in ARRAYS:
        assert lay_a[k].shape == lay_b[k].shape, (what, k, lay_a[k].shape, lay_b[k].shape)
        x, y = (_bits(lay_a[k]), _bits(lay_b[k])) if k.endswith("uv") else (lay_a[k], lay_b[k])
        bad = np.flatnonzero(x != y)
        assert bad.size == 0, (what, k, int(bad[0]), lay_a[k][bad[0]], lay_b[k][bad[0]])


def _same_solve(a, b, what):
    (out_a, par_a), (out_b, par_b) = a, b
    assert np.array_equal(_bits(out_a["final_cost"]), _bits(out_b["final_cost"])), (what, out_a["final_cost"], out_b["final_cost"])
    assert out_a["pcg_iterations"] == out_b["pcg_iterations"], what
    assert np.array_equal(_bits(par_a[0]), _bits(par_b[0])) and np.array_equal(_bits(par_a[1]), _bits(par_b[1])), what


def _check(p, lay, sc):
    check_layout(p.cam_idx, p.pt_idx, p.uv, p.n_cams, p.n_pts, lay, sc)


CASES = [(c, None) for c in BUILDERS if c not in ("hand_back", "track_lengths", "duplicates")]
CASES += [("track_lengths", 2), ("track_lengths", None), ("duplicates", 2), ("duplicates", None)]


@pytest.mark.parametrize("case,lanes", CASES, ids=[c + ("_2_lanes" if ln else "") for c, ln in CASES])
def test_both_builds_match_the_reference_and_one_another(case, lanes, monkeypatch):
    p = _problem(case)
    host = _fresh(monkeypatch, case, "host", lanes)
    dev = _fresh(monkeypatch, case, "device", lanes)
    assert host[1]["build_path"] == 0 and dev[1]["build_path"] == 1
    sc = dev[1]
    if lanes:
        assert sc["lanes"] == lanes
    # the problem is the one the case is meant to be
    n_of_cam = np.bincount(p.cam_idx, minlength=p.n_cams)
    n_of_pt = np.bincount(p.pt_idx, minlength=p.n_pts)
    if case.startswith("scan_"):
        assert case == f"scan_{p.n_pts}_pts_{p.n_cams}_cams" and np.all(n_of_pt == 3)
    elif case.startswith("tile_"):
        assert case == f"tile_{p.n_obs}_obs"
    elif case == "track_lengths":
        assert n_of_pt[0] == 0 and n_of_pt[-1] == 0
        for n in TRACK_LENGTHS:
            assert np.count_nonzero(n_of_pt == n) >= 3, n
        pairs = p.cam_idx.astype(np.int64) * p.n_pts + p.pt_idx
        assert np.unique(pairs).size == pairs.size
        if lanes == 2:                                  # median 3: tracks of more than 8 observations get rows of their own
            assert sc["long_thr"] == 8 and sc["n_long"] == 30 and sc["nblkL"] > 0
        else:
            assert sc["lanes"] != 2 and sc["n_long"] == 0
    elif case == "empty_cameras":
        assert list(n_of_cam[[0, 3, 5, 11]]) == [0, 1, 0, 0]
    elif case == "heavy_cameras":                       # 12 288 keys: the last segment sorted in LDS; 12 289 and 13 000: from memory
        assert {c: int(n_of_cam[c]) for c in HEAVY} == HEAVY and np.delete(n_of_cam, list(HEAVY)).max() < 1000
    elif case == "duplicates":
        pairs = p.cam_idx.astype(np.int64) * p.n_pts + p.pt_idx
        assert np.count_nonzero(np.unique(pairs, return_counts=True)[1] == 3) == 400
    else:
        assert p.n_pts == 1 and p.n_obs == {"single_seen_once": 1, "single_seen_by_all": 9}[case]
    _check(p, *host[:2])
    _check(p, *dev[:2])
    _same_layout(dev[:2], host[:2], case)
    _same_solve(dev[2:], host[2:], case)


def test_device_build_hands_a_problem_past_its_histogram_back_to_the_host_build(monkeypatch):
    p = _problem("hand_back")
    assert np.all(np.bincount(p.pt_idx) == 2100)
    host = _fresh(monkeypatch, "hand_back", "host", 2)
    dev = _fresh(monkeypatch, "hand_back", "device", 2)
    assert host[1]["build_path"] == 0 and dev[1]["build_path"] == 0
    assert dev[1]["lanes"] == 2 and dev[1]["long_thr"] == 4200 and dev[1]["n_long"] == 0
    _check(p, *host[:2])
    _check(p, *dev[:2])
    _same_layout(dev[:2], host[:2], "hand_back")
    _same_solve(dev[2:], host[2:], "hand_back")
    assert np.isfinite(dev[2]["final_cost"]) and dev[2]["final_cost"] <= dev[2]["initial_cost"]


@pytest.mark.parametrize("n_cams,n_obs,path", [(20, 49999, 0), (20, 50000, 1), (8, 60000, 0), (1100, 60000, 0)],
                         ids=["below_the_threshold", "at_the_threshold", "too_few_cameras", "table_past_lds"])
def test_automatic_choice_of_the_build(n_cams, n_obs, path, monkeypatch):
    p = _auto(n_cams, n_obs)
    assert p.n_obs == n_obs and p.n_cams == n_cams
    _environment(monkeypatch, None, None)
    with hip_backend.Solver(0) as s:
        s.set_problem(p)
        lay, sc = _read(s)
    assert sc["build_path"] == path
    if n_cams == 1100:                                  # the only case with a renumbered point table
        assert not table_fits(n_cams) and not np.array_equal(lay["slot"], np.arange(p.n_pts))
        n = np.bincount(p.pt_idx, minlength=p.n_pts)
        key = np.bincount(p.pt_idx, weights=p.cam_idx, minlength=p.n_pts)[n > 0] / n[n > 0]
        assert np.count_nonzero(n == 0) == 3 and np.unique(key).size <= key.size - 10      # points nobody sees; equal keys
        _check(p, lay, sc)
    elif n_cams == 20:
        _check(p, lay, sc)


def test_one_handle_builds_one_problem_after_another(monkeypatch):
    """the device build works in scratch kept from call to call (a hand-bounded memset, flagged index buffers doubling as
    seg / p_pt / d_cam / d_pt): smaller after larger, host between device builds, and every result is a fresh handle's"""
    steps = [("scan_8193_pts_9_cams", "device", None), ("scan_4095_pts_257_cams", "device", None), ("track_lengths", "host", 2),
             ("heavy_cameras", "device", None), ("single_seen_by_all", "device", None)]
    fresh = [_fresh(monkeypatch, *step) for step in steps]
    with hip_backend.Solver(0) as s:
        for (case, mode, lanes), want in zip(steps, fresh):
            _environment(monkeypatch, mode, lanes)
            s.set_problem(_problem(case))
            got = _read(s)
            assert got[1]["build_path"] == want[1]["build_path"] == (mode == "device"), case
            _same_layout(got, want[:2], "reused handle: " + case)
            _check(_problem(case), *got)
        _same_solve(_solve(s), fresh[-1][2:], "reused handle: solve")
