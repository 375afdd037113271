"""GPU: ba_covariance -- marginal covariances of cameras and points after a solve -- against the fp64 reference of
tests/covariance_reference.py, its refusals, the handle it leaves behind, full-size problems and the BundleAdjuster drop-in."""
import os
import subprocess
import sys

import numpy as np
import pytest

from bundle_adjustment_amd import hip_backend
from bundle_adjustment_amd.hip_backend import COV_TILE
from bundle_adjustment_amd.problem import BAProblem
from oracle import ba_oracle as o
from tests import covariance_reference as cr
from tests.held_reference import Reduced
from tests.schur_cases import bal_case, pinhole_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
# c of the bound below, fixed once: the Cholesky inverse's error constant (N-independent in practice for the blocked
# algorithm) with the assembly's rounding folded in
C_COV = 256.0


def _gauge_fixed(case, rng=None):
    """fixed_cam 0 (BAL: the whole 9-parameter block) plus t[0] of camera 1; with rng, Case.hold masks and held points."""
    m = np.zeros(case.n_cams, np.uint16)
    if rng is not None:
        case.hold(rng)
        m = case.cam_mask.copy()
        m[0] = 0
    m[1] |= np.uint16(1 << 3)
    case.cam_mask = m
    return case


def _reduced(case):
    return Reduced(case.cams, case.pts, case.ci, case.pi, case.uv, case.K4, case.fixed, case.cam_mask, case.pt_held)


def check_covariance(ref, out, nb):
    """The device's Sigma against the reference's, both formed in fp64.

    Let S~ = D^-1/2 S D^-1/2 (D = diag S) and Sigma~ = D^1/2 Sigma D^1/2 = S~^-1.  The device assembles S with a
    componentwise error of a few u per entry relative to the terms that are summed (the scaled entries are O(1)), and
    inverts it by Cholesky, whose computed inverse satisfies |dSigma~| <= c u kappa(S~) ||Sigma~||_2 (Higham, ASNA 14.3;
    the error of the assembled S propagates as Sigma~ dS~ Sigma~, which has the same form).  The reference's own
    np.linalg.inv error has the same form.  Hence, entrywise, |dSigma_ij| <= C_COV u kappa(S~) ||Sigma~|| / sqrt(D_i D_j).
    A point's block is V^-1 + V^-1 W^T Sigma W V^-1: the camera error enters through |V^-1 W^T| D^-1/2 (g below) and the
    3x3 inverse adds C_COV u kappa(V) |Sigma_p|."""
    kap, nrm, dinv = cr.scaled_condition(ref["S"])
    lim = C_COV * U * kap * nrm * np.outer(dinv, dinv)
    err = np.abs(out["full"] - ref["full"])
    assert np.all(err <= lim), float((err / lim).max())
    nc = ref["cams"].shape[0]
    assert np.array_equal(out["cams"], np.array([out["full"][nb * c:nb * c + nb, nb * c:nb * c + nb] for c in range(nc)]))
    assert np.array_equal(out["full"], out["full"].T)
    free = ~np.isnan(ref["points"][:, 0, 0]) & np.any(ref["points"] != 0, axis=(1, 2))
    for p in np.nonzero(free)[0]:
        obs = np.nonzero(ref["pi"] == p)[0]
        g = np.zeros(3)
        for q in obs:
            c = ref["ci"][q]
            g += np.abs(ref["Vinv"][p] @ ref["Wobs"][q].T) @ dinv[nb * c:nb * c + nb]
        kv = np.linalg.cond(ref["Vinv"][p])
        lim_p = C_COV * U * (kap * nrm * np.outer(g, g) + kv * np.abs(ref["points"][p]))
        e = np.abs(out["points"][p] - ref["points"][p])
        assert np.all(e <= lim_p), (int(p), float((e / lim_p).max()))


def _run(case, loss):
    red = _reduced(case)
    ref = cr.schur_covariance(red, case.cams, case.pts, loss)
    ref["ci"], ref["pi"] = case.ci, case.pi
    with hip_backend.Solver(0) as s:
        intr = case.upload(s)
        out = s.covariance(loss=loss, intr=intr, full=True)
    return ref, out, red


def _cams_with(nb, rem, k=1):
    """The k-th camera count whose system N = nb Nc leaves N % COV_TILE == rem."""
    hits = [c for c in range(1, 64 * COV_TILE) if nb * c % COV_TILE == rem]
    return hits[k - 1]


# the sizes at the tile's borders, by what N = nb Nc leaves of a tile: nothing (no padding at all, every tile full; pinhole
# twice, BAL once), two rows into the next tile, one row short of a tile.  6 Nc: 32, 64, 11 cameras; 9 Nc: 64, 7 cameras.
BORDER_SIZES = {("pinhole", _cams_with(6, 0)): 0, ("pinhole", _cams_with(6, 0, 2)): 0, ("pinhole", _cams_with(6, 2)): 2,
                ("bal", _cams_with(9, COV_TILE - 1)): COV_TILE - 1, ("bal", _cams_with(9, 0)): 0}
PARITY_SIZES = [(model, n) for model in ("pinhole", "bal") for n in (3, 17, 70)] + list(BORDER_SIZES)


@pytest.mark.parametrize("model,loss,n_cams", [pytest.param(model, loss, n, id=f"{n}-{loss}-{model}")
                                               for model, n in PARITY_SIZES for loss in ("linear", "huber")])
def test_parity_with_the_reference(model, loss, n_cams):
    """N = nb Nc crosses the 64-wide tiles at every size (18 / 27, 102 / 153, 420 / 630), and at the sizes of BORDER_SIZES it
    ends on a tile's border (192, 384 and 576: no identity padding, npad == N), two rows past one (66) and one row short of
    one (63)."""
    mk = pinhole_case if model == "pinhole" else bal_case
    case = _gauge_fixed(mk(n_cams, 12 * n_cams, min(4, n_cams), seed=n_cams))
    if (model, n_cams) in BORDER_SIZES:
        assert case.nb * n_cams % COV_TILE == BORDER_SIZES[(model, n_cams)]
    else:
        assert case.nb * n_cams % COV_TILE not in (0, 1, COV_TILE - 1)
    ref, out, _ = _run(case, loss)
    check_covariance(ref, out, case.nb)
    assert np.all(np.diagonal(out["full"])[~_reduced(case).held_cam.ravel()] > 0)


@pytest.mark.parametrize("model", ["pinhole", "bal"])
def test_held_parameters_are_exact_zeros(model):
    mk = pinhole_case if model == "pinhole" else bal_case
    case = _gauge_fixed(mk(17, 200, 4, seed=4), np.random.default_rng(8))
    ref, out, red = _run(case, "huber")
    held = red.held_cam.ravel()
    assert held.sum() > case.nb + 1 and red.held_pt.any()
    assert np.all(out["full"][held] == 0.0) and np.all(out["full"][:, held] == 0.0)
    assert np.all(out["points"][red.held_pt] == 0.0)
    check_covariance(ref, out, case.nb)


def _raw(s, intr, nb, rcond=0.0):
    """ba_covariance with sentinel-filled outputs: (rc, message, cam, pts, full)."""
    cam = np.full((s.n_cams, nb * (nb + 1) // 2), 7.0)
    pts = np.full((s.n_pts, 6), 7.0)
    full = np.full((nb * s.n_cams, nb * s.n_cams), 7.0)
    lib = s._lib
    ip = None if intr is None else hip_backend._dp(intr)
    rc = lib.ba_covariance(s._h, ip, 0, 1.0, rcond, hip_backend._dp(cam), hip_backend._dp(pts), hip_backend._dp(full))
    return rc, lib.ba_last_error().decode(), cam, pts, full


@pytest.mark.parametrize("model", ["pinhole", "bal"])
def test_free_gauge_is_refused_by_camera(model):
    """Pinhole with fixed_cam only (scale free), BAL with nothing held (7 dof free): BA_ERR_NUMERIC naming a camera."""
    case = (pinhole_case(8, 120, 4, seed=2) if model == "pinhole" else bal_case(8, 120, 4, seed=2, fixed_cam=-1))
    with hip_backend.Solver(0) as s:
        intr = case.upload(s)
        rc, msg, cam, pts, full = _raw(s, intr, case.nb)
    assert rc == -4, msg
    assert "camera" in msg and "gauge" in msg
    assert np.all(cam == 7.0) and np.all(pts == 7.0) and np.all(full == 7.0)


def _without_camera(case, cam):
    """The case with every observation of camera `cam` removed (4 observations per point: every point keeps three)."""
    keep = case.ci != cam
    case.ci, case.pi, case.uv = case.ci[keep], case.pi[keep], case.uv[keep]
    assert np.bincount(case.pi, minlength=len(case.pts)).min() >= 3 and not (case.ci == cam).any()
    return case


PARAM_NAMES = ("rvec[0]", "rvec[1]", "rvec[2]", "t[0]", "t[1]", "t[2]", "f", "k1", "k2")     # the header's names of a camera's parameters
# (model, cameras, the empty camera, bits held on it, the parameter named, its row, what the row is to the tiles)
NAMED_PIVOTS = [("bal", 12, 7, 0, "rvec[0]", COV_TILE - 1, "last row of tile 0"),
                ("pinhole", 12, 10, 0b1111, "t[1]", COV_TILE, "first row of tile 1"),
                ("pinhole", _cams_with(6, 0), _cams_with(6, 0) - 1, 0, "rvec[0]", 6 * (_cams_with(6, 0) - 1), "no padding")]


@pytest.mark.parametrize("model,n_cams,empty,bits,name,row,where", NAMED_PIVOTS, ids=[c[-1].replace(" ", "-") for c in NAMED_PIVOTS])
def test_rank_test_names_the_first_failing_pivot(model, n_cams, empty, bits, name, row, where):
    """A free camera without observations has an exactly zero block in S: with the gauge fixed, its first free parameter is
    the first failing pivot, with no rounding involved.  The refusal names that camera and parameter when the pivot is the
    last row of a tile, the first row of the next, and a row of a system without padding; nothing is written; with that
    camera held the call succeeds."""
    mk = pinhole_case if model == "pinhole" else bal_case
    case = _gauge_fixed(_without_camera(mk(n_cams, 12 * n_cams, 4, seed=n_cams + 40), empty))
    nb = case.nb
    first_free = min(q for q in range(nb) if not bits >> q & 1)
    assert nb * empty + first_free == row and PARAM_NAMES[first_free] == name
    if where == "no padding":
        assert nb * n_cams % COV_TILE == 0
    else:
        assert row == {"last row of tile 0": COV_TILE - 1, "first row of tile 1": COV_TILE}[where] and nb * n_cams > COV_TILE + 1
    case.cam_mask[empty] |= np.uint16(bits)
    with hip_backend.Solver(0) as s:
        intr = case.upload(s)
        rc, msg, cam, pts, full = _raw(s, intr, nb)
        assert rc == -4, msg
        assert f"singular at camera {empty}, parameter {name} (" in msg, msg
        assert np.all(cam == 7.0) and np.all(pts == 7.0) and np.all(full == 7.0)
        case.cam_mask[empty] = np.uint16((1 << nb) - 1)
        s.set_held(cams=case.cam_mask, points=case.pt_held)
        out = s.covariance(loss="linear", intr=intr, full=True)
    ref = cr.schur_covariance(_reduced(case), case.cams, case.pts, "linear")
    ref["ci"], ref["pi"] = case.ci, case.pi
    check_covariance(ref, out, nb)
    assert np.all(out["cams"][empty] == 0.0)


def test_one_camera_point_is_nan_and_leaves_the_cameras_alone():
    case = _gauge_fixed(pinhole_case(6, 80, 4, seed=9))
    base = cr.schur_covariance(_reduced(case), case.cams, case.pts, "linear")
    o0 = int(np.nonzero(case.ci == 3)[0][0])
    case.pts = np.concatenate([case.pts, case.pts[case.pi[o0]][None] + 0.03])
    case.ci = np.append(case.ci, np.int32(3)); case.pi = np.append(case.pi, np.int32(len(case.pts) - 1))
    case.uv = np.concatenate([case.uv, case.uv[o0][None] + 0.7])
    with hip_backend.Solver(0) as s:
        case.upload(s)
        out = s.covariance(full=True)
    assert np.isnan(out["points"][-1]).all() and not np.isnan(out["points"][:-1]).any()
    base["ci"], base["pi"] = case.ci[:-1], case.pi[:-1]
    check_covariance(base, dict(full=out["full"], cams=out["cams"], points=out["points"][:-1]), 6)


def test_zero_parallax_point_is_refused_by_name_until_held():
    """Camera 2 moved onto camera 1's optical axis; a new point further down that axis is seen by both at zero parallax."""
    case = _gauge_fixed(pinhole_case(6, 80, 4, seed=12))
    R1 = o.rodrigues_batch(case.cams[1:2, :3])[0]
    C1 = -R1.T @ case.cams[1, 3:6]
    d = R1.T @ np.array([0.0, 0.0, 1.0])
    cams = case.cams.copy()
    cams[2] = cams[1]
    cams[2, 3:6] = -R1 @ (C1 + 0.5 * d)
    X = C1 + 6.0 * d
    case.cams = cams
    pts = np.concatenate([case.pts, X[None]])
    ci = np.append(case.ci, np.int32([1, 2])); pi = np.append(case.pi, np.int32([len(pts) - 1] * 2))
    uv_new = o.residuals(cams, pts, np.int32([1, 2]), np.int32([len(pts) - 1] * 2), np.zeros((2, 2)), case.K4) * -1.0
    case.pts, case.ci, case.pi = pts, ci, pi
    case.uv = np.concatenate([case.uv, uv_new])
    with hip_backend.Solver(0) as s:
        case.upload(s)
        rc, msg, cam, ptsc, full = _raw(s, None, 6)
        assert rc == -4 and f"point {len(pts) - 1}" in msg, msg
        assert np.all(cam == 7.0) and np.all(full == 7.0)
        held = np.zeros(len(pts), bool); held[-1] = True
        s.set_held(cams=case.cam_mask, points=held)
        out = s.covariance()
    assert np.all(out["points"][-1] == 0.0) and np.isfinite(out["points"][:-1]).all()


def test_camera_system_over_the_cap_is_refused():
    from bundle_adjustment_amd.synthetic import make_problem
    p = make_problem(2731, 6000, 3, seed=0)           # N = 16386
    with hip_backend.Solver(0) as s:
        s.set_problem(p)
        rc = s._lib.ba_covariance(s._h, None, 0, 1.0, 0.0, None, None, None)
        msg = s._lib.ba_last_error().decode()
    assert rc == -1 and "16384" in msg, msg


SHM_WORKER = r"""
import os, sys
sys.path.insert(0, %(root)r)
import numpy as np
import torch.distributed as dist
from bundle_adjustment_amd import hip_backend
from bundle_adjustment_amd.problem import extract_shard, shard_by_landmark
from bundle_adjustment_amd.synthetic import make_problem
dist.init_process_group("gloo")
rank, world = dist.get_rank(), dist.get_world_size()
uid = [hip_backend.comm_unique_id() if rank == 0 else None]
dist.broadcast_object_list(uid, src=0)
p = make_problem(8, 400, 4, seed=3)
b, e = shard_by_landmark(p, world)[rank]
shard, _ = extract_shard(p, b, e)
s = hip_backend.Solver(0)
s.comm_init(rank, world, uid[0])
s.set_problem(shard)
rc = s._lib.ba_covariance(s._h, None, 0, 1.0, 0.0, None, None, None)
open(os.path.join(%(out)r, f"rc_{rank}.txt"), "w").write(f"{rc} {s._lib.ba_last_error().decode()}")
s.close()
dist.barrier()
dist.destroy_process_group()
"""


def test_two_rank_job_is_refused(tmp_path):
    import socket
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = str(so.getsockname()[1])
    script = tmp_path / "cov_worker.py"
    script.write_text(SHM_WORKER % dict(root=ROOT, out=str(tmp_path)))
    env = dict(os.environ, BA_COMM="shm")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", port, str(script)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    for rank in range(2):
        rc, msg = (tmp_path / f"rc_{rank}.txt").read_text().split(" ", 1)
        assert int(rc) == -1 and "multi-rank" in msg


@pytest.mark.parametrize("model", ["pinhole", "bal"])
def test_handle_is_unchanged(model):
    case = _gauge_fixed((pinhole_case if model == "pinhole" else bal_case)(12, 300, 4, seed=21))
    kw = dict(loss="huber", max_iters=15, small_solver=1)

    def solve(with_cov):
        with hip_backend.Solver(0) as s:
            intr = case.upload(s)
            if with_cov:
                s.covariance(loss="cauchy", f_scale=2.0, intr=intr, full=True)
            if intr is None:
                summ = s.solve(**kw)
            else:
                summ = s.solve_bal_resident(intr, **kw)
            cams, pts = s.get_params()
            tr = [(r["iteration"], r["accepted"], r["pcg_iterations"], r["cost"], r["cost_trial"], r["damping"], r["step_norm"])
                  for r in s.trace()]
            return {k: v for k, v in summ.items() if not k.startswith("seconds")}, tr, cams, pts, intr

    a, b = solve(False), solve(True)
    assert a[0] == b[0] and a[1] == b[1]
    for x, y in zip(a[2:], b[2:]):
        assert (x is None and y is None) or np.array_equal(x, y)


def _backward_error(s, out, intr, held, nb, rng):
    n = out["full"].shape[0]
    Sig = out["full"]
    assert np.array_equal(Sig, Sig.T)
    dg = np.diagonal(Sig)[~held]
    assert np.all(dg > 0)
    V = rng.normal(size=(8, n))
    V[:, held] = 0.0
    X = V @ Sig
    SX = s.schur_system(0.0, X.reshape(8, -1, nb), loss="linear", intr=intr, precond=0)["sv"].reshape(8, n)
    SX[:, held] = 0.0
    # ||S||_2 by power iteration on the same operator (8 steps from a random vector: within a few % of the top eigenvalue)
    y = rng.normal(size=n)
    y[held] = 0.0
    for _ in range(8):
        y = y / np.linalg.norm(y)
        y = s.schur_system(0.0, y.reshape(-1, nb), loss="linear", intr=intr, precond=0)["sv"].ravel()
        y[held] = 0.0
    Snorm = 2.0 * np.linalg.norm(y)
    for i in range(8):
        be = np.linalg.norm(SX[i] - V[i])
        assert be <= 64 * n * U * Snorm * np.linalg.norm(X[i]), (i, be / (n * U * Snorm * np.linalg.norm(X[i])))


def _point_check(out, cams, pts, ci, pi, K4, held, nb, rng, intr=None):
    full = out["full"]
    if intr is None:
        Jc, Jp = o.jacobian_blocks(cams, pts, ci, pi, K4)
    else:
        Jc, Jp = o.bal_jacobian_blocks(np.concatenate([cams, intr], axis=1), pts, ci, pi)
    Jc = Jc * (~held.reshape(-1, nb)[ci])[:, None, :]
    order = np.argsort(pi, kind="stable")
    starts = np.searchsorted(pi[order], np.arange(len(pts) + 1))
    picked = rng.choice(len(pts), size=200, replace=False)
    for p in picked:
        obs = order[starts[p]:starts[p + 1]]
        if len(set(ci[obs].tolist())) < 2:
            assert np.isnan(out["points"][p]).all()
            continue
        V = sum(Jp[q].T @ Jp[q] for q in obs)
        Vi = np.linalg.inv(V)
        W = {q: Jc[q].T @ Jp[q] for q in obs}
        T = np.zeros((3, 3))
        for qi in obs:
            for qj in obs:
                a, b = ci[qi], ci[qj]
                T += W[qi].T @ full[nb * a:nb * a + nb, nb * b:nb * b + nb] @ W[qj]
        ref = Vi + Vi @ T @ Vi
        np.testing.assert_allclose(out["points"][p], ref, rtol=1e-6, atol=1e-9 * np.abs(ref).max())


def test_full_size_c3():
    from bundle_adjustment_amd.synthetic import make_config
    p = make_config("C3")
    m = np.zeros(p.n_cams, np.uint16); m[1] = 1 << 3
    rng = np.random.default_rng(0)
    with hip_backend.Solver(0) as s:
        s.set_problem(BAProblem(p.cams, p.pts, p.cam_idx, p.pt_idx, p.uv, p.K4, 0))
        s.set_held(cams=m)
        out = s.covariance(full=True)
        held = np.zeros((p.n_cams, 6), bool); held[0] = True; held[1, 3] = True
        _backward_error(s, out, None, held.ravel(), 6, rng)
    _point_check(out, p.cams, p.pts, p.cam_idx, p.pt_idx, p.K4, held.ravel(), 6, rng)


def test_full_size_config5_bal():
    from bundle_adjustment_amd.synthetic import make_bal_problem
    b = make_bal_problem()
    rng = np.random.default_rng(1)
    m = np.zeros(b.n_cams, np.uint16); m[1] = 1 << 3
    with hip_backend.Solver(0) as s:
        intr = s._set_bal(b, 0)
        s.set_held(cams=m)
        out = s.covariance(intr=intr, full=True)
        held = np.zeros((b.n_cams, 9), bool); held[0] = True; held[1, 3] = True
        _backward_error(s, out, intr, held.ravel(), 9, rng)
    _point_check(out, np.ascontiguousarray(b.cams[:, :6]), b.pts, b.cam_idx, b.pt_idx, None, held.ravel(), 9, rng,
                 intr=b.cams[:, 6:9])


@pytest.mark.parametrize("name", ["run_seed0", "run_seed1", "run_global"])
def test_bundle_adjuster_leaves_the_covariances_of_the_window(name):
    import io
    from contextlib import redirect_stdout
    from bundle_adjustment_amd import BundleAdjuster
    from tests.helpers import load_golden, rebuild_map
    g = load_golden(name)
    maps, adjusters = [], []
    for cov in (False, True):
        gmap = rebuild_map(g)
        ba = BundleAdjuster(g["K"], window_size=int(g["window_size"]), fixed_keyframes=2, covariance=cov)
        with redirect_stdout(io.StringIO()):
            ba.run(gmap)
        maps.append(gmap)
        adjusters.append(ba)
    ba = adjusters[1]
    cov = ba.last_covariance
    w = int(g["window_size"])
    local = sorted(maps[1].keyframes)[-(w + 1):-1]
    assert sorted(cov["keyframes"]) == local[2:]
    mp_ids, _, _ = ba._gather_local_data(maps[1], local)
    assert sorted(cov["points"]) == sorted(int(i) for i in mp_ids)
    for a, b in zip(sorted(maps[0].keyframes), sorted(maps[1].keyframes)):
        assert np.array_equal(maps[0].keyframes[a].R, maps[1].keyframes[b].R)
        assert np.array_equal(maps[0].keyframes[a].t, maps[1].keyframes[b].t)
    for i in maps[0].map_points:
        assert np.array_equal(maps[0].map_points[i].position, maps[1].map_points[i].position)
    # the same numbers through Solver.covariance on the window the adjuster holds (same parameters, same loss)
    again = ba._solver.covariance(loss="huber")
    assert len(cov["keyframes"]) == again["cams"].shape[0] - 2
    for i, kf in enumerate(local[2:]):
        np.testing.assert_allclose(cov["keyframes"][kf], again["cams"][2 + i], rtol=1e-9, atol=0)
    vals = np.array(list(cov["points"].values()))
    nan = np.isnan(vals[:, 0, 0])
    assert np.all(np.isnan(vals[nan])) and np.all(np.isfinite(vals[~nan]))
    for a in adjusters:
        a.close()
