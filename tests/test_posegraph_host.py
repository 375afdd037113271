"""CPU: the numpy yardstick of the pose graph (tests/posegraph_reference.py) against scipy and against itself, and the host
module bundle_adjustment_amd/posegraph.py.  No GPU: close_loop runs on a double backed by the yardstick's LM mirror."""
import functools

import numpy as np
import pytest
from scipy.optimize import least_squares

from bundle_adjustment_amd import posegraph
from bundle_adjustment_amd.synthetic import make_problem
from tests import posegraph_reference as R

TIGHT = dict(ftol=1e-14, xtol=1e-14, gtol=1e-14)


@functools.lru_cache(maxsize=None)
def scene(with_scale=True, false_edge=False):
    sc = R.ring(16, with_scale)
    return R.with_false_edge(sc) if false_edge else sc


@functools.lru_cache(maxsize=None)
def mirror(loss="linear", with_scale=True, false_edge=False):
    sc = scene(with_scale, false_edge)
    return R.lm_solve(sc["start"], sc["ei"], sc["ej"], sc["meas"], sc["info"], sc["held"], loss=loss, with_scale=with_scale,
                      max_iters=50, **TIGHT)


# ---------------------------------------------------------------------------------------------------------- the yardstick
def test_closed_form_jacobians_agree_with_central_differences():
    rng = np.random.default_rng(0)
    n = 8
    poses = np.concatenate([rng.normal(0, 0.8, (n, 3)), rng.uniform(-10, 10, (n, 3)), rng.uniform(0.5, 2.0, (n, 1))], axis=1)
    poses[1, :3] = 0.0
    ei, ej = np.arange(n), (np.arange(n) + 3) % n
    noise = np.concatenate([rng.normal(0, 0.5, (n, 3)), rng.normal(0, 1.0, (n, 3)), np.exp(rng.normal(0, 0.2, (n, 1)))], axis=1)
    meas = R.compose(noise, R.relative(poses[ei], poses[ej]))
    meas[0] = R.relative(poses[ei[0]], poses[ej[0]])                 # a zero residual: the series branch
    A, B, d_fd = R.jacobians(poses, ei, ej, meas)
    Aa, Ba = R.jacobians_analytic(poses, ei, ej, meas)
    err = max(np.abs(A - Aa).max(), np.abs(B - Ba).max())
    print(f"closed form against central differences: {err:.2e} (d_fd {d_fd:.2e})")
    assert err <= 10.0 * d_fd + 1e-12


@pytest.mark.parametrize("with_scale", [True, False])
def test_mirror_reaches_scipys_minimiser_on_the_clean_ring(with_scale):
    sc = scene(with_scale)
    n = 16
    L = np.linalg.cholesky(R.RING_INFO)
    cols = 7 if with_scale else 6

    def unpack(x):
        p = sc["start"].copy()
        p[1:, :cols] = x.reshape(n - 1, cols)
        if with_scale:
            p[1:, 6] = np.exp(p[1:, 6])
        return p

    def fun(x):
        return (R.residuals(unpack(x), sc["ei"], sc["ej"], sc["meas"]) @ L).reshape(-1)
    x0 = sc["start"][1:, :cols].copy()
    if with_scale:
        x0[:, 6] = np.log(x0[:, 6])
    sp = least_squares(fun, x0.reshape(-1), x_scale="jac", ftol=1e-14, xtol=1e-14, gtol=1e-14)
    d_sp = R.pose_distance(unpack(sp.x), sc["truth"])
    ref = mirror("linear", with_scale)
    d = R.pose_distance(ref["poses"], sc["truth"])
    e0 = R.residuals(sc["start"], sc["ei"], sc["ej"], sc["meas"])
    white = float(np.sqrt(R.chi2(e0[15:16], sc["info"][15:16])[0]))
    print(f"with_scale={with_scale}: initial cost {ref['cost0']:.3f}, loop edge |e| {np.linalg.norm(e0[15]):.3f} (whitened {white:.3f}); scipy {sp.nfev} evaluations, "
          f"{d_sp:.2e} from the truth; mirror {ref['iterations']} iterations ({ref['status']}), {d:.2e}")
    assert ref["status"] != "max_iters"
    assert d <= 100.0 * d_sp + 1e-12
    if not with_scale:
        assert np.all(ref["poses"][:, 6] == 1.0)
    assert np.array_equal(ref["poses"][0], sc["start"][0])


def _fd_gradient(sc, poses, loss, mask, h):
    n = poses.shape[0]
    g = np.zeros((n, 7))
    for k in range(n):
        for c in range(7):
            if mask[k, c]:
                continue
            d = np.zeros((n, 7))
            d[k, c] = h
            g[k, c] = (R.cost(R.retract(poses, d), sc["ei"], sc["ej"], sc["meas"], sc["info"], loss)[0] -
                       R.cost(R.retract(poses, -d), sc["ei"], sc["ej"], sc["meas"], sc["info"], loss)[0]) / (2.0 * h)
    return g


@pytest.mark.parametrize("loss", R.LOSSES)
def test_robust_mirror_ends_at_a_stationary_point(loss):
    """The gradient of the robust objective at the mirror's final point, by central differences at two steps, Richardson-
    extrapolated; d_fd, the difference of the two, is the differences' own uncertainty.  Bound: the gtol the mirror ran with
    + 10 d_fd (gtol = 1e-14 itself is far below what finite differences of a cost of order 1 resolve, about 1e-7)."""
    sc = scene(True, True)
    ref = mirror(loss, True, True)
    assert ref["status"] != "max_iters", ref["status"]
    mask = R.held_mask(16, sc["ei"], sc["ej"], sc["held"], True)
    g1, g2 = _fd_gradient(sc, ref["poses"], loss, mask, 1e-5), _fd_gradient(sc, ref["poses"], loss, mask, 5e-6)
    d_fd = float(np.abs(g1 - g2).max())
    g = (4.0 * g2 - g1) / 3.0
    print(f"{loss}: final cost {ref['cost']:.6f} after {ref['iterations']} iterations ({ref['status']}); max |gradient| {np.abs(g).max():.2e} "
          f"(d_fd {d_fd:.2e})")
    assert np.abs(g).max() <= TIGHT["gtol"] + 10.0 * d_fd


@pytest.mark.parametrize("loss", R.LOSSES[1:])
def test_false_edge_stands_out_under_every_robust_loss(loss):
    sc = scene(True, True)
    _, c2, w = R.cost(mirror(loss, True, True)["poses"], sc["ei"], sc["ej"], sc["meas"], sc["info"], loss)
    assert np.argmax(c2) == len(c2) - 1
    assert np.argmin(w) == len(w) - 1 and w[-1] < w[:-1].min()


def test_cauchy_lands_closer_to_the_truth_than_least_squares():
    sc = scene(True, True)
    d = {loss: R.pose_distance(mirror(loss, True, True)["poses"], sc["truth"]) for loss in ("linear", "cauchy")}
    print(f"distance to the truth with the false edge: linear {d['linear']:.3e}, cauchy {d['cauchy']:.3e}")
    assert d["cauchy"] < d["linear"]


# ---------------------------------------------------------------------------------------------------------- posegraph.py
def _random_nodes(rng, n):
    return np.concatenate([rng.normal(0, 0.7, (n, 3)), rng.uniform(-5, 5, (n, 3)), rng.uniform(0.5, 2.0, (n, 1))], axis=1)


def test_relative_and_camera_identities():
    rng = np.random.default_rng(1)
    a, b = _random_nodes(rng, 20), _random_nodes(rng, 20)
    ms = posegraph.relative(a, b)
    assert np.allclose(ms, R.relative(a, b), rtol=0, atol=1e-13)
    assert np.abs(R.residuals(np.concatenate([a, b]), np.arange(20), np.arange(20, 40), ms)).max() <= 1e-13
    assert posegraph.relative(a[0], b[0]).shape == (7,) and np.array_equal(posegraph.relative(a[0], b[0]), ms[0])
    same = posegraph.relative(a, a)
    assert np.abs(same - np.array([0, 0, 0, 0, 0, 0, 1.0])).max() <= 1e-13
    cams = np.concatenate([a[:, :6], rng.normal(size=(20, 3))], axis=1)
    nodes = posegraph.from_cameras(cams)
    assert np.array_equal(nodes[:, :6], cams[:, :6]) and np.all(nodes[:, 6] == 1.0)
    assert np.array_equal(posegraph.to_cameras(nodes), cams[:, :6])
    # a node and its camera see every point along the same ray
    X = rng.normal(size=(20, 3)) + np.array([0, 0, 9.0])
    x = a[:, 6:7] * np.einsum("nij,nj->ni", R.rodrigues(a[:, :3]), X) + a[:, 3:6]
    c = posegraph.to_cameras(a)
    xc = np.einsum("nij,nj->ni", R.rodrigues(c[:, :3]), X) + c[:, 3:6]
    assert np.allclose(x, a[:, 6:7] * xc, rtol=0, atol=1e-12)


def test_correct_points_undoes_a_per_camera_drift():
    rng = np.random.default_rng(2)
    n, npts = 5, 40
    truth, D = _random_nodes(rng, n), _random_nodes(rng, n)
    truth[:, 6] = 1.0
    X = rng.normal(size=(npts, 3))
    ref = rng.integers(0, n, npts)
    ref[:3] = -1
    Dp = D[np.maximum(ref, 0)]
    moved = Dp[:, 6:7] * np.einsum("nij,nj->ni", R.rodrigues(Dp[:, :3]), X) + Dp[:, 3:6]
    moved[:3] = X[:3]
    drifted = R.compose(truth, R.inverse(D))
    back = posegraph.correct_points(moved, ref, drifted, truth)
    assert np.abs(back - X).max() <= 1e-12
    assert np.array_equal(back[:3], X[:3])


def test_covisibility_edges_equal_the_loop_built_version():
    rng = np.random.default_rng(3)
    n_cams, n_pts, min_shared = 6, 60, 7
    seen = rng.random((n_cams, n_pts)) < 0.45
    seen[0, :] = False
    seen[1, :] = False
    seen[0, :min_shared] = True                                   # cameras 0 and 1 share exactly min_shared points
    seen[1, :min_shared] = True
    seen[2:, :min_shared] = False
    cam_idx, pt_idx = np.nonzero(seen)
    order = rng.permutation(cam_idx.size)
    cam_idx, pt_idx = np.concatenate([cam_idx[order], cam_idx[:5]]), np.concatenate([pt_idx[order], pt_idx[:5]])   # with repeats
    poses = _random_nodes(rng, n_cams)
    want = [(i, j, int((seen[i] & seen[j]).sum())) for i in range(n_cams) for j in range(i + 1, n_cams)
            if (seen[i] & seen[j]).sum() >= min_shared]
    assert (0, 1, min_shared) in want and len(want) < n_cams * (n_cams - 1) // 2
    ei, ej, meas, info = posegraph.covisibility_edges(cam_idx, pt_idx, n_cams, poses, min_shared)
    assert list(zip(ei.tolist(), ej.tolist())) == [(i, j) for i, j, _ in want]
    assert ei.dtype == np.int32 and meas.shape == (len(want), 7) and info.shape == (len(want), 7, 7)
    for q, (i, j, c) in enumerate(want):
        assert np.array_equal(info[q], c * np.eye(7))
        assert np.array_equal(meas[q], posegraph.relative(poses[i], poses[j]))
    none = posegraph.covisibility_edges(cam_idx, pt_idx, n_cams, poses, 10 ** 6)
    assert none[0].shape == (0,) and none[2].shape == (0, 7) and none[3].shape == (0, 7, 7)


class MirrorSolver:
    """Test double of hip_backend.Solver.pose_graph backed by the yardstick's LM mirror."""

    def pose_graph(self, poses, edge_i, edge_j, meas, info=None, held=None, **opts):
        self.call = dict(poses=poses, edge_i=edge_i, edge_j=edge_j, meas=meas, info=info, held=held, opts=opts)
        out = R.lm_solve(poses, edge_i, edge_j, meas, info, held, loss=opts.get("loss", "linear"), **TIGHT)
        _, c2, w = R.cost(out["poses"], edge_i, edge_j, meas, info, opts.get("loss", "linear"))
        return dict(poses=out["poses"], status=R.STATUS_CODE[out["status"]], final_cost=out["cost"], edge_chi2=c2, edge_weight=w)


@pytest.mark.parametrize("kind", ["pinhole", "bal"])
def test_close_loop_on_a_double(kind):
    from bundle_adjustment_amd.bal import from_pinhole
    prob, cams_true, _ = make_problem(6, 150, 4, seed=8, return_truth=True, K4=np.array([900.0, 900.0, 640.0, 360.0]))
    if kind == "bal":
        prob = from_pinhole(prob)
    truth = posegraph.from_cameras(cams_true)
    s = MirrorSolver()
    out, fixed = posegraph.close_loop(prob, [5], [0], posegraph.relative(truth[5], truth[0])[None], held=(0,), solver=s, min_shared=20,
                                      loss="huber")
    m = len(out["edge_i"])
    assert m > 1 and (out["edge_i"][-1], out["edge_j"][-1]) == (5, 0) and s.call["opts"] == dict(loss="huber")
    assert np.array_equal(s.call["held"], np.array([1, 0, 0, 0, 0, 0], np.uint8))
    assert np.array_equal(s.call["info"][-1], s.call["info"][:-1, 0, 0].max() * np.eye(7))
    assert type(fixed) is type(prob) and fixed.cams.shape == prob.cams.shape and fixed.pts.shape == prob.pts.shape
    assert np.array_equal(fixed.cams[:, 6:], prob.cams[:, 6:])
    assert np.allclose(fixed.cams[:, :6], posegraph.to_cameras(out["poses"]), rtol=0, atol=0)
    assert np.array_equal(fixed.cams[0, :6], prob.cams[0, :6])
    assert not np.array_equal(fixed.pts, prob.pts)
    with pytest.raises(ValueError):
        posegraph.close_loop(prob, [5, 4], [0], posegraph.relative(truth[5], truth[0])[None], solver=s)


# ---- the Jacobian fixture ---------------------------------------------------------------------------------------------------
def _fixture_generator():
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_posegraph_jacobians.py")
    spec = importlib.util.spec_from_file_location("make_posegraph_jacobians", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_jacobian_fixture_bounds_the_closed_form():
    """tests/golden/pg_jacobians.npz: e, A, B of nine edges from 60-digit central differences of the header's residual and
    retraction.  The inputs are the generator's (the values are regenerated by the next test).  The fp64 closed form of the yardstick, held to 10 d_fd = 6e-7 by the test above,
    is measured against the fixture: the figure printed here, rounded up, is the generator's REF_REL, and 50 x REF_REL is
    what test_gpu_posegraph.py asks of the device."""
    gen = _fixture_generator()
    fix = np.load(gen.OUT)
    poses, ei, ej, meas = gen.inputs()
    for key, want in (("poses", poses), ("ei", ei), ("ej", ej), ("meas", meas), ("phi", np.array(gen.PHI))):
        assert np.array_equal(fix[key], want), key
    assert np.abs(np.linalg.norm(fix["e"][:, :3], axis=1) - fix["phi"]).max() <= 1e-15
    assert fix["phi"][3] ** 2 < 1e-4 < fix["phi"][4] ** 2                       # the two sides of the series switch
    assert np.linalg.norm(meas[:, :3], axis=1).max() <= np.pi and (np.abs(np.log(poses[ei, 6] / poses[ej, 6])) > 0.01).all()
    Aa, Ba = R.jacobians_analytic(poses, ei, ej, meas)
    jmax = max(np.abs(fix["A"]).max(), np.abs(fix["B"]).max())
    rel = max(np.abs(Aa - fix["A"]).max(), np.abs(Ba - fix["B"]).max()) / jmax
    e_err = np.abs(R.residuals(poses, ei, ej, meas) - fix["e"]).max()
    print(f"closed form against the 60-digit differences: {rel:.3e} of max |J| = {jmax:.3f}; residuals {e_err:.3e}; REF_REL {gen.REF_REL:.1e}")
    # (measured 5.16e-16 with this machine's libm; twice REF_REL leaves room for one whose sin and cos round another way)
    assert rel <= 2.0 * gen.REF_REL and gen.TOL == 50.0 * gen.REF_REL
    assert e_err <= gen.TOL


def test_jacobian_fixture_regenerates():
    """Where mpmath imports, the generator's 60-digit values are the fixture's (1e-15 relative: the differences' own error is 1e-40)."""
    pytest.importorskip("mpmath")
    gen = _fixture_generator()
    fix = np.load(gen.OUT)
    poses, ei, ej, meas = gen.inputs()
    e, A, B = gen.values(poses, ei, ej, meas)
    for key, want in (("e", e), ("A", A), ("B", B)):
        assert np.allclose(fix[key], want, rtol=1e-15, atol=1e-300), key
