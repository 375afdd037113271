"""GPU: ba_pose_graph / ba_pose_graph_system against the numpy yardstick of tests/posegraph_reference.py.

Tolerances.  Residuals 1e-12 absolute (about 60 rounded fp64 operations on values up to 10).  Jacobians 10 d_fd + 1e-12,
d_fd the difference of the yardstick's two finite-difference steps.  H against the sum formed in numpy from the device's
own A, B: 1e-12 of its largest entry.  Costs against the dense LM mirror (exact inner solve on both sides): COST_RTOL
relative plus the round-off floor of a cost that is a sum of squares of residuals known to E_ROUND each,
sqrt(2 lambda_max(info) cost 7 m) E_ROUND -- a cost of 1e-17 is made of residuals of 1e-10, which fp64 arithmetic on poses of
size 10 knows to four digits only (measured there: 3.4e-4 relative).  Distances to the truth: 100 x the mirror's own + 1e-12."""
import functools
import math
import os

import numpy as np
import pytest

from bundle_adjustment_amd import hip_backend, posegraph
from bundle_adjustment_amd.hip_backend import PG_CHUNK_MIN, PG_HUB_CHUNKS, PG_HUB_MIN, PG_MAX_BLOCKS, PG_TEAMS, PG_THREADS, pg_chunk_len
from bundle_adjustment_amd.problem import BAProblem
from bundle_adjustment_amd.synthetic import make_problem
from tests import posegraph_reference as R

pytestmark = pytest.mark.gpu
COST_RTOL = 1e-10         # 10 x the worst relative difference measured among costs above 1e-9 x the initial one (9.5e-12)
E_ROUND = 1e-13
TIGHT = dict(ftol=1e-14, xtol=1e-14, gtol=1e-14)
MIRROR_TIGHT = dict(ftol=1e-14, xtol=1e-14, gtol=1e-14)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def cost_bound(cost, m, lam_max):
    return COST_RTOL * abs(cost) + math.sqrt(2.0 * lam_max * abs(cost) * 7 * m) * E_ROUND


def lam_max(info):
    return 1.0 if info is None else float(np.linalg.eigvalsh(info).max())


def exact(n, sweeps=1):
    """An inner solve that is exact for practical purposes: CG ends after 7 n iterations in exact arithmetic.  In fp64 the
    257-node chain, whose loop-wide mode puts the condition number near 1e8, needs 1.6 x that (measured: 2856 iterations), and
    an inner solve that runs into its cap raises ba_solve's damping floor, which the mirror's exact solve never does: the
    shapes get sweeps = 4."""
    return dict(pcg_tol=1e-13, pcg_max_iters=7 * n * sweeps)


@pytest.fixture(scope="module")
def solver():
    import __graft_entry__ as g
    g.build()
    with hip_backend.Solver(0) as s:
        yield s


# ------------------------------------------------------------------------------------------------------------ scenes
@functools.lru_cache(maxsize=None)
def system_scene(with_scale=True):
    """9 nodes / 14 edges: a duplicated pair, an edge with i > j, a node with rvec = 0, a residual rotation of 3.0 rad, scales in
    0.5 .. 2 with |t| <= 10, random full-rank information blocks and a rotation-only one, a held node (4), an isolated one (8)."""
    rng = np.random.default_rng(11)
    n = 9
    poses = np.zeros((n, 7))
    poses[:, :3] = rng.normal(0.0, 0.8, (n, 3))
    poses[2, :3] = 0.0
    poses[:, 3:6] = rng.uniform(-10.0, 10.0, (n, 3))
    poses[:, 6] = rng.uniform(0.5, 2.0, n) if with_scale else 1.0
    pairs = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 6), (6, 7), (7, 0), (0, 1), (5, 2), (1, 3), (6, 2), (7, 4), (3, 0)]
    ei = np.array([p[0] for p in pairs], np.int32)
    ej = np.array([p[1] for p in pairs], np.int32)
    m = len(pairs)
    noise = np.concatenate([rng.normal(0.0, 0.3, (m, 3)), rng.normal(0.0, 0.5, (m, 3)),
                            np.exp(rng.normal(0.0, 0.2, (m, 1))) if with_scale else np.ones((m, 1))], axis=1)
    meas = R.compose(noise, R.relative(poses[ei], poses[ej]))
    # edge 4: R_ij^T R_r = exp(phi), |phi| = 3.0
    phi = 3.0 * np.array([0.6, -0.48, 0.64])
    Rr = R.rodrigues(poses[ej[4], :3]) @ R.rodrigues(poses[ei[4], :3]).T
    meas[4, :3] = R.log_map(Rr @ R.rodrigues(phi).T)
    M = rng.normal(0.0, 1.0, (m, 7, 7))
    info = M @ np.swapaxes(M, 1, 2) + np.eye(7)
    info[6] = 0.0
    info[6, :3, :3] = M[6, :3, :3] @ M[6, :3, :3].T + np.eye(3)      # rotation only: rank 3
    held = np.zeros(n, np.uint8)
    held[4] = 1
    return dict(poses=poses, ei=ei, ej=ej, meas=meas, info=info, held=held)


@functools.lru_cache(maxsize=None)
def ring(with_scale=True, false_edge=False):
    sc = R.ring(16, with_scale)
    return R.with_false_edge(sc) if false_edge else sc


@functools.lru_cache(maxsize=None)
def mirror(name, loss="linear", with_scale=True):
    sc = SCENES[name](with_scale) if name in ("ring", "false") else SCENES[name]()
    return R.lm_solve(sc["start"], sc["ei"], sc["ej"], sc["meas"], sc["info"], sc["held"], loss=loss, with_scale=with_scale,
                      max_iters=50, **MIRROR_TIGHT)


def chain_scene():
    """257 nodes on a circle, odometry edges and the loop edge: more than 256 edges, more teams than a workgroup holds."""
    n = 257
    truth = R.circle_poses(n, 20.0)
    ei = np.arange(n, dtype=np.int32)
    ej = ((np.arange(n) + 1) % n).astype(np.int32)
    held = np.zeros(n, np.uint8)
    held[0] = 1
    start = R.drifted_start(truth, True, scale=1.0004, rot=(0.0, 2e-4, 5e-5), shift=1e-3)
    return dict(truth=truth, start=start, ei=ei, ej=ej, meas=R.relative(truth[ei], truth[ej]),
                info=np.broadcast_to(R.RING_INFO, (n, 7, 7)).copy(), held=held)


def star_scene():
    """Node 0 with 300 incident edges to 300 leaves plus a ring over the leaves: an incidence list longer than a wave and than
    one chunk.  info = None (the identity)."""
    rng = np.random.default_rng(5)
    n = 301
    truth = np.concatenate([np.array([[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]]), R.circle_poses(300, 8.0)])
    leaves = np.arange(1, n)
    ei = np.concatenate([np.zeros(300, np.int64), leaves]).astype(np.int32)
    ej = np.concatenate([leaves, np.roll(leaves, -1)]).astype(np.int32)
    d = np.concatenate([rng.normal(0.0, 0.02, (n, 3)), rng.normal(0.0, 0.1, (n, 3)), rng.normal(0.0, 0.03, (n, 1))], axis=1)
    d[0] = 0.0
    held = np.zeros(n, np.uint8)
    held[0] = 1
    return dict(truth=truth, start=R.retract(truth, d), ei=ei, ej=ej, meas=R.relative(truth[ei], truth[ej]), info=None, held=held)


def tiny_scene():
    truth = R.circle_poses(2)
    start = truth.copy()
    start[1, 3:6] += 0.3
    start[1, 6] = 1.2
    return dict(truth=truth, start=start, ei=np.array([0], np.int32), ej=np.array([1], np.int32),
                meas=R.relative(truth[:1], truth[1:]), info=None, held=np.array([1, 0], np.uint8))


SCENES = dict(ring=lambda ws=True: ring(ws), false=lambda ws=True: ring(ws, True), chain=functools.lru_cache(None)(chain_scene),
              star=functools.lru_cache(None)(star_scene), tiny=functools.lru_cache(None)(tiny_scene))


def run(s, sc, **opts):
    return s.pose_graph(sc["start"], sc["ei"], sc["ej"], sc["meas"], info=sc["info"], held=sc["held"], **opts)


# ------------------------------------------------------------------------------------------------------------ 1: system
@pytest.mark.parametrize("with_scale", [True, False])
def test_system(solver, with_scale):
    sc = system_scene(with_scale)
    n, m = 9, 14
    ref = R.system(sc["poses"], sc["ei"], sc["ej"], sc["meas"], sc["info"], sc["held"], "huber", 1.5, with_scale, lam=0.3)
    got = solver.pose_graph_system(sc["poses"], sc["ei"], sc["ej"], sc["meas"], info=sc["info"], held=sc["held"], lam=0.3,
                                   loss="huber", f_scale=1.5, with_scale=with_scale)
    e_err = float(np.abs(got["e"] - ref["e"]).max())
    j_err = max(float(np.abs(got["A"] - ref["A"]).max()), float(np.abs(got["B"] - ref["B"]).max()))
    print(f"pose_graph_system: max |e - e_ref| {e_err:.2e}; max |J - J_fd| {j_err:.2e} (d_fd {ref['d_fd']:.2e}); "
          f"largest rotation residual {np.linalg.norm(ref['e'][:, :3], axis=1).max():.3f} rad")
    assert abs(np.linalg.norm(ref["e"][4, :3]) - 3.0) < 1e-9
    assert e_err <= 1e-12
    assert j_err <= 10.0 * ref["d_fd"] + 1e-12
    H, g, _ = R.dense_system(n, sc["ei"], sc["ej"], got["e"], got["A"], got["B"], sc["info"], ref["w"], ref["mask"], lam=0.3)
    h_err = float(np.abs(got["H"] - H).max() / np.abs(H).max())
    g_err = float(np.abs(got["g"] - g).max() / np.abs(g).max())
    print(f"  H relative {h_err:.2e}, g relative {g_err:.2e}")
    assert h_err <= 1e-12 and g_err <= 1e-12
    assert same_bits(got["H"], got["H"].T)
    rows = np.flatnonzero(ref["mask"].reshape(-1))
    assert rows.size == (14 if with_scale else 14 + 7)
    assert np.array_equal(got["H"][rows], np.eye(7 * n)[rows]) and np.array_equal(got["H"][:, rows], np.eye(7 * n)[:, rows])
    assert np.all(got["g"][rows] == 0.0)


# ------------------------------------------------------------------------------------------------------------ 1b: hubs, edge grid
N_ORDINARY = 40
# degrees of the chosen nodes 0 .. 5: one short of a hub and the largest node that is none; a hub whose last chunk holds one
# edge; 64 chunks of 16; chunk length 17; chunk length 65 in 64 chunks, the last one short
CHOSEN_DEGREES = (PG_HUB_MIN - 1, PG_HUB_MIN, PG_HUB_MIN + 1, PG_HUB_CHUNKS * PG_CHUNK_MIN, PG_HUB_CHUNKS * PG_CHUNK_MIN + 1,
                  PG_HUB_CHUNKS * PG_HUB_CHUNKS + 1)


@functools.lru_cache(maxsize=None)
def multigraph_scene(with_scale=True):
    """48 nodes, m = 2 PG_MAX_BLOCKS PG_TEAMS + 5 edges (the edge pass makes a third, partly filled trip), parallel edges
    throughout.  Nodes 0 .. 5 have the CHOSEN_DEGREES, nodes 6 and 7 are two further hubs that take the rest, nodes 8 .. 47 are
    ordinary: a ring among themselves plus ten edges from every chosen node.  Each chosen node's other edges alternate between
    the two further hubs, and the remaining edges join those two.  Edges in random order and random direction (i > j on about
    half); poses, noise and information blocks as in system_scene: generic rotations, |t| <= 10, scales 0.5 .. 2, random
    full-rank info and a rotation-only one, node 12 held."""
    rng = np.random.default_rng(31)
    n = 8 + N_ORDINARY
    m = 2 * PG_MAX_BLOCKS * PG_TEAMS + 5
    h1, h2, first = 6, 7, 8
    pairs = [(first + k, first + (k + 1) % N_ORDINARY) for k in range(N_ORDINARY)]
    for c, deg in enumerate(CHOSEN_DEGREES):
        pairs += [(c, first + (10 * c + k) % N_ORDINARY) for k in range(10)]
        pairs += [(c, h1 if k % 2 else h2) for k in range(deg - 10)]
    assert len(pairs) < m
    pairs += [(h1, h2)] * (m - len(pairs))
    pairs = np.array(pairs)[rng.permutation(m)]
    flip = rng.random(m) < 0.5
    ei = np.where(flip, pairs[:, 1], pairs[:, 0]).astype(np.int32)
    ej = np.where(flip, pairs[:, 0], pairs[:, 1]).astype(np.int32)
    poses = np.zeros((n, 7))
    poses[:, :3] = rng.normal(0.0, 0.8, (n, 3))
    poses[:, 3:6] = rng.uniform(-10.0, 10.0, (n, 3))
    poses[:, 6] = rng.uniform(0.5, 2.0, n) if with_scale else 1.0
    noise = np.concatenate([rng.normal(0.0, 0.3, (m, 3)), rng.normal(0.0, 0.5, (m, 3)),
                            np.exp(rng.normal(0.0, 0.2, (m, 1))) if with_scale else np.ones((m, 1))], axis=1)
    meas = R.compose(noise, R.relative(poses[ei], poses[ej]))
    M = rng.normal(0.0, 1.0, (m, 7, 7))
    info = M @ np.swapaxes(M, 1, 2) + np.eye(7)
    info[6] = 0.0
    info[6, :3, :3] = M[6, :3, :3] @ M[6, :3, :3].T + np.eye(3)      # rotation only: rank 3
    held = np.zeros(n, np.uint8)
    held[12] = 1
    return dict(poses=poses, ei=ei, ej=ej, meas=meas, info=info, held=held)


def check_multigraph_borders(sc):
    """The degree list, the hubs and their chunks, the trips of the edge pass: what the scene is for."""
    n, m = sc["poses"].shape[0], len(sc["ei"])
    deg = np.bincount(np.concatenate([sc["ei"], sc["ej"]]), minlength=n)
    assert 7 * n <= 4096 and m == 2 * PG_MAX_BLOCKS * PG_TEAMS + 5
    assert -(-m // (PG_MAX_BLOCKS * PG_TEAMS)) == 3 and m % (PG_MAX_BLOCKS * PG_TEAMS) == 5
    assert tuple(deg[:6]) == CHOSEN_DEGREES
    hubs = np.flatnonzero(deg > PG_HUB_MIN)
    assert hubs.tolist() == [2, 3, 4, 5, 6, 7] and int((deg <= PG_HUB_MIN).sum()) == n - 6 == 42
    assert deg[8:].max() < PG_HUB_MIN and deg[8:].min() >= 2
    chunks = {int(k): (pg_chunk_len(int(deg[k])), -(-int(deg[k]) // pg_chunk_len(int(deg[k]))), int(deg[k]) % pg_chunk_len(int(deg[k]))) for k in hubs}
    assert chunks[2] == (PG_CHUNK_MIN, 5, 1)                                   # 65 edges: four chunks of 16 and one edge
    assert chunks[3] == (PG_CHUNK_MIN, PG_HUB_CHUNKS, 0) and chunks[4] == (PG_CHUNK_MIN + 1, 61, 5)
    assert chunks[5] == (PG_HUB_CHUNKS + 1, PG_HUB_CHUNKS, 2)                  # 4097 edges: 63 chunks of 65 and one of 2
    assert all(c[1] <= PG_HUB_CHUNKS for c in chunks.values()) and min(chunks[6][0], chunks[7][0]) > PG_HUB_CHUNKS + 1
    assert (sc["ei"] > sc["ej"]).sum() > 1000 and (sc["ei"] < sc["ej"]).sum() > 1000
    return deg


@pytest.mark.parametrize("with_scale", [True, False])
def test_system_multigraph(solver, with_scale):
    """test_system on the multigraph scene: hubs of every chunk geometry and three trips of the edge pass.  e, A, B against the
    closed form in numpy (absolute 1e-12, as there with d_fd = 0); H and g against the sums formed in numpy from the device's
    own e, A, B, 1e-12 of the largest entry -- test_system's bound, which holds at degree 13 152 too (measured: H 7.0e-15,
    g 3.7e-15), so no componentwise bound replaces it."""
    sc = multigraph_scene(with_scale)
    deg = check_multigraph_borders(sc)
    n, m = sc["poses"].shape[0], len(sc["ei"])
    ref = R.system(sc["poses"], sc["ei"], sc["ej"], sc["meas"], sc["info"], sc["held"], "huber", 1.5, with_scale, lam=0.3, analytic=True)
    got = solver.pose_graph_system(sc["poses"], sc["ei"], sc["ej"], sc["meas"], info=sc["info"], held=sc["held"], lam=0.3,
                                   loss="huber", f_scale=1.5, with_scale=with_scale)
    e_err = float(np.abs(got["e"] - ref["e"]).max())
    j_err = max(float(np.abs(got["A"] - ref["A"]).max()), float(np.abs(got["B"] - ref["B"]).max()))
    print(f"multigraph system ({m} edges, degrees up to {deg.max()}): max |e - e_ref| {e_err:.2e}; max |J - J_ref| {j_err:.2e} "
          f"(max |J| {max(np.abs(ref['A']).max(), np.abs(ref['B']).max()):.1f}); weights below 1: {(ref['w'] < 1).mean():.2f}")
    assert (ref["w"] < 1).any()
    assert e_err <= 1e-12
    assert j_err <= 10.0 * ref["d_fd"] + 1e-12 and ref["d_fd"] == 0.0
    H, g, _ = R.dense_system(n, sc["ei"], sc["ej"], got["e"], got["A"], got["B"], sc["info"], ref["w"], ref["mask"], lam=0.3)
    h_err = float(np.abs(got["H"] - H).max() / np.abs(H).max())
    g_err = float(np.abs(got["g"] - g).max() / np.abs(g).max())
    print(f"  H relative {h_err:.2e}, g relative {g_err:.2e}")
    assert h_err <= 1e-12 and g_err <= 1e-12
    assert same_bits(got["H"], got["H"].T)
    rows = np.flatnonzero(ref["mask"].reshape(-1))
    assert rows.size == (7 if with_scale else 7 + (n - 1))
    assert np.array_equal(got["H"][rows], np.eye(7 * n)[rows]) and np.array_equal(got["H"][:, rows], np.eye(7 * n)[:, rows])
    assert np.all(got["g"][rows] == 0.0)


def test_jacobians_to_fp64_accuracy(solver):
    """e, A, B of the nine edges of tests/golden/pg_jacobians.npz -- residual rotations 0, 1e-9, 1e-5, both sides of the series
    switch at 0.01, 1, 3, pi - 1e-3, pi - 1e-6 -- against central differences in 60-digit arithmetic, to 50 x the error the
    fp64 closed form of the yardstick has against the same values (tests/golden/make_posegraph_jacobians.py says why)."""
    import importlib.util
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    spec = importlib.util.spec_from_file_location("make_posegraph_jacobians", os.path.join(golden, "make_posegraph_jacobians.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)                              # (for its constants: only the fixture's values are used here)
    fix = np.load(os.path.join(golden, "pg_jacobians.npz"))
    tol = gen.TOL
    assert tol == 50.0 * 5.2e-16
    got = solver.pose_graph_system(fix["poses"], fix["ei"], fix["ej"], fix["meas"])
    jmax = max(float(np.abs(fix["A"]).max()), float(np.abs(fix["B"]).max()))
    a_err, b_err = float(np.abs(got["A"] - fix["A"]).max()), float(np.abs(got["B"] - fix["B"]).max())
    e_err = float(np.abs(got["e"] - fix["e"]).max())
    per_edge = np.maximum(np.abs(got["A"] - fix["A"]).max(axis=(1, 2)), np.abs(got["B"] - fix["B"]).max(axis=(1, 2)))
    print(f"Jacobians against the 60-digit differences: A {a_err:.2e}, B {b_err:.2e} (bound {tol * jmax:.2e}, max |J| {jmax:.3f}); "
          f"e {e_err:.2e} (bound {tol:.2e}); per edge " + " ".join(f"{v:.1e}" for v in per_edge))
    assert fix["phi"][3] ** 2 < 1e-4 < fix["phi"][4] ** 2 and len(fix["phi"]) == 9
    assert a_err <= tol * jmax and b_err <= tol * jmax
    assert e_err <= tol


# ------------------------------------------------------------------------------------------------------------ 2: clean ring
@pytest.mark.parametrize("with_scale", [True, False])
def test_clean_ring(solver, with_scale):
    sc = ring(with_scale)
    ref = mirror("ring", "linear", with_scale)
    out = run(solver, sc, with_scale=with_scale, **TIGHT)
    d_ref, d = R.pose_distance(ref["poses"], sc["truth"]), R.pose_distance(out["poses"], sc["truth"])
    print(f"clean ring, with_scale={with_scale}: {out['iterations']} LM / {out['pcg_iterations']} PCG iterations, status "
          f"{out['status_name']}, distance to the truth {d:.2e} (mirror {d_ref:.2e})")
    assert out["status"] != 0
    assert d <= 100.0 * d_ref + 1e-12
    assert same_bits(out["poses"][0], sc["start"][0])
    if not with_scale:
        assert np.all(out["poses"][:, 6] == 1.0)


# ------------------------------------------------------------------------------------------------------------ 3: trace
def follow(out, trace, ref, m, lmax):
    """The same number of LM iterations; accept / reject sequence equal and per-iteration costs within cost_bound while the
    cost is above 1e-18 x the initial one.  -> (worst relative cost difference there, the worst among costs above 1e-9 x the
    initial one, where the round-off floor of cost_bound is below its relative term)."""
    assert out["iterations"] == ref["iterations"] == len(trace), (out["iterations"], ref["iterations"], len(trace))
    worst, worst_large = 0.0, 0.0
    for t, h in zip(trace, ref["history"]):
        if h["cost"] <= 1e-18 * ref["cost0"]:
            break
        assert t["accepted"] == bool(h["rho"] > 0), (t, h)
        for a, b in ((t["cost"], h["cost"]), (t["cost_trial"], h["cost_new"])):
            rel = abs(a - b) / max(abs(b), 1e-300)
            worst = max(worst, rel)
            if b >= 1e-9 * ref["cost0"]:
                worst_large = max(worst_large, rel)
            assert abs(a - b) <= cost_bound(b, m, lmax), (t, h)
    return worst, worst_large


@pytest.mark.parametrize("with_scale", [True, False])
def test_trace_follows_mirror(solver, with_scale):
    sc = ring(with_scale)
    ref = mirror("ring", "linear", with_scale)
    out = run(solver, sc, with_scale=with_scale, **TIGHT, **exact(16))
    worst, worst_large = follow(out, solver.pose_graph_trace(), ref, len(sc["ei"]), 100.0)
    print(f"trace, with_scale={with_scale}: {out['iterations']} iterations (mirror {ref['iterations']}); worst relative cost "
          f"difference {worst:.2e}, {worst_large:.2e} among costs above 1e-9 x the initial one")
    assert abs(out["initial_cost"] - ref["cost0"]) <= cost_bound(ref["cost0"], len(sc["ei"]), 100.0)


# ------------------------------------------------------------------------------------------------------------ 4: false edge
@pytest.mark.parametrize("loss", R.LOSSES)
def test_false_edge(solver, loss):
    sc = ring(True, True)
    ref = mirror("false", loss)
    out = run(solver, sc, loss=loss, **TIGHT, **exact(16))
    worst, worst_large = follow(out, solver.pose_graph_trace(), ref, len(sc["ei"]), 100.0)
    print(f"false edge, {loss}: worst relative cost difference over the iterations {worst:.2e}")
    rel = abs(out["final_cost"] - ref["cost"]) / ref["cost"]
    print(f"false edge, {loss}: final cost {out['final_cost']:.12e} (mirror {ref['cost']:.12e}, relative {rel:.2e}), "
          f"{out['iterations']} / {ref['iterations']} iterations; false edge chi2 {out['edge_chi2'][-1]:.3f} weight {out['edge_weight'][-1]:.4f}")
    assert abs(out["final_cost"] - ref["cost"]) <= cost_bound(ref["cost"], len(sc["ei"]), 100.0)
    _, c2, w = R.cost(out["poses"], sc["ei"], sc["ej"], sc["meas"], sc["info"], loss)
    assert np.allclose(out["edge_chi2"], c2, rtol=1e-9, atol=1e-12) and np.allclose(out["edge_weight"], w, rtol=1e-9)
    if loss != "linear":
        assert np.argmax(out["edge_chi2"]) == len(sc["ei"]) - 1
        assert np.argmin(out["edge_weight"]) == len(sc["ei"]) - 1 and out["edge_weight"][-1] < out["edge_weight"][:-1].min()


def test_cauchy_is_closer_to_the_truth_than_linear(solver):
    sc = ring(True, True)
    d = {loss: R.pose_distance(run(solver, sc, loss=loss, **TIGHT, **exact(16))["poses"], sc["truth"]) for loss in ("linear", "cauchy")}
    print(f"false edge: distance to the truth linear {d['linear']:.3e}, cauchy {d['cauchy']:.3e}")
    assert d["cauchy"] < d["linear"]


# ------------------------------------------------------------------------------------------------------------ 5: shapes
def test_one_node_no_edge(solver):
    p = np.array([[0.1, -0.2, 0.3, 1.0, 2.0, 3.0, 1.5]])
    out = solver.pose_graph(p, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 7)))
    assert same_bits(out["poses"], p) and out["status"] == 3 and out["final_cost"] == 0.0 and out["initial_cost"] == 0.0
    assert out["edge_chi2"].shape == (0,) and out["iterations"] == 0


@pytest.mark.parametrize("name", ["tiny", "chain", "star"])
def test_shapes(solver, name):
    sc = SCENES[name]()
    n, m = sc["start"].shape[0], len(sc["ei"])
    ref = mirror(name)
    out = run(solver, sc, **TIGHT, **exact(n, 4))
    print(f"{name}: n {n}, m {m}: {out['iterations']} LM / {out['pcg_iterations']} PCG iterations, status {out['status_name']}; final "
          f"cost {out['final_cost']:.3e} (mirror {ref['cost']:.3e}, {ref['iterations']} iterations, {ref['status']})")
    assert out["status"] != 0
    assert abs(out["final_cost"] - ref["cost"]) <= cost_bound(ref["cost"], m, lam_max(sc["info"])) + 1e-18 * ref["cost0"]
    d_ref, d = R.pose_distance(ref["poses"], sc["truth"]), R.pose_distance(out["poses"], sc["truth"])
    print(f"  distance to the truth {d:.2e} (mirror {d_ref:.2e})")
    assert d <= 100.0 * d_ref + 1e-12


def test_star_bits_do_not_depend_on_the_split(solver):
    """BA_DEBUG_PG_SPLITS (read when the handle is created): the hub's list shared by 1 and by 7 teams instead of 32."""
    sc = star_scene()
    ref = run(solver, sc, **exact(301, 4))
    old = os.environ.get("BA_DEBUG_PG_SPLITS")
    try:
        for k in (1, 7):
            os.environ["BA_DEBUG_PG_SPLITS"] = str(k)
            with hip_backend.Solver(0) as s:
                out = run(s, sc, **exact(301, 4))
            for key in ("poses", "edge_chi2", "edge_weight"):
                assert same_bits(out[key], ref[key]), (k, key)
            assert out["final_cost"] == ref["final_cost"] and out["pcg_iterations"] == ref["pcg_iterations"]
    finally:
        if old is None:
            os.environ.pop("BA_DEBUG_PG_SPLITS", None)
        else:
            os.environ["BA_DEBUG_PG_SPLITS"] = old


def test_multigraph_bits_do_not_depend_on_the_split(solver):
    """The split test on the multigraph scene, whose hubs have chunks of 16, 17, 65 and some 200 edges and short last chunks:
    the dense system and three LM iterations with 1 and 7 teams per hub give the bits of the default 32."""
    sc = multigraph_scene(True)
    check_multigraph_borders(sc)
    args = (sc["poses"], sc["ei"], sc["ej"], sc["meas"])
    kw = dict(info=sc["info"], held=sc["held"], loss="huber", f_scale=1.5)
    ref_sys = solver.pose_graph_system(*args, lam=0.3, **kw)
    ref = solver.pose_graph(*args, max_iters=3, **kw)
    assert ref["pcg_iterations"] > 0 and ref["final_cost"] < ref["initial_cost"]
    old = os.environ.get("BA_DEBUG_PG_SPLITS")
    try:
        for k in (1, 7):
            os.environ["BA_DEBUG_PG_SPLITS"] = str(k)
            with hip_backend.Solver(0) as s:
                out_sys = s.pose_graph_system(*args, lam=0.3, **kw)
                out = s.pose_graph(*args, max_iters=3, **kw)
            for key in ("H", "g"):
                assert same_bits(out_sys[key], ref_sys[key]), (k, key)
            for key in ("poses", "edge_chi2", "edge_weight"):
                assert same_bits(out[key], ref[key]), (k, key)
            assert out["final_cost"] == ref["final_cost"] and out["pcg_iterations"] == ref["pcg_iterations"]
    finally:
        if old is None:
            os.environ.pop("BA_DEBUG_PG_SPLITS", None)
        else:
            os.environ["BA_DEBUG_PG_SPLITS"] = old


# ------------------------------------------------------------------------------------------------------------ 5b: node grids
NODE_GRID_SIZES = (PG_MAX_BLOCKS * PG_TEAMS, PG_MAX_BLOCKS * PG_TEAMS + 1, PG_MAX_BLOCKS * PG_THREADS, PG_MAX_BLOCKS * PG_THREADS + 1)
U = 2.0 ** -53


@pytest.mark.parametrize("n", NODE_GRID_SIZES)
def test_node_grids(solver, n):
    """Rings of PG_MAX_BLOCKS PG_TEAMS and PG_MAX_BLOCKS PG_THREADS nodes and one more: the last node is the second trip of the
    grid-stride loops of the node passes (a team per node) and of the step kernel (a thread per node); the edge pass makes
    its second trip at every size.  Six LM iterations under Huber; the dense mirror cannot follow at this size, so what a
    vectorised reference certifies at the returned poses: chi2 and weight of every edge, their sum, the initial cost, the held
    nodes, a decrease of the cost and of the gradient, and the bits of a second call."""
    sc = R.big_ring(n)
    m = len(sc["ei"])
    teams, threads = PG_MAX_BLOCKS * PG_TEAMS, PG_MAX_BLOCKS * PG_THREADS
    assert (-(-n // teams), -(-n // threads)) == {teams: (1, 1), teams + 1: (2, 1), threads: (8, 1), threads + 1: (9, 2)}[n]
    assert m > teams and np.bincount(np.concatenate([sc["ei"], sc["ej"]])).max() <= 4 < PG_HUB_MIN        # no hubs
    loss, fs = "huber", 0.02
    lmax = lam_max(sc["info"][0])
    gtol = 1e-8
    opts = dict(loss=loss, f_scale=fs, max_iters=6, gtol=gtol)
    out = run(solver, sc, **opts)
    again = run(solver, sc, **opts)
    print(f"ring of {n} nodes / {m} edges: {out['iterations']} LM / {out['pcg_iterations']} PCG iterations, status {out['status_name']}, "
          f"cost {out['initial_cost']:.6e} -> {out['final_cost']:.6e}")
    cost0, _, w0 = R.cost(sc["start"], sc["ei"], sc["ej"], sc["meas"], sc["info"], loss, fs)
    assert abs(out["initial_cost"] - cost0) <= cost_bound(cost0, m, lmax)
    cost1, c2, w = R.cost(out["poses"], sc["ei"], sc["ej"], sc["meas"], sc["info"], loss, fs)
    per_edge = COST_RTOL * c2 + np.sqrt(2.0 * lmax * c2 * 7) * E_ROUND                # cost_bound of one edge
    d_c2 = np.abs(out["edge_chi2"] - c2)
    assert np.all(d_c2 <= per_edge), float((d_c2 / per_edge).max())
    # Huber's w = min(1, (chi2 / f_scale^2)^-1/2) has |dw / w| <= |d chi2 / chi2| / 2
    assert np.all(np.abs(out["edge_weight"] - w) * c2 <= w * per_edge)
    assert 0.02 < (w < 1).mean() < 0.98                 # (the weights compared above are not all 1)
    assert abs(out["final_sse"] - c2.sum()) <= cost_bound(c2.sum(), m, lmax)
    assert abs(out["final_cost"] - cost1) <= cost_bound(cost1, m, lmax)
    held = sc["held"] != 0
    assert held.sum() == n // 64 and not held[n - 1] and same_bits(out["poses"][held], sc["start"][held])
    assert not same_bits(out["poses"][n - 1], sc["start"][n - 1])                       # the last node moved too
    assert out["final_cost"] < out["initial_cost"] and out["accepted"] > 0
    for key in ("poses", "edge_chi2", "edge_weight"):
        assert same_bits(out[key], again[key]), key
    assert out["final_cost"] == again["final_cost"] and out["pcg_iterations"] == again["pcg_iterations"]
    # the gradient at the returned poses: a term is two inner products of length 7 of factors known to a few u each
    mask = R.held_mask(n, sc["ei"], sc["ej"], sc["held"])
    g0, _ = R.gradient(sc["start"], sc["ei"], sc["ej"], sc["meas"], sc["info"], w0, mask)
    g1, g1_abs = R.gradient(out["poses"], sc["ei"], sc["ej"], sc["meas"], sc["info"], w, mask)
    print(f"  max |g| over the free parameters {np.abs(g0).max():.3e} -> {np.abs(g1).max():.3e}")
    if out["status_name"] == "gtol":
        assert np.all(np.abs(g1) <= gtol + 64.0 * U * g1_abs)
    else:
        assert np.abs(g1).max() < np.abs(g0).max()


# ------------------------------------------------------------------------------------------------------------ 6: reproducibility
def test_two_calls_give_the_same_bits(solver):
    sc = ring(True, True)
    a, b = run(solver, sc, loss="cauchy"), run(solver, sc, loss="cauchy")
    for key in ("poses", "edge_chi2", "edge_weight"):
        assert same_bits(a[key], b[key]), key
    assert a["final_cost"] == b["final_cost"] and a["pcg_iterations"] == b["pcg_iterations"]


def test_permuted_edges_give_the_same_minimiser(solver):
    """(the sums run in list order, so the bits may differ: the minimiser may not)"""
    sc = ring(True)
    perm = np.random.default_rng(2).permutation(len(sc["ei"]))
    a = run(solver, sc, **TIGHT, **exact(16))
    b = solver.pose_graph(sc["start"], sc["ei"][perm], sc["ej"][perm], sc["meas"][perm], info=sc["info"][perm],
                          held=sc["held"], **TIGHT, **exact(16))
    d = R.pose_distance(a["poses"], b["poses"])
    print(f"permuted edge order: distance between the two minimisers {d:.2e}")
    assert d <= 100.0 * R.pose_distance(mirror("ring")["poses"], sc["truth"]) + 1e-12


# ------------------------------------------------------------------------------------------------------------ 7: resident problem
def test_resident_problem_is_untouched(solver):
    prob = make_problem(8, 200, 4, seed=4)
    kw = dict(loss="huber", max_iters=8, small_solver=1)
    with hip_backend.Solver(0) as s:
        s.set_problem(prob)
        base = s.solve(**kw)
        base_params = s.get_params()
        base_trace = s.trace()
        s.set_params(prob.cams, prob.pts)
        before = s.get_params()
        run(s, ring(True))
        after = s.get_params()
        assert same_bits(before[0], after[0]) and same_bits(before[1], after[1])
        assert len(s.trace()) == len(base_trace)
        again = s.solve(**kw)
        params = s.get_params()
    assert again["final_cost"] == base["final_cost"] and again["iterations"] == base["iterations"]
    assert same_bits(params[0], base_params[0]) and same_bits(params[1], base_params[1])


# ------------------------------------------------------------------------------------------------------------ 8: errors
def _refused(solver, field, sc=None, **change):
    sc = dict(ring(True) if sc is None else sc)
    opts = change.pop("opts", {})
    for k, v in change.items():
        sc[k] = v
    with pytest.raises(hip_backend.BAHipError) as err:
        solver.pose_graph(sc["start"], sc["ei"], sc["ej"], sc["meas"], info=sc["info"], held=sc["held"], **opts)
    assert field in str(err.value), str(err.value)


def test_refusals_name_the_field(solver):
    sc = ring(True)

    def changed(key, idx, value):
        a = np.array(sc[key], dtype=sc[key].dtype)
        a[idx] = value
        return {key: a}
    _refused(solver, "edge_i == edge_j", **changed("ei", 3, sc["ej"][3]))
    _refused(solver, "edge_i[2]", **changed("ei", 2, 16))
    _refused(solver, "edge_j[5]", **changed("ej", 5, -1))
    _refused(solver, "poses[7]", **changed("start", (7, 4), np.nan))
    _refused(solver, "meas[1]", **changed("meas", (1, 0), np.inf))
    _refused(solver, "info[4]", **changed("info", (4, 2, 2), np.nan))
    _refused(solver, "poses[3]: the scale", **changed("start", (3, 6), 0.0))
    _refused(solver, "meas[6]: the scale", **changed("meas", (6, 6), -1.0))
    _refused(solver, "poses[2]: |rvec|", **changed("start", (2, slice(0, 3)), np.array([math.pi + 1e-6, 0.0, 0.0])))
    asym = sc["info"].copy()
    asym[9, 0, 1] += 1e-6
    _refused(solver, "info[9] is not symmetric", info=asym)
    neg = sc["info"].copy()
    neg[10, 6, 6] = -1.0
    _refused(solver, "info[10] is not positive semidefinite", info=neg)
    _refused(solver, "unknown loss", opts=dict(loss=7))
    _refused(solver, "f_scale", opts=dict(f_scale=0.0))
    _refused(solver, "max_iters", opts=dict(max_iters=-1))
    _refused(solver, "pcg_max_iters", opts=dict(pcg_max_iters=-1))
    _refused(solver, "ftol", opts=dict(ftol=-1e-3))
    _refused(solver, "xtol", opts=dict(xtol=-1e-3))
    _refused(solver, "gtol", opts=dict(gtol=-1e-3))
    _refused(solver, "pcg_tol", opts=dict(pcg_tol=-0.5))
    _refused(solver, "pcg_min_iters", opts=dict(pcg_min_iters=-1))
    _refused(solver, "initial_lambda", opts=dict(initial_lambda=0.0))
    _refused(solver, "initial_lambda", opts=dict(initial_lambda=-1e-4))
    # negative counts: the Python layer takes n and m from the arrays, so through the symbol itself
    import ctypes as C
    o = solver.posegraph_options()
    p7 = np.ascontiguousarray(sc["start"])
    for n_, m_, field in ((-1, 0, "n must not be negative"), (16, -1, "m must not be negative")):
        rc = solver._lib.ba_pose_graph(solver._h, n_, hip_backend._dp(p7), m_, None, None, None, None, None, C.byref(o), None, None, None, None)
        assert rc == -1 and field in solver._lib.ba_last_error().decode(), solver._lib.ba_last_error()
    _refused(solver, "with_scale = 0", opts=dict(with_scale=False))              # the Sim(3) start has scales off 1
    se3 = dict(ring(False))
    m6 = se3["meas"].copy()
    m6[0, 6] = 1.0 + 1e-12
    _refused(solver, "meas[0]: with_scale = 0", sc=se3, meas=m6, opts=dict(with_scale=False))
    with pytest.raises(ValueError):
        solver.posegraph_options(loss="l2")
    with pytest.raises(ValueError):
        solver.posegraph_options(damping=1.0)
    big = np.tile(sc["start"][:1], (586, 1))
    with pytest.raises(hip_backend.BAHipError) as err:
        solver.pose_graph_system(big, sc["ei"], sc["ej"], sc["meas"])
    assert "n = 586" in str(err.value)
    out = run(solver, sc)                                                        # the handle is still usable
    assert out["status"] != 0 and out["final_cost"] < 1e-3 * out["initial_cost"]


# ------------------------------------------------------------------------------------------------------------ 9: end to end
def test_close_loop_end_to_end(solver):
    """12 cameras / 300 points; camera k moved by its own similarity D_k (the accumulated drift, D_0 = identity), each point by
    the D of its first observer; odometry and loop measurements from the truth."""
    prob, cams_true, pts_true = make_problem(12, 300, 4, seed=6, return_truth=True, pixel_sigma=0.0)
    n = 12
    truth = posegraph.from_cameras(cams_true)
    k = np.arange(n)[:, None]
    D = np.concatenate([k * np.array([[0.002, 0.004, -0.001]]), k * np.array([[0.03, -0.01, 0.02]]), 1.0 + 0.01 * k], axis=1)
    drifted_nodes = R.compose(truth, R.inverse(D))                      # S_k o D_k^-1: sees D_k X as S_k sees X
    ref_cam = posegraph.first_observers(prob.cam_idx, prob.pt_idx, 300)
    Dp = D[ref_cam]
    pts = Dp[:, 6:7] * np.einsum("nij,nj->ni", R.rodrigues(Dp[:, :3]), pts_true) + Dp[:, 3:6]
    drifted = BAProblem(posegraph.to_cameras(drifted_nodes), pts, prob.cam_idx, prob.pt_idx, prob.uv, prob.K4, 0)
    li = np.concatenate([np.arange(n - 1), [n - 1]]).astype(np.int32)
    lj = np.concatenate([np.arange(1, n), [0]]).astype(np.int32)
    out, fixed = posegraph.close_loop(drifted, li, lj, R.relative(truth[li], truth[lj]), held=(0,), solver=solver, min_shared=10 ** 9,
                                      **TIGHT)
    sc = dict(start=posegraph.from_cameras(drifted.cams), ei=li, ej=lj, meas=R.relative(truth[li], truth[lj]), info=None,
              held=np.eye(1, n, 0, dtype=np.uint8)[0])
    ref = R.lm_solve(sc["start"], li, lj, sc["meas"], None, sc["held"], max_iters=50, **MIRROR_TIGHT)
    d_ref = R.pose_distance(ref["poses"], truth)
    d = R.pose_distance(posegraph.from_cameras(fixed.cams), truth)
    sse = []
    with hip_backend.Solver(0) as s:
        for p in (drifted, fixed):
            s.set_problem(p)
            sse.append(s.residuals("linear")[1])
    print(f"close_loop: status {out['status_name']}, cameras within {d:.2e} of the truth (mirror {d_ref:.2e}); reprojection SSE "
          f"{sse[0]:.4e} -> {sse[1]:.4e} (ratio {sse[1] / sse[0]:.3e})")
    assert out["status"] != 0
    assert d <= 100.0 * d_ref + 1e-12
    assert sse[1] < sse[0]
