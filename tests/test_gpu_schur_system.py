"""GPU: the reduced camera system of one LM iteration (ba_schur_system) -- right-hand side g, preconditioner blocks Minv
and the operator product S v in the PCG loop's launch form -- against the fp64 reference of the oracle, componentwise
(bounds: tests/schur_cases.check_system), for the pinhole and the BAL camera, fp64 and fp32 Jacobian blocks, linear /
Huber / Cauchy losses with one-component outliers, Jacobi / Schur-Jacobi / kept Schur-Jacobi blocks and held
parameters; each layout shape asserts the kernel variant it is meant to reach."""
import numpy as np
import pytest

from tests import schur_cases as sc

pytestmark = pytest.mark.gpu
LAM = 1e-3


@pytest.fixture(scope="module")
def solver():
    from bundle_adjustment_amd import hip_backend
    s = hip_backend.Solver(0)
    yield s
    s.close()


def run(s, case, loss="huber", precision=0, precond=1, n_vec=3, lam_prev=None, seed=0):
    intr = case.upload(s)
    v = np.random.default_rng(seed).normal(size=(n_vec, case.n_cams, case.nb))
    out = s.schur_system(LAM, v, loss=loss, intr=intr, precond=precond, lam_prev=lam_prev, jacobian_precision=precision)
    sysr, w = case.reference(loss, LAM)
    prev = case.reference(loss, lam_prev)[0] if precond == 2 else None
    sc.check_system(case, out, sysr, w, v, precision, precond, prev)
    return out, v, sysr


_SMALL = {"pinhole": lambda: sc.pinhole_case(17, 900, 5, seed=3), "bal": lambda: sc.bal_case(17, 900, 5, seed=3)}


@pytest.mark.parametrize("precond", [0, 1, 2])
@pytest.mark.parametrize("loss", ["linear", "huber", "cauchy"])
@pytest.mark.parametrize("precision", [0, 1], ids=["f64", "f32"])
@pytest.mark.parametrize("model", ["pinhole", "bal"])
def test_reduced_system_with_held_parameters(solver, model, precision, loss, precond):
    case = _SMALL[model]().hold(np.random.default_rng(11))
    run(solver, case, loss, precision, precond, lam_prev=1e-2 if precond == 2 else None)
    assert solver.debug_layout("scalars")["cam_segl"] == 16


def _one_obs_cameras(case):
    """The last camera keeps one observation, the one before it two: every other partition of theirs is empty."""
    keep = np.ones(len(case.ci), bool)
    for c, n in ((case.n_cams - 1, 1), (case.n_cams - 2, 2)):
        idx = np.nonzero(case.ci == c)[0]
        keep[idx[n:]] = False
    case.ci, case.pi, case.uv = case.ci[keep], case.pi[keep], case.uv[keep]
    return case


def _long_tracks(case, n=60):
    """n points seen by every camera (pixels from the model, small noise): tracks past the long-track threshold."""
    from oracle import ba_oracle as o
    from bundle_adjustment_amd.synthetic import bal_project
    seen = set(zip(case.ci.tolist(), case.pi.tolist()))
    ci, pi = zip(*[(c, p) for p in range(n) for c in range(case.n_cams) if (c, p) not in seen])
    ci, pi = np.array(ci, np.int32), np.array(pi, np.int32)
    if case.K4 is None:
        uv = bal_project(case.cams, case.pts, ci, pi)
    else:
        uv = -o.residuals(case.cams, case.pts, ci, pi, np.zeros((len(ci), 2)), case.K4)
    uv = uv + np.random.default_rng(5).normal(0, 0.5, uv.shape)
    case.ci, case.pi = np.concatenate([case.ci, ci]), np.concatenate([case.pi, pi])
    case.uv = np.concatenate([case.uv, uv])
    return case


# name -> (case builder, environment, expected layout scalars)
SHAPES = {
    "segl16_nc17": (lambda m: (sc.pinhole_case if m == "pinhole" else sc.bal_case)(17, 900, 5, seed=21), {}, dict(cam_segl=16)),
    "segl16_nc33": (lambda m: (sc.pinhole_case if m == "pinhole" else sc.bal_case)(33, 1500, 5, seed=22), {}, dict(cam_segl=16)),
    "segl64_nc17": (lambda m: (sc.pinhole_case if m == "pinhole" else sc.bal_case)(17, 12000, 6, seed=23), {}, dict(cam_segl=64)),
    "one_obs_cams": (lambda m: _one_obs_cameras((sc.pinhole_case if m == "pinhole" else sc.bal_case)(33, 1500, 5, seed=24)), {},
                     dict(cam_segl=16)),
    "lanes2": (lambda m: (sc.pinhole_case if m == "pinhole" else sc.bal_case)(20, 3000, 4, seed=25), {"BA_PT_LANES": "2"}, dict(lanes=2)),
    "lanes4": (lambda m: (sc.pinhole_case if m == "pinhole" else sc.bal_case)(20, 3000, 4, seed=25), {"BA_PT_LANES": "4"}, dict(lanes=4)),
    "lanes8": (lambda m: (sc.pinhole_case if m == "pinhole" else sc.bal_case)(20, 3000, 4, seed=25), {"BA_PT_LANES": "8"}, dict(lanes=8)),
    "lanes16": (lambda m: (sc.pinhole_case if m == "pinhole" else sc.bal_case)(20, 3000, 4, seed=25), {"BA_PT_LANES": "16"}, dict(lanes=16)),
    "long_tracks": (lambda m: _long_tracks((sc.pinhole_case if m == "pinhole" else sc.bal_case)(20, 3000, 4, seed=26)),
                    {"BA_PT_LANES": "2"}, dict(lanes=2)),
    "multi_round": (lambda m: (sc.pinhole_case if m == "pinhole" else sc.bal_case)(20, 6000, 4, seed=27), {"BA_PT_BLOCKS": "3"},
                    dict(nblkP=3)),
    "window_not_in_lds": (lambda m: (sc.pinhole_case if m == "pinhole" else sc.bal_case)(1100 if m == "pinhole" else 760, 8000, 4, seed=28),
                          {"BA_PT_BLOCKS": "1"}, dict(nblkP=1)),
}


@pytest.mark.parametrize("precision", [0, 1], ids=["f64", "f32"])
@pytest.mark.parametrize("model", ["pinhole", "bal"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_layout_variants(solver, monkeypatch, shape, model, precision):
    build, env, want = SHAPES[shape]
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    case = build(model)
    run(solver, case, "huber", precision, 1, n_vec=2)
    st = solver.debug_layout("scalars")
    for k, val in want.items():
        assert st[k] == val, (k, st)
    if shape == "segl16_nc17":
        assert case.n_cams % (256 // 16) != 0
    if shape == "long_tracks":
        assert st["nblkL"] > 0, st
    if shape == "window_not_in_lds":
        assert st["all_lds_" + model] == 0, st
    if shape == "one_obs_cams":
        assert (np.bincount(case.ci, minlength=case.n_cams)[-2:] == [2, 1]).all()


@pytest.mark.parametrize("precision", [0, 1], ids=["f64", "f32"])
def test_config5_full_size(solver, precision):
    """BASELINE config 5 (1723 BAL cameras, ~662k observations), against the matrix-free reference."""
    from bundle_adjustment_amd.synthetic import make_bal_problem
    p = make_bal_problem()
    case = sc.Case(p.cams, p.pts, p.cam_idx, p.pt_idx, p.uv, None, 0)
    run(solver, case, "huber", precision, 1, n_vec=2)
    assert solver.debug_layout("scalars")["cam_segl"] == 16


@pytest.mark.parametrize("model", ["pinhole", "bal"])
def test_fp64_operator_is_symmetric(solver, model):
    """a.(S b) = b.(S a) to C u (|a| B(b) + |b| B(a))."""
    from oracle import ba_oracle as o
    case = _SMALL[model]().hold(np.random.default_rng(12))
    out, v, sysr = run(solver, case, "huber", 0, 1, n_vec=2, seed=4)
    a, b = v[0].copy(), v[1].copy()
    a[sysr.held] = 0.0
    b[sysr.held] = 0.0
    sa, sb = out["sv"][0], out["sv"][1]
    ba = sum(sysr.bound(b)); aa = sum(sysr.bound(a))
    lim = sc.C64 * o.U64 * (float((np.abs(a) * ba).sum()) + float((np.abs(b) * aa).sum()))
    assert abs(float((a * sb).sum()) - float((b * sa).sum())) <= lim


@pytest.mark.parametrize("model", ["pinhole", "bal"])
def test_kept_blocks_rhs_equals_fresh_build(solver, model):
    """precond 2 takes its right-hand side from the 6-sum camera pass: the same g as a fresh build, within the bound."""
    from oracle import ba_oracle as o
    case = _SMALL[model]().hold(np.random.default_rng(13))
    intr = case.upload(solver)
    kept = solver.schur_system(LAM, None, loss="cauchy", intr=intr, precond=2, lam_prev=0.1)
    fresh = solver.schur_system(LAM, None, loss="cauchy", intr=intr, precond=1)
    sysr, _ = case.reference("cauchy", LAM)
    assert np.all(np.abs(kept["g"] - fresh["g"]) <= 2 * sc.C64 * o.U64 * sysr.rhs_bound())
    assert not np.array_equal(kept["minv"], fresh["minv"])
