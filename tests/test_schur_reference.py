"""CPU: the references the reduced-camera-system GPU tests (test_gpu_schur_system.py) are held to.  The held-parameter
operator of the oracle agrees with the dense reduced system at nb = 6 and 9; the float32 emulation of the fp32-Jacobian
PCG passes lies inside the fp32 bound on every test shape, and its emulated mutants (the point vector y rounded through
float16; w.x applied to both residual components) fall outside it."""
import numpy as np
import pytest

from oracle import ba_oracle as o
from tests import schur_cases as sc

SHAPES = [("pinhole", lambda: sc.pinhole_case(17, 900, 5, seed=3)), ("bal", lambda: sc.bal_case(17, 900, 5, seed=3)),
          ("pinhole_long", lambda: sc.pinhole_case(33, 2500, 4, seed=5)), ("bal_33", lambda: sc.bal_case(33, 1500, 5, seed=6))]


@pytest.mark.parametrize("model", ["pinhole", "bal"])
def test_held_operator_matches_the_dense_reduced_system(model):
    case = (sc.pinhole_case if model == "pinhole" else sc.bal_case)(12, 300, 4, seed=1).hold(np.random.default_rng(2))
    lam = 1e-3
    sysr, _ = case.reference("huber", lam)
    from tests.held_reference import Reduced
    red = Reduced(case.cams, case.pts, case.ci, case.pi, case.uv, case.K4, case.fixed, case.cam_mask, case.pt_held)
    S, rhs = red.schur(red.normal_equations(case.cams, case.pts, "huber"), lam)
    assert sysr.held.any() and sysr.held_pt.any() and (case.nb == 6 or sysr.held[:, 6:].any())
    v = np.random.default_rng(3).normal(size=(case.n_cams, case.nb))
    ref = S @ v.ravel()
    assert np.abs(sysr.apply(v).ravel() - ref).max() <= 1e-13 * np.abs(ref).max()
    assert np.abs(sysr.rhs().ravel() - rhs).max() <= 1e-13 * np.abs(rhs).max()
    nb = case.nb
    D = sysr.schur_jacobi_blocks()
    for c in range(case.n_cams):
        blk = S[nb * c:nb * c + nb, nb * c:nb * c + nb]
        assert np.abs(D[c] - blk).max() <= 1e-13 * np.abs(blk).max()
        assert np.array_equal(sysr.jacobi_blocks()[c][sysr.held[c]], np.eye(nb)[sysr.held[c]])


@pytest.mark.parametrize("loss", ["linear", "huber", "cauchy"])
@pytest.mark.parametrize("shape", [s[0] for s in SHAPES])
def test_float32_emulation_lies_inside_the_bound_and_mutants_outside(shape, loss):
    case = dict(SHAPES)[shape]().hold(np.random.default_rng(7))
    sysr, w = case.reference(loss, 1e-3)
    v = np.random.default_rng(8).normal(size=(case.n_cams, case.nb))
    ref = sysr.apply(v)
    b1, b2 = sysr.bound(v)
    lim = sc.C64 * o.U64 * (b1 + b2) + sc.C32 * o.U32 * sysr.bound(v, cond=False)[1]
    free = ~sysr.held

    def worst(x):
        return float((np.abs(x - ref)[free] / lim[free]).max())

    assert worst(case.emulate_f32(sysr, w, v)) <= 1.0 / 2          # twice inside the bound
    assert worst(case.emulate_f32(sysr, w, v, "y_f16")) > 2.0      # M3
    if loss != "linear":                                            # (linear: w = 1 in both components)
        assert worst(case.emulate_f32(sysr, w, v, "wx_both")) > 1e3  # M5
