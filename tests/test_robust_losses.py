"""CPU: the loss (and preconditioner) names the Python layer accepts, the C enums behind them, and the tests' numpy
statement of scipy's losses (tests/robust_losses.py) against scipy's own loss functions."""
import importlib
import os
import re

import numpy as np
import pytest

from tests import robust_losses as rl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = np.array([[718.856, 0.0, 607.1928], [0.0, 718.856, 185.2157], [0.0, 0.0, 1.0]])


def test_backend_accepts_scipy_loss_names():
    from bundle_adjustment_amd import hip_backend as hb
    assert set(hb.LOSS) == set(rl.LOSSES)
    assert [hb.loss_code(n) for n in rl.LOSSES] == [0, 1, 2, 3, 4]
    assert hb.loss_code(3) == 3                         # by value: passed through, the library validates it


@pytest.mark.parametrize("bad", ["bogus", "Huber", "l1", ""])
def test_backend_rejects_unknown_loss_names(bad):
    from bundle_adjustment_amd import hip_backend as hb
    with pytest.raises(ValueError, match="soft_l1"):
        hb.loss_code(bad)


def test_options_reject_unknown_loss_before_any_device_call():
    """Solver._options is what solve / solve_bal / bal.solve build their ba_options with: the name is checked there."""
    from bundle_adjustment_amd import hip_backend as hb

    class NoDevice(hb.Solver):
        def __init__(self):
            pass

        def default_options(self):
            return hb.BAOptions()

    s = NoDevice()
    assert s._options(dict(loss="cauchy")).loss == 3
    with pytest.raises(ValueError):
        s._options(dict(loss="tukey"))
    assert s._options(dict(preconditioner="jacobi")).preconditioner == 0
    assert s._options(dict(preconditioner=1)).preconditioner == 1        # by value: passed through, the library validates it
    for bad in ("two_level", "bogus"):                                    # two_level: retired (enum value 2)
        with pytest.raises(ValueError, match="'jacobi', 'schur_jacobi'"):
            s._options(dict(preconditioner=bad))


def test_bundle_adjuster_rejects_unknown_loss_at_construction():
    from bundle_adjustment_amd import BundleAdjuster
    with pytest.raises(ValueError, match="bogus"):
        BundleAdjuster(K, loss="bogus")
    for name in rl.LOSSES:
        assert BundleAdjuster(K, loss=name).solver_options["loss"] == name
    with pytest.raises(ValueError, match="two_level"):
        BundleAdjuster(K, preconditioner="two_level")


def test_header_enum_matches_backend_names():
    from bundle_adjustment_amd import hip_backend as hb
    hdr = open(os.path.join(ROOT, "include", "ba_hip.h")).read()
    body = re.search(r"enum ba_loss \{(.*?)\};", hdr, flags=re.S).group(1)
    enum = {k.lower(): int(v) for k, v in re.findall(r"BA_LOSS_([A-Z_0-9]+)\s*=\s*(\d+)", body)}
    assert enum == hb.LOSS
    body = re.search(r"enum ba_precond \{(.*?)\};", hdr, flags=re.S).group(1)
    enum = {k.lower(): int(v) for k, v in re.findall(r"BA_PRECOND_([A-Z_0-9]+)\s*=\s*(\d+)", body)}
    assert enum == hb.PRECOND


@pytest.mark.parametrize("loss", rl.LOSSES[1:])
def test_numpy_losses_match_scipy(loss):
    """rho and rho' against scipy's own loss callables over z from 1e-12 to 1e12, at rtol 1e-12.  The absolute slack of a
    few units in the last place of 1 covers scipy's naive soft_l1, 2 (sqrt(1 + z) - 1), which cancels at small z; the
    statement here does not (checked against the series 2 (z/2 - z^2/8 + z^3/16) below)."""
    L = importlib.import_module("scipy.optimize._lsq.least_squares")
    z = np.concatenate([np.logspace(-12, 12, 2001), [1e-4, 0.5, 1.0, 2.0]])
    ref = np.empty((3, z.size))
    L.IMPLEMENTED_LOSSES[loss](z, ref, cost_only=False)
    r0, r1 = rl.rho(z, loss)
    np.testing.assert_allclose(r0, ref[0], rtol=1e-12, atol=4e-16)
    np.testing.assert_allclose(r1, ref[1], rtol=1e-12, atol=0)
    big = z >= 1e-4
    np.testing.assert_allclose(r0[big], ref[0][big], rtol=1e-11 if loss == "soft_l1" else 1e-12)
    if loss == "soft_l1":
        small = z[z < 1e-6]
        np.testing.assert_allclose(rl.rho(small, loss)[0], small - small ** 2 / 4 + small ** 3 / 8, rtol=1e-14)


@pytest.mark.parametrize("loss", rl.LOSSES)
@pytest.mark.parametrize("f_scale", [0.7, 3.0])
def test_numpy_cost_and_weights_match_scipy_loss_function(loss, f_scale):
    """cost = 0.5 sum C^2 rho((f/C)^2) and w = rho'((f/C)^2), as scipy's construct_loss_function scales them."""
    L = importlib.import_module("scipy.optimize._lsq.least_squares")
    f = np.random.default_rng(1).normal(0.0, 5.0, 4000)
    fn = L.construct_loss_function(f.size, loss, f_scale)
    if fn is None:
        assert rl.cost(f, loss, f_scale) == pytest.approx(0.5 * float((f * f).sum()), rel=1e-13)
        assert np.all(rl.weights(f, loss, f_scale) == 1.0)
        return
    assert rl.cost(f, loss, f_scale) == pytest.approx(fn(f, cost_only=True), rel=1e-12)
    np.testing.assert_allclose(rl.weights(f, loss, f_scale), fn(f)[1], rtol=1e-12)


def test_outlier_injection_moves_the_chosen_observations_by_20_to_200_px():
    uv = np.zeros((1000, 2))
    out, mask = rl.inject_outliers(uv, 0.05, seed=0)
    d = np.hypot(*(out - uv).T)
    assert mask.sum() == 50 and np.all(d[~mask] == 0)
    assert d[mask].min() >= 20.0 and d[mask].max() <= 200.0
