"""GPU: shared intrinsics in BAL solves (ba_set_shared_intrinsics) -- cameras of a group adjust ONE f, k1, k2.  The
reference is tests/shared_reference.py: the dense normal equations E^T (J^T w J + L) E of the shared parametrisation."""
import numpy as np
import pytest

from bundle_adjustment_amd import bal, hip_backend
from bundle_adjustment_amd.problem import BAProblem
from bundle_adjustment_amd.synthetic import make_bal_problem, make_shared_bal_problem
from oracle import ba_oracle as o
from tests import robust_losses as rl
from tests import shared_reference as sr
from tests.held_reference import Reduced

pytestmark = pytest.mark.gpu
TIGHT = dict(ftol=0.0, xtol=0.0, gtol=0.0)
ONE_STEP = dict(max_iters=1, initial_lambda=1e-3, pcg_tol=1e-12, pcg_max_iters=5000, **TIGHT)
A = np.arange(0, 16, 2)             # interleaved: spans both k_pcg_step workgroups (8 cameras each)
B = np.array([1, 3, 5])
POSE = 0x3F


def _labels():
    lab = -np.ones(16, dtype=np.int32)
    lab[A], lab[B], lab[7] = 40, 3, 11          # arbitrary labels; 7 is a singleton
    return lab


def _pose_mask(n):
    m = np.zeros(n, dtype=np.uint16)
    m[0] = POSE                                  # camera 0's pose held: the gauge, without touching its (shared) intrinsics
    return m


@pytest.fixture(scope="module")
def std():
    """The standard input, built once: problem, labels, held mask."""
    b, lab = make_shared_bal_problem(_labels(), 16, 800, 3500, seed=0)
    return b, lab, _pose_mask(16)


@pytest.fixture(scope="module")
def std_outliers():
    b, lab = make_shared_bal_problem(_labels(), 16, 800, 3500, seed=0, outlier_frac=0.05)
    return b, lab, _pose_mask(16)


def _rel(a, b):
    return float(np.abs(a - b).max() / max(1e-300, np.abs(b).max()))


def _solve(b, labels, mask, priors=None, **kw):
    """(summary, cams (Nc, 9), pts, trace, stats) of solve_bal with the groups, mask and priors given."""
    with hip_backend.Solver(0) as s:
        out, cams, pts = s.solve_bal(b, held_cameras=mask, shared_intrinsics=labels, camera_priors=priors, **kw)
        return out, cams, pts, s.trace(), s.stats()


def _one_step(b, labels, mask, loss, f_scale, priors=None):
    """One LM iteration on the GPU against the dense step of the y problem: (error of the step, error of the gain ratio,
    |step_norm - |d||, |d|, PCG iterations)."""
    red = Reduced(b.cams, b.pts, b.cam_idx, b.pt_idx, b.uv, None, -1, mask)
    ref = sr.SharedProblem(red, -np.ones(b.n_cams, int) if labels is None else labels, priors)
    out, cams, pts, tr, _ = _solve(b, labels, mask, priors, loss=loss, f_scale=f_scale, **ONE_STEP)
    assert out["iterations"] == 1 and out["accepted"] == 1 and 0 < out["pcg_iterations"] < 5000
    st = ref.dense_step(b.cams, b.pts, 1e-3, loss, f_scale)
    d = st["step"]
    e = _rel(ref.step_of(b.cams, b.pts, cams, pts), d)
    g = abs(tr[0]["gain_ratio"] - st["gain"]) / abs(st["gain"])
    dn = float(np.linalg.norm(d))
    return e, g, abs(tr[0]["step_norm"] - dn), dn, out["pcg_iterations"]


def _check_one_step(b, labels, mask, loss, f_scale, what, priors=None):
    e0, g0, _, _, k0 = _one_step(b, None, mask, loss, f_scale, priors)
    e1, g1, sn, dn, k1 = _one_step(b, labels, mask, loss, f_scale, priors)
    print(f"{what}, {loss}: step error ungrouped {e0:.3e} grouped {e1:.3e}; gain-ratio error {g0:.3e} / {g1:.3e}; "
          f"|step_norm - |d|| {sn:.3e} of |d| {dn:.3e}; PCG iterations to 1e-12: {k0} / {k1}")
    assert e1 <= 10.0 * e0
    assert g1 <= max(10.0 * g0, 16.0 * 2.0 ** -53)
    assert sn <= 10.0 * max(e1, 1e-12) * dn


# ---------------------------------------------------------------- 1. one LM step against the dense y step
@pytest.mark.parametrize("loss,f_scale", [("linear", 1.0), ("huber", 2.0)])
def test_one_lm_step_matches_the_dense_y_step(std, loss, f_scale):
    """Tolerances: the same comparison with no groups on the same input (the behaviour before shared intrinsics) sets the
    scale; the grouped step may be ten times worse.  step_norm is the y problem's: a member counted twice misses by orders
    of magnitude.  Measured on an MI355X: DESIGN.md section 4g."""
    b, lab, mask = std
    _check_one_step(b, lab, mask, loss, f_scale, "16 cameras")


# ---------------------------------------------------------------- 2. a group larger than any workgroup
def test_one_lm_step_large_single_group():
    """300 cameras in ONE group: more members than the reducing workgroup has threads, 38 k_pcg_step workgroups."""
    b, lab = make_shared_bal_problem(True, 300, 700, 6000, seed=2)
    _check_one_step(b, lab, _pose_mask(300), "linear", 1.0, "300 cameras, one group")


# ---------------------------------------------------------------- 3. members stay bit-equal
def test_members_stay_bit_equal(std_outliers):
    b, lab, mask = std_outliers
    out, cams, pts, tr, st = _solve(b, lab, mask, loss="huber", max_iters=12, pcg_tol=1e-3, **TIGHT)
    assert st["shared_groups"] == 2 and out["iterations"] == 12 and out["accepted"] >= 3
    for m in (A, B):
        assert (cams[m, 6:].view(np.uint64) == cams[m[0], 6:].view(np.uint64)).all()
        assert not np.array_equal(cams[m[0], 6:], b.cams[m[0], 6:])
    free = np.setdiff1d(np.arange(16), np.concatenate([A, B]))
    assert np.unique(cams[free, 6]).size == free.size and not np.isin(cams[free, 6], cams[[A[0], B[0]], 6]).any()
    assert np.array_equal(cams[0, :6], b.cams[0, :6])
    cost = rl.cost(o.bal_residuals(cams, pts, b.cam_idx, b.pt_idx, b.uv).ravel(), "huber", 1.0)
    assert abs(out["final_cost"] - cost) <= 1e-12 * cost
    for r in tr:
        assert (r["cost_trial"] < r["cost"]) == r["accepted"]


# ---------------------------------------------------------------- 4. a minimiser of the y problem, linear loss
def test_solve_is_a_minimiser_of_the_shared_problem(std):
    b, lab, mask = std
    out, cams, pts, _, _ = _solve(b, lab, mask, loss="linear", max_iters=100, pcg_tol=1e-6, **TIGHT)
    assert out["final_cost"] < out["initial_cost"]
    ref = sr.SharedProblem(Reduced(b.cams, b.pts, b.cam_idx, b.pt_idx, b.uv, None, -1, mask), lab)
    report = []
    ref.certify(b.cams, b.pts, cams, pts, "linear", report=report)
    print(f"shared minimiser: gradient ratio {report[0][0]:.3e}, scipy restart drop {report[0][1]:.3e}, {out['iterations']} LM iterations")


# ---------------------------------------------------------------- 5. sharing acts
def test_sharing_acts_on_data_with_distinct_truth():
    b = make_bal_problem(16, 800, 3500, seed=0)
    lab, mask = _labels(), _pose_mask(16)
    start = bal._shared_start(b, sr.normalise(lab), "median")
    kw = dict(loss="linear", max_iters=30, pcg_tol=1e-4, **TIGHT)
    free = _solve(start, None, mask, **kw)
    grouped = _solve(start, lab, mask, **kw)
    assert grouped[0]["final_cost"] > free[0]["final_cost"]
    for m in (A, B):
        assert np.ptp(grouped[1][m, 6:], axis=0).max() == 0.0
        assert np.ptp(free[1][m, 6], axis=0) > 0.0


# ---------------------------------------------------------------- 6. no groups, no change
def test_no_groups_no_change(std_outliers):
    b, _, mask = std_outliers
    kw = dict(loss="huber", max_iters=8, pcg_tol=1e-3, **TIGHT)

    def run(prepare):
        with hip_backend.Solver(0) as s:
            intr = s.set_problem_bal(b)
            s.set_held(mask)
            if prepare is not None:
                prepare(s)
            groups = s.stats()["shared_groups"]
            out = s.solve_bal_resident(intr, **kw)
            cams, pts = s.get_params()
            tr = [{k: v for k, v in r.items() if k != "seconds"} for r in s.trace()]
            return {k: v for k, v in out.items() if not k.startswith("seconds")}, tr, cams, intr, pts, groups

    def set_then_clear(s):
        s.set_shared_intrinsics(_labels())
        assert s.stats()["shared_groups"] == 2
        s.set_shared_intrinsics(None)

    ref = run(None)
    assert ref[5] == 0 and ref[0]["accepted"] >= 2
    for prepare in (set_then_clear, lambda s: s.set_shared_intrinsics(-np.ones(16, np.int32)),
                    lambda s: s.set_shared_intrinsics(100 - np.arange(16, dtype=np.int32))):
        got = run(prepare)
        assert got[5] == 0
        assert got[0] == ref[0] and got[1] == ref[1]
        for x, y in zip(got[2:5], ref[2:5]):
            assert np.array_equal(x, y)


# ---------------------------------------------------------------- 7. held parameters and priors compose
def test_held_intrinsics_of_a_group(std):
    b, lab, mask = std
    m = mask.copy()
    m[A] |= 0x1C0
    out, cams, _, _, _ = _solve(b, lab, m, loss="linear", max_iters=6, pcg_tol=1e-4, **TIGHT)
    assert out["accepted"] >= 2
    assert np.array_equal(cams[A, 6:], b.cams[A, 6:])
    assert (cams[B, 6:] == cams[B[0], 6:]).all() and not np.array_equal(cams[B[0], 6:], b.cams[B[0], 6:])


def test_priors_on_members_add_up(std):
    """nb = 9 priors on two members of B (f only, means either side of the start): the group's prior is their sum."""
    b, lab, mask = std
    mean, info = np.zeros((16, 9)), np.zeros((16, 9, 9))
    for c, df in ((1, +8.0), (5, -4.0)):
        mean[c] = b.cams[c]
        mean[c, 6] += df
        info[c, 6, 6] = 1.0 / 0.5 ** 2
    _check_one_step(b, lab, mask, "linear", 1.0, "priors on two members of B", priors=(mean, info))
    out, cams, _, _, _ = _solve(b, lab, mask, (mean, info), loss="linear", max_iters=20, pcg_tol=1e-6, **TIGHT)
    free = _solve(b, lab, mask, None, loss="linear", max_iters=20, pcg_tol=1e-6, **TIGHT)
    target = 0.5 * (mean[1, 6] + mean[5, 6])
    assert abs(cams[1, 6] - target) < abs(free[1][1, 6] - target)


def test_precond_lag_keeps_blocks_across_grouped_systems(std_outliers):
    b, lab, mask = std_outliers
    out, cams, _, _, st = _solve(b, lab, mask, loss="huber", max_iters=15, pcg_tol=1e-3, precond_lag=3, **TIGHT)
    assert st["precond_reuses"] > 0 and st["precond_builds"] > 0
    assert out["final_cost"] < out["initial_cost"]
    for m in (A, B):
        assert (cams[m, 6:] == cams[m[0], 6:]).all()


# ---------------------------------------------------------------- 8. refusals
def test_refusals(std):
    b, lab, mask = std
    kw = dict(loss="linear", max_iters=2, pcg_tol=1e-3)

    def refused(call, *names):
        with pytest.raises(hip_backend.BAHipError) as e:
            call()
        msg = str(e.value)
        assert "error -1" in msg, msg                       # BA_ERR_INVALID
        for n in names:
            assert n in msg, msg

    with hip_backend.Solver(0) as s:
        intr0 = s.set_problem_bal(b)
        s.set_held(mask)
        s.set_shared_intrinsics(lab)
        assert s.stats()["shared_groups"] == 2
        # unequal member intrinsics
        intr = intr0.copy()
        intr[4, 1] = np.nextafter(intr[4, 1], 1.0)
        refused(lambda: s.solve_bal_resident(intr, **kw), "camera 4")
        # unequal held bits 6-8
        m = mask.copy()
        m[3] |= 0x40
        s.set_held(m)
        refused(lambda: s.solve_bal_resident(intr0.copy(), **kw), "camera 3")
        s.set_held(mask)
        # label -2
        bad = lab.copy()
        bad[9] = -2
        refused(lambda: s.set_shared_intrinsics(bad), "camera 9")
        assert s.stats()["shared_groups"] == 2               # a refused call leaves the groups alone
        # the pinhole solve, and the covariance
        refused(lambda: s.solve(**kw), "shared intrinsics")
        refused(lambda: s.covariance(intr=intr0), "ba_covariance", "shared intrinsics")
        # after clearing, the handle solves normally
        s.set_shared_intrinsics(None)
        s.set_params(b.cams[:, :6], b.pts)
        out = s.solve_bal_resident(intr0.copy(), **kw)
        assert out["accepted"] >= 1
    # fixed_cam inside a group
    with hip_backend.Solver(0) as s:
        intr0 = s.set_problem_bal(b, fixed_cam=2)
        s.set_shared_intrinsics(lab)
        refused(lambda: s.solve_bal_resident(intr0.copy(), **kw), "camera 2", "ba_set_held", "bits 0-5")
        # set_problem clears the groups
        s.set_problem_bal(b)
        assert s.stats()["shared_groups"] == 0


# ---------------------------------------------------------------- 9. Python surfaces
def test_bal_solve_surfaces():
    b = make_bal_problem(16, 800, 3500, seed=0)              # per-camera starts
    assert np.unique(b.cams[:, 6]).size == 16
    res, out = bal.solve(b, fixed_cam=0, shared_intrinsics=True, loss="linear", max_iters=10, pcg_tol=1e-4, **TIGHT)
    assert (res.cams[:, 6:].view(np.uint64) == res.cams[0, 6:].view(np.uint64)).all()
    assert out["final_cost"] < out["initial_cost"]
    assert np.array_equal(res.cams[0, :6], b.cams[0, :6])                     # fixed_cam: the pose stays, bit for bit
    assert not np.array_equal(res.cams[0, 6:], np.median(b.cams[:, 6:], axis=0))
    with pytest.raises(ValueError):
        bal.solve(b, fixed_cam=0, shared_intrinsics=True, shared_init="given", loss="linear", max_iters=2)
    with pytest.raises(ValueError):
        bal.covariance(b, fixed_cam=0, shared_intrinsics=[[0, 1]])
    # BAProblem(cam_group=) reaches the handle through set_problem
    p = BAProblem(np.ascontiguousarray(b.cams[:, :6]), b.pts, b.cam_idx, b.pt_idx, b.uv, np.array([1.0, 1.0, 0.0, 0.0]), -1,
                  cam_group=[[0, 1, 2], [5, 9]])
    with hip_backend.Solver(0) as s:
        s.set_problem(p)
        assert s.stats()["shared_groups"] == 2
