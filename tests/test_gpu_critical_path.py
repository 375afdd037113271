"""GPU: three places on the LM step's critical path that were reworked for latency only (csrc/ba_kernels.hpp) -- the
partition fold of k_pcg_setup (every partition's words requested in one round, unpredicated loads with the predicate
applied afterwards; its results written back in one round too), the camera-update riders (sums parked in LDS across camera_state, no scratch in the point-pass
launches) and the fused launch's early fetch of its window's slice of the iterate.  None of them may move a bit.

Setup fold: the reduced system (ba_schur_system, the hook of tests/test_gpu_schur_system.py) at camera counts that leave
the last vector workgroup partly empty -- the lanes past the end of a slice and the slices' last words are where an
unpredicated load can go wrong -- for the three block modes, against the oracle at tests/schur_cases.check_system's
bounds, and bit-identical when asked twice.

Fused hand-over and riders: BA_RIDERS=7 against launches of their own (BA_RIDERS=0), identical bits, at a window whose
slice of the iterate is shorter than one trip of the copy loop, at one that needs a second trip, and for the BAL camera."""
import numpy as np
import pytest

from bundle_adjustment_amd import hip_backend
from bundle_adjustment_amd.synthetic import make_problem
from tests import schur_cases as sc

pytestmark = pytest.mark.gpu
LAM, LAM_PREV = 1e-3, 1e-2
PT_THREADS = 1024                 # threads of a point-pass workgroup: the copy loop moves 4 * PT_THREADS doubles per trip


@pytest.fixture(scope="module")
def solver():
    s = hip_backend.Solver(0)
    yield s
    s.close()


# camera counts that are no multiple of the cameras per vector workgroup: pinhole 16, BAL camera 8
FOLD_CASES = {
    "pinhole17": lambda: sc.pinhole_case(17, 300, 5, seed=31),
    "pinhole33": lambda: sc.pinhole_case(33, 300, 5, seed=32),
    "bal9": lambda: sc.bal_case(9, 300, 4, seed=33),
    "bal17": lambda: sc.bal_case(17, 300, 4, seed=34),
}
_refs = {}


def _reference(name, case, lam):
    """The oracle's system of a case at a damping, computed once."""
    key = (name, lam)
    if key not in _refs:
        _refs[key] = case.reference("huber", lam)
    return _refs[key]


@pytest.mark.parametrize("precond", [1, 2, 0], ids=["schur_jacobi", "kept_blocks", "jacobi"])
@pytest.mark.parametrize("name", sorted(FOLD_CASES))
def test_setup_fold_matches_the_oracle_and_repeats_its_bits(solver, name, precond):
    case = FOLD_CASES[name]()
    vc = 16 if case.nb == 6 else 8
    assert case.n_cams % vc != 0 and case.n_cams > vc
    intr = case.upload(solver)
    v = np.random.default_rng(7).normal(size=(2, case.n_cams, case.nb))
    kw = dict(loss="huber", intr=intr, precond=precond, lam_prev=LAM_PREV if precond == 2 else None)
    first = solver.schur_system(LAM, v, **kw)
    second = solver.schur_system(LAM, v, **kw)
    sysr, w = _reference(name, case, LAM)
    prev = _reference(name, case, LAM_PREV)[0] if precond == 2 else None
    sc.check_system(case, first, sysr, w, v, 0, precond, prev)
    for k in ("g", "minv", "sv"):
        assert np.array_equal(first[k], second[k]), k


def _solve(p, monkeypatch, riders, bal, **kw):
    monkeypatch.setenv("BA_RIDERS", str(riders))
    with hip_backend.Solver(0) as s:
        if bal:
            intr = s.set_problem_bal(p, fixed_cam=0)
            out = s.solve_bal_resident(intr, **kw)
        else:
            intr = None
            s.set_problem(p)
            out = s.solve(**kw)
        cams, pts = s.get_params()
        lay = s.debug_layout("scalars")
        win = np.asarray(s.debug_layout("blk_win")).reshape(-1, 2)
        return dict(out=out, cams=cams, pts=pts, intr=intr, trace=s.trace(), kernels=s.profile(reset=True), lay=lay, win=win)


def _bal_problem():
    from tests.test_bal import _synthetic_bal
    return _synthetic_bal(40, 2000, 5, 41)


# name -> (problem, BAL camera, doubles per camera of the iterate)
HANDOVER = {
    "slice_shorter_than_a_trip": (lambda: make_problem(20, 400, 4, seed=42, outlier_frac=0.02), False, 6),
    "slice_needs_a_second_trip": (lambda: make_problem(700, 3000, 5, seed=43, outlier_frac=0.02), False, 6),
    "bal_camera": (_bal_problem, True, 9),
}


@pytest.mark.parametrize("name", list(HANDOVER))
def test_fused_handover_and_riders_give_the_bits_of_separate_launches(name, monkeypatch):
    build, bal, nb = HANDOVER[name]
    p = build()
    kw = dict(loss="huber", max_iters=6, ftol=0.0, xtol=0.0, gtol=0.0, small_solver=1, profile=1)
    ref = _solve(p, monkeypatch, 0, bal, **kw)
    got = _solve(p, monkeypatch, 7, bal, **kw)
    assert got["lay"]["all_lds_bal" if bal else "all_lds_pinhole"] == 1, got["lay"]
    slice_max = int(got["win"][:, 1].max()) * nb          # doubles of the iterate the widest window fetches
    if name == "slice_shorter_than_a_trip":
        assert slice_max < PT_THREADS, slice_max
    if name == "slice_needs_a_second_trip":
        assert slice_max > 4 * PT_THREADS, slice_max
    assert ref["kernels"].get("schur_pt_then_backsub", {}).get("launches", 0) == 0
    if not bal:
        fused = got["kernels"].get("schur_pt_then_backsub", {}).get("launches", 0)
        assert fused > 0, sorted(got["kernels"])
    a, b = got["out"], ref["out"]
    assert a["iterations"] == b["iterations"] > 0 and a["pcg_iterations"] == b["pcg_iterations"] > 0
    for k in ("initial_cost", "final_cost", "accepted"):
        assert a[k] == b[k], k
    assert np.array_equal(got["cams"], ref["cams"]) and np.array_equal(got["pts"], ref["pts"])
    if bal:
        assert np.array_equal(got["intr"], ref["intr"])
    assert len(got["trace"]) == len(ref["trace"])
    for x, y in zip(got["trace"], ref["trace"]):
        assert (x["cost_trial"], x["gain_ratio"], x["damping"], x["pcg_iterations"], x["accepted"]) == \
               (y["cost_trial"], y["gain_ratio"], y["damping"], y["pcg_iterations"], y["accepted"])
