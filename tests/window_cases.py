"""The cases of tests/test_gpu_window_held.py -- the two single-launch window kernels under held parameters, all five
losses and f_scale, step by step -- and their reference runs (tests/window_reference.window_lm).  Shared with
tests/test_window_reference_host.py, which checks on the CPU that each case is well enough conditioned for the GPU test's
tolerances, that none of its iterations is decided by round-off, and that the comparison fails for faulty kernels.
Test infrastructure only.  The reference runs are cached and shared: leave them unchanged."""
import functools

import numpy as np

from bundle_adjustment_amd.synthetic import make_problem
from tests import lm_trace
from tests import robust_losses as rl
from tests.window_reference import window_lm

OFF = dict(ftol=0.0, xtol=0.0, gtol=0.0)
# The project's own tolerances: lm_trace.TOL on damping (1e-6), gain ratio (1e-6) and step norm (1e-7); test_gpu_small.py's
# 1e-9 relative on cost and trial cost and 1e-7 max(1, |x|) on parameters.  Every case is held to them, the rejected
# steps included; test_window_reference_host.py shows what entitles each case to them: its first damped step solved two
# ways differs by 1 / 100 of them at most, its whole run driven two ways by 1 / 10.
TOL = dict(lm_trace.TOL, cost_trial=1e-9)
COST_TOL, PARAM_TOL = 1e-9, 1e-7

# name -> (cameras, points, observations per point, repeated (camera, point) pairs, observations shuffled); what each
# reaches (k_small_lm: tile rows of [V; z] = (6 Nc + 16) / 16; k_small_mw<NT>: workgroups = ceil(Np / 64)):
SHAPES = {
    "c2_p37": (2, 37, 2, 0, False),      # lm 1 tile row | mw<2>, 1 workgroup; one adjustable camera with a partial mask
    "c4_p65": (4, 65, 3, 0, False),      # lm 2 | mw<2>, 2 workgroups, the second one's only landmark held
    "c5_p129": (5, 129, 4, 0, False),    # lm 2 (30 + 1 rows) | mw<2>, 3 workgroups
    "c7_p200": (7, 200, 5, 0, False),    # lm 3 | mw<3>, 4 workgroups
    "c8_p130": (8, 130, 6, 0, False),    # lm 4, the z row alone in tile row 3 | mw<4>, 3 workgroups
    "c6_p520": (6, 520, 3, 0, True),     # lm 3, more points than threads, held points at indices >= 512 | mw<3>, 9 workgroups,
                                         # the last one held entirely; observations in shuffled order
    "c3_p130_dup": (3, 130, 3, 5, False),  # lm 2, repeated pairs add up inside V; never k_small_mw's case
}
LM_ONLY = ("c3_p130_dup",)


def start(shape, loss):
    """The start, in multiples of make_problem's default distance from the truth (0.005 rad, 0.02 m, points 0.05 m).  From
    the default one a linear case is at round-off in its fourth iteration: four times further out (the three-camera case:
    ten times) it gets there in iteration 5 to 8.  The robust losses start there as well, but for two kinds of case that
    are too ill-conditioned from so far for the tolerances above (test_window_reference_host.py measures it: the run
    driven by block elimination drifts from the one driven by the full system by up to 9e-8 in a step norm): arctan,
    whose weights 1 / (1 + z^2) are next to nothing for nearly every observation 4 x out, and the two-camera case, all
    two-view landmarks.  Those start at the default distance."""
    if loss == "linear":
        return 10.0 if shape == "c3_p130_dup" else 4.0
    return 1.0 if (loss == "arctan" or shape == "c2_p37") else 4.0


# (loss, f_scale): all five at f_scale 2, and huber once below 1
LOSSES = (("linear", 2.0), ("huber", 2.0), ("soft_l1", 2.0), ("cauchy", 2.0), ("arctan", 2.0), ("huber", 0.5))
STEP_CASES = [(shape, loss, f_scale) for shape in SHAPES for loss, f_scale in LOSSES]
# A robust case still lowers its cost by more than 1e-7 of it in iteration 8, a linear one by more than 1e-7 in iteration 4
# (test_window_reference_host.py asserts the margin to lm_trace.ROUND_OFF_STOP for every case)
ITERS = dict(linear=4, robust=8)

REJECTED_GPU_LOSSES = ("cauchy", "soft_l1")              # arctan accepts every step: the contrast, on the CPU only
REJECTED_LOSSES = REJECTED_GPU_LOSSES + ("arctan",)
# cauchy: the streak and two accepted steps.  (From its third accepted step on the landmarks behind the outliers leave for
# infinity -- steps of 2 km, 25 km, 100 km -- and the two ways of driving the run drift apart by 1e-4.)
REJECTED_ITERS = dict(cauchy=6, soft_l1=10, arctan=10)
REJECTED_LAMBDA = 1e-6

WHOLE, INTERIOR, TRANSLATION, ROTATION = 0x3F, 0b001100, 0b111000, 0b000111


def iters(loss):
    return ITERS["linear" if loss == "linear" else "robust"]


def _with(p, **kw):
    f = dict(cams=p.cams, pts=p.pts, cam_idx=p.cam_idx, pt_idx=p.pt_idx, uv=p.uv, K4=p.K4, fixed_cam=p.fixed_cam)
    f.update(kw)
    return type(p)(f["cams"], f["pts"], f["cam_idx"], f["pt_idx"], f["uv"], f["K4"], f["fixed_cam"])


def with_duplicates(p, n_dup, seed):
    """n_dup extra observations that repeat an existing (camera, point) pair with a slightly different pixel."""
    rng = np.random.default_rng(seed)
    pick = rng.choice(p.n_obs, n_dup, replace=False)
    return _with(p, cam_idx=np.concatenate([p.cam_idx, p.cam_idx[pick]]), pt_idx=np.concatenate([p.pt_idx, p.pt_idx[pick]]),
                 uv=np.concatenate([p.uv, p.uv[pick] + rng.normal(0, 0.5, (n_dup, 2))]))


def masks(n_cams, n_pts, fixed):
    """-> (camera bit masks (Nc,) uint16, held points (Np,) bool).  The last camera keeps its translation, the first two
    adjustable ones are held whole and in two interior parameters (rvec z, t x) -- with one or two adjustable cameras
    what fits, the interior mask first; every 13th point and the last 64-landmark group are held."""
    cm = np.zeros(n_cams, np.uint16)
    rest = [c for c in range(n_cams) if c != fixed]
    if len(rest) >= 2 and rest[-1] == n_cams - 1:
        cm[rest.pop()] = TRANSLATION
    if len(rest) >= 2:
        cm[rest[0]], cm[rest[1]] = WHOLE, INTERIOR
    else:
        cm[rest[0]] = INTERIOR
    pm = np.arange(n_pts) % 13 == 0
    if n_pts > 64:
        pm[64 * ((n_pts - 1) // 64):] = True
    return cm, pm


def _robust_pixels(p, loss, seed):
    """Non-linear losses: 5 % of the observations moved by 5 .. 40 px."""
    return p if loss == "linear" else _with(p, uv=rl.inject_outliers(p.uv, 0.05, seed, lo=5.0, hi=40.0)[0])


@functools.lru_cache(maxsize=None)
def step_problem(shape, loss):
    """The BAProblem of a step-by-step case: the fixed camera in the middle."""
    nc, npt, k, dups, shuffled = SHAPES[shape]
    far = start(shape, loss)
    p = make_problem(nc, npt, k, seed=100 + nc, rot_sigma=0.005 * far, trans_sigma=0.02 * far, point_sigma=0.05 * far)
    p = _robust_pixels(_with(p, fixed_cam=nc // 2), loss, seed=nc)
    if dups:
        p = with_duplicates(p, dups, seed=nc)
    if shuffled:
        order = np.random.default_rng(npt).permutation(p.n_obs)
        p = _with(p, cam_idx=p.cam_idx[order], pt_idx=p.pt_idx[order], uv=p.uv[order])
    return p.validate()


def step_masks(shape):
    nc, npt = SHAPES[shape][:2]
    return masks(nc, npt, nc // 2)


@functools.lru_cache(maxsize=None)
def step_reference(shape, loss, f_scale, mutate=None, max_iters=None):
    cm, pm = step_masks(shape)
    return window_lm(step_problem(shape, loss), cm, pm, loss=loss, f_scale=f_scale, max_iters=max_iters or iters(loss),
                     mutate=mutate, **OFF)


# ---------------------------------------------------------------- rejected steps
@functools.lru_cache(maxsize=None)
def rejected_problem(loss):
    """test_gpu_small.py's start far from the minimiser (camera 0 fixed), under masks and with outliers: cauchy rejects
    the first four steps, soft_l1 the first five, arctan none."""
    p = make_problem(5, 200, 4, seed=5, point_sigma=3.0, rot_sigma=0.2, trans_sigma=1.0)
    return _robust_pixels(p, loss, seed=5).validate()


def rejected_masks():
    return masks(5, 200, 0)


@functools.lru_cache(maxsize=None)
def rejected_reference(loss):
    cm, pm = rejected_masks()
    return window_lm(rejected_problem(loss), cm, pm, loss=loss, f_scale=2.0, max_iters=REJECTED_ITERS[loss], lam0=REJECTED_LAMBDA, **OFF)


# ---------------------------------------------------------------- exits
EXIT_LOSS, EXIT_ITERS = "huber", 12
# where the reference leaves: gtol after this many iterations (at the next linearisation), xtol / ftol in this iteration
GTOL_AFTER, XTOL_AT, FTOL_AT = 4, 6, 5
MARGIN = 1.1


@functools.lru_cache(maxsize=None)
def exit_problem():
    """6 cameras, 150 points: camera 2 held whole, camera 4's rotation; 70 % of the points held where N(0, 0.3 m) has
    pushed them, so the gradient of the held entries stays large while that of the free ones falls."""
    p = make_problem(6, 150, 4, seed=41, outlier_frac=0.03)
    rng = np.random.default_rng(41)
    pm = rng.random(p.n_pts) < 0.7
    pts = p.pts.copy()
    pts[pm] += rng.normal(0.0, 0.3, (int(pm.sum()), 3))
    cm = np.zeros(p.n_cams, np.uint16)
    cm[2], cm[4] = WHOLE, ROTATION
    return _with(p, pts=pts, fixed_cam=3).validate(), cm, pm


@functools.lru_cache(maxsize=None)
def exit_reference(which=None, mutate=None):
    """which None: all tolerances off (the history the thresholds come from); 'gtol' / 'xtol' / 'ftol': that one set."""
    p, cm, pm = exit_problem()
    tol = dict(OFF)
    if which is not None:
        tol[which] = exit_thresholds()[which]
    return window_lm(p, cm, pm, loss=EXIT_LOSS, f_scale=1.0, max_iters=EXIT_ITERS, mutate=mutate, **tol)


def _between(late, early, earlier):
    """The geometric mean of two adjacent iterations' values, MARGIN away from both and below everything earlier."""
    t = float(np.sqrt(late * early))
    assert late * MARGIN <= t and t * MARGIN <= early and all(t * MARGIN <= e for e in earlier), (late, early, earlier)
    return t


@functools.lru_cache(maxsize=None)
def exit_thresholds():
    """Each threshold from the reference's own history with every tolerance off, between the tested quantity's values at
    the exit iteration and at the one before."""
    h = exit_reference()["history"]
    assert all(r["rho"] > 0 for r in h[:max(GTOL_AFTER + 1, XTOL_AT, FTOL_AT)])         # every one a new linearisation
    g = [r["gmax"] for r in h]
    x = [r["step"] / r["xnorm"] for r in h]
    f = [(r["cost"] - r["cost_new"]) / r["cost_new"] for r in h]
    return dict(gtol=_between(g[GTOL_AFTER], g[GTOL_AFTER - 1], g[:GTOL_AFTER - 1]),
                xtol=_between(x[XTOL_AT - 1], x[XTOL_AT - 2], x[:XTOL_AT - 2]),
                ftol=_between(f[FTOL_AT - 1], f[FTOL_AT - 2], f[:FTOL_AT - 2]))


# ---------------------------------------------------------------- handle reuse
@functools.lru_cache(maxsize=None)
def reuse_problem():
    """97 points: V's padding to 16 columns is in play."""
    p = make_problem(5, 97, 4, seed=21, outlier_frac=0.03)
    return _with(p, fixed_cam=2).validate()


# ---------------------------------------------------------------- the comparison both test files make
def follow(summary, trace, ref, tol=None, exit_under_test=False):
    """(summary, trace) of a window kernel -- or of a mutant of the reference, through lm_trace.from_oracle -- against the
    reference run `ref`: lm_trace.check_follows, EVERY iteration of the reference compared (so the exit always is: status,
    iteration count, accepted steps, final damping), the cost carried into each iteration and the final cost.  Raises
    AssertionError; returns check_follows' largest deviations."""
    tol = TOL if tol is None else tol
    compared, dev = lm_trace.check_follows(summary, trace, ref, tol=tol, exit_under_test=exit_under_test)
    assert compared == ref["iterations"] == len(ref["history"]) == summary["iterations"] == len(trace), \
        (compared, ref["iterations"], summary["iterations"], len(trace))
    assert abs(summary["initial_cost"] - ref["cost0"]) <= COST_TOL * ref["cost0"], (summary["initial_cost"], ref["cost0"])
    for t, h in zip(trace, ref["history"]):
        assert abs(t["cost"] - h["cost"]) <= max(COST_TOL, tol["cost_trial"]) * h["cost"], (t, h)
    assert abs(summary["final_cost"] - ref["cost"]) <= max(COST_TOL, tol["cost_trial"]) * ref["cost"], (summary["final_cost"], ref["cost"])
    return dev


def params_agree(cams, pts, ref):
    """Largest parameter deviation from the reference over PARAM_TOL max(1, |x|): <= 1 passes."""
    return max(np.abs(cams - ref["cams"]).max() / max(1.0, np.abs(ref["cams"]).max()),
               np.abs(pts - ref["pts"]).max() / max(1.0, np.abs(ref["pts"]).max())) / PARAM_TOL
