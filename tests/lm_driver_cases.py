"""The cases of tests/test_gpu_lm_driver.py, and what makes them fair: test_lm_trace_host.py checks on the CPU, with the
oracle alone, that each case has the PCG stop margin, exit margin, insensitivity to noise and coverage stated there.
Test infrastructure only.  A case: the problem, the solve's options under the device's names, and the mirror's run."""
import functools

import numpy as np

from bundle_adjustment_amd.bal import BALProblem
from bundle_adjustment_amd.synthetic import make_problem
from oracle import ba_oracle as o

# what every case sets (the multi-kernel path, no minimum PCG iteration count, the residual test alone ends an inner solve)
COMMON = dict(small_solver=1, pcg_min_iters=0, pcg_model_tol=0.0)
OFF = dict(ftol=0.0, xtol=0.0, gtol=0.0)
_ORACLE_NAME = dict(initial_lambda="lam0", preconditioner="precond")
_DEVICE_ONLY = ("small_solver", "pcg_min_iters", "loss")


@functools.lru_cache(maxsize=None)
def rejections_problem():
    return make_problem(16, 1000, 5, seed=1, rot_sigma=0.05, trans_sigma=0.3, point_sigma=0.5)


@functools.lru_cache(maxsize=None)
def capped_problem():
    return make_problem(17, 900, 5, seed=4, outlier_frac=0.02)


@functools.lru_cache(maxsize=None)
def bal_problem(far):
    """tests.test_bal._synthetic_bal(20, 600, 5, seed=8); far = (scale, seed): its start moved further away, by scale times
    the default perturbation (poses 1e-3, points 0.02).  The default start is never rejected before round-off decides.  On
    the grid scale 16, 32, 48, 64, 80, 96 x seed 100 .. 103 at initial_lambda 1e-6, most starts give one streak only, or
    inner solves of 40 and more PCG iterations, through which the 1e-13 noise of the sensitivity condition grows past 1e-2 of
    a tolerance; the smallest scale (then seed) that meets every condition of test_lm_trace_host.py is (64, 101) with
    fixed_cam = 0 (streaks of 4 and 3) and (80, 103) with fixed_cam = -1 (5 and 2)."""
    from tests.test_bal import _perturbed, _synthetic_bal
    p = _synthetic_bal(20, 600, 5, seed=8)
    return _perturbed(p, far[1], pose=1e-3 * far[0], pt=0.02 * far[0], focal=0.0) if far else p


REJ = dict(loss="linear", initial_lambda=1e-6, pcg_tol=1e-1, max_iters=12, **OFF)
CAP = dict(loss="huber", pcg_tol=1e-2, pcg_max_iters=2, max_iters=6, **OFF)
EXIT = dict(REJ, max_iters=40)
# held parameters of the xtol cases: one camera's translation, another one's rotation, and
#   exit_xtol_held         every 25th point: the mirror's trajectory keeps its rejections and leaves xtol late.  (With more
#                          held at this start -- whole cameras, every 7th point -- its steps halve from one iteration to the
#                          next, which leaves no threshold a factor two on either side.)  The held share is 2 % of |x|.
#   exit_xtol_mostly_held  all but every 16th point: the free entries are a quarter of |x| (100 of 393), so a driver that
#                          counts the held share leaves an iteration early, and one that subtracts it twice one late.  The
#                          problem is then nearly a resection and leaves xtol at once: the exit alone is what it is for.
HELD_CAM_BITS = {3: 0x38, 7: 0x07}
HELD_POINTS = dict(exit_xtol_held=lambda i: i % 25 == 0, exit_xtol_mostly_held=lambda i: i % 16 != 0)

# name -> (problem function, its argument or None, fixed_cam, options)
CASES = {
    "rejections": (rejections_problem, None, 0, REJ),
    "rejections_jacobi": (rejections_problem, None, 0, dict(REJ, preconditioner="jacobi")),
    "rejections_lag0": (rejections_problem, None, 0, dict(REJ, precond_lag=0)),
    "capped": (capped_problem, None, 0, CAP),
    "bal_rejections_fixed": (bal_problem, (64, 101), 0, REJ),
    "bal_rejections_free": (bal_problem, (80, 103), -1, REJ),
    "bal_capped_fixed": (bal_problem, False, 0, CAP),
    "bal_capped_free": (bal_problem, False, -1, CAP),
    # the exits, on the rejections problem; each threshold sits between the tested quantity's values at the mirror's exit
    # iteration (<= 1/2 of it) and at every earlier one (>= 2 x)
    "exit_ftol": (rejections_problem, None, 0, dict(EXIT, ftol=1e-4)),
    "exit_xtol": (rejections_problem, None, 0, dict(EXIT, xtol=5e-4)),
    "exit_gtol": (rejections_problem, None, 0, dict(EXIT, gtol=50.0)),
    "exit_gtol_at_once": (rejections_problem, None, 0, dict(EXIT, gtol=1e30)),
    "exit_max_iters": (rejections_problem, None, 0, dict(REJ, max_iters=6)),        # ends on the third rejection of a streak
    "exit_xtol_held": (rejections_problem, None, 0, dict(EXIT, xtol=2e-3)),
    "exit_xtol_mostly_held": (rejections_problem, None, 0, dict(EXIT, xtol=2e-2)),
}
REJECTION_CASES = ("rejections", "rejections_lag0", "bal_rejections_fixed", "bal_rejections_free")
CAPPED_CASES = ("capped", "bal_capped_fixed", "bal_capped_free")
EXIT_STATUS = dict(exit_ftol="ftol", exit_xtol="xtol", exit_gtol="gtol", exit_gtol_at_once="gtol", exit_max_iters="max_iters",
                   exit_xtol_held="xtol", exit_xtol_mostly_held="xtol")
SHORT_CASES = dict(exit_gtol_at_once=0, exit_xtol_mostly_held=3)      # iterations of the cases that are about their exit alone


def problem(name):
    fn, arg, _, _ = CASES[name]
    return fn() if arg is None else fn(arg)


def fixed_cam(name):
    return CASES[name][2]


def options(name):
    """The solve's options as Solver.solve / solve_bal take them (fixed_cam apart)."""
    return dict(COMMON, **CASES[name][3])


def held(name):
    """(camera bit masks (Nc,) uint16, held points (Np,) bool) of a case with held parameters, else (None, None)."""
    if name not in HELD_POINTS:
        return None, None
    p = problem(name)
    cm = np.zeros(p.n_cams, dtype=np.uint16)
    for c, bits in HELD_CAM_BITS.items():
        cm[c] = bits
    return cm, HELD_POINTS[name](np.arange(p.n_pts))


def oracle_kwargs(name):
    kw = {_ORACLE_NAME.get(k, k): v for k, v in options(name).items() if k not in _DEVICE_ONLY}
    cm, pm = held(name)
    if cm is not None:
        nb = 9 if isinstance(problem(name), BALProblem) else 6
        kw.update(held_cam=((cm[:, None] >> np.arange(nb)[None]) & 1).astype(bool), held_pt=pm)
    return kw


@functools.lru_cache(maxsize=None)
def mirror(name, mutate=None, noise_seed=None):
    """oracle.lm_solve on the case.  noise_seed: every pixel perturbed by 1e-13 relative (the sensitivity condition).
    Cached: the result is shared, leave it unchanged."""
    p = problem(name)
    uv = p.uv if noise_seed is None else p.uv * (1.0 + 1e-13 * np.random.default_rng(noise_seed).normal(size=p.uv.shape))
    bal = isinstance(p, BALProblem)
    return o.lm_solve(p.cams, p.pts, p.cam_idx, p.pt_idx, uv, None if bal else p.K4, fixed_cam(name), options(name)["loss"],
                      model="bal" if bal else "pinhole", mutate=mutate, **oracle_kwargs(name))


def streaks(history):
    """Lengths of the runs of rejected steps that an accepted step follows."""
    out, run = [], 0
    for h in history:
        if h["rho"] > 0:
            if run:
                out.append(run)
            run = 0
        else:
            run += 1
    return out
