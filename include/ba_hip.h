/*
 * ba_hip.h -- C ABI of libba_hip.so, the MI355X (gfx950) bundle-adjustment solve step.
 *
 * This is the boundary a maintainer of egirgin/bundle_adjustment binds (ctypes; see
 * INTEGRATION.md) to replace the solve step of src/bundle_adjuster.py.  Each entry point
 * names the reference interface it stands in for (paths relative to the reference root).
 *
 * Conventions: every function returns 0 on success and a negative ba_status on failure;
 * ba_last_error() then holds a message for the calling thread.  All pointers are host
 * pointers owned by the caller unless a function says "device"; the library copies in
 * and out.  One handle = one GPU = one host thread at a time.  No callbacks, no global
 * state besides the per-thread error string.
 *
 * Flat problem layout (what BundleAdjuster.run packs at src/bundle_adjuster.py:157-162,
 * plus the fixed keyframe as an ordinary camera whose index is `fixed_cam`):
 *   cams  double[Nc][6]   rvec(3) | tvec(3), world->camera (Xc = R(rvec) X + t)
 *   pts   double[Np][3]
 *   obs   cam_idx int32[Nobs], pt_idx int32[Nobs], uv double[Nobs][2]
 *         row 2i, 2i+1 of the residual vector <-> observation i (src/bundle_adjuster.py:52-70)
 *   K4    double[4]       fx, fy, cx, cy (the only entries of camera_matrix that
 *                          cv2.projectPoints reads, src/bundle_adjuster.py:67)
 */
#ifndef BA_HIP_H
#define BA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ba_handle ba_handle;

enum ba_status {
  BA_OK = 0,
  BA_ERR_INVALID = -1,   /* bad argument / shape / index out of range */
  BA_ERR_HIP = -2,       /* a HIP runtime call failed */
  BA_ERR_STATE = -3,     /* call order (e.g. solve before set_problem) */
  BA_ERR_NUMERIC = -4,   /* non-finite residuals or cost */
  BA_ERR_COMM = -5,      /* RCCL load / init / collective failure */
  BA_ERR_INTERNAL = -6   /* a safety net of the library's own was hit (ba_build_tracks: the round cap) */
};

/* scipy least_squares' losses, rho(z) of z = (f / f_scale)^2 per scalar residual f; cost = 0.5 sum f_scale^2 rho(z):
 * linear z, huber z <= 1 ? z : 2 sqrt(z) - 1, soft_l1 2 (sqrt(1 + z) - 1), cauchy log(1 + z), arctan atan(z). */
enum ba_loss { BA_LOSS_LINEAR = 0, BA_LOSS_HUBER = 1, BA_LOSS_SOFT_L1 = 2, BA_LOSS_CAUCHY = 3, BA_LOSS_ARCTAN = 4 };
/* JACOBI: blocks of Hcc + lambda D.  SCHUR_JACOBI (default): the diagonal blocks of the reduced camera matrix S.
 * Any other value is refused by ba_solve and ba_solve_bal (BA_ERR_INVALID). */
enum ba_precond { BA_PRECOND_JACOBI = 0, BA_PRECOND_SCHUR_JACOBI = 1 /* 2: retired (BA_PRECOND_TWO_LEVEL) */ };

/* Solver knobs.  The reference's literals at src/bundle_adjuster.py:170-174 are
 * loss='huber' (f_scale 1), xtol = ftol = 1e-5, max_nfev = 50. */
typedef struct ba_options {
  int32_t loss;            /* ba_loss */
  int32_t max_iters;       /* LM iterations (accepted + rejected) */
  double f_scale;          /* the loss's soft threshold in pixels (scipy f_scale) */
  double ftol;             /* stop when cost decrease <= ftol * cost (on an accepted step) */
  double xtol;             /* stop when |step| <= xtol * (xtol + |x|) */
  double gtol;             /* stop when max |gradient| <= gtol */
  double initial_lambda;   /* Marquardt damping at the first iteration */
  double pcg_tol;          /* PCG stops at sqrt(rz / rz0) <= pcg_tol */
  int32_t pcg_max_iters;
  int32_t pcg_min_iters;
  int32_t preconditioner;  /* ba_precond */
  int32_t jacobian_precision; /* 0 = f64 (default); 1 = f32 Jacobian blocks in the PCG passes, f64 accumulation / solve */
  int32_t reserved0;       /* must be 0 */
  int32_t profile;         /* 1 = bracket every kernel with HIP events (see ba_get_profile) */
  int32_t verbose;
  int32_t small_solver;    /* 0 = problems of at most 8 cameras and 6144 observations on one rank (the reference's sliding
                              window, src/pipeline.py:39 window_size 5) are solved by the single-launch window solver
                              (csrc/ba_small.hpp: whole LM loop in one kernel, reduced system formed by fp64 MFMA and
                              factorised exactly); 1 = always the multi-kernel LM / Schur / PCG path.  A problem with priors
                              (ba_set_priors) always takes the multi-kernel path: the window kernels do not know them */
  double pcg_model_tol;    /* second PCG stopping test, on the quadratic model q(x) = 1/2 x^T S x - g^T x the iteration
                              minimises: stop after iteration i >= pcg_model_min_iters when i (q_{i-1} - q_i) <= pcg_model_tol |q_i|
                              (Nash & Sofer's truncated-Newton test; 0.5 is their value; 0 = off).  On ill-conditioned
                              reduced systems (long camera chains at small damping) the residual test of pcg_tol keeps
                              iterating long after the step has stopped improving the model: BASELINE config 5 on the
                              BAL camera at the reference's tolerances 1148 -> 557 PCG iterations, 39 -> 20 ms; on the
                              well-conditioned C3 it truncates useful iterations (a run to convergence needs 54 LM
                              iterations instead of 22), and on a chain driven to ftol = 1e-8 the truncated steps
                              stall the outer iteration.  Hence the default -1 = AUTOMATIC: 0.5 when ba_set_problem found
                              the problem band-structured (mean camera span of a track <= Nc / 8: sequential captures;
                              BA_STAT_BANDED; the statistic is summed over the landmark shards of a multi-rank job, so
                              every rank decides what a single rank would) AND the outer tolerance is loose (ftol >= 1e-6,
                              e.g. the reference's 1e-5); off otherwise. */
  int32_t pcg_model_min_iters; /* default 5 */
  int32_t precond_lag;     /* Schur-Jacobi only: how many consecutive damped systems may KEEP the preconditioner blocks
                              (M^-1 = blockdiag(S)^-1) built for an earlier one instead of rebuilding them (a preconditioner
                              need not be current: PCG solves the same system, only its iteration count can change).  A
                              kept system gets its right-hand side from the 6-sum camera pass instead of the 27-sum
                              one and skips the per-camera inversions.  The blocks are rebuilt anyway when the damping
                              has moved by more than 10x since they were built, when the last inner solve needed more
                              than 1.5x + 2 the iterations of the first solve after the build, or when the last accepted
                              step lowered the cost by more than 1 % (early, large steps: there a stale preconditioner
                              costs more PCG iterations than the pass it saves; measured at C3).  0 = rebuild for every
                              damped system.  Default 3 (ba_default_options).  Counted in BA_STAT_PRECOND_BUILDS / _REUSES. */
} ba_options;

typedef struct ba_summary {
  int32_t iterations;      /* LM iterations done */
  int32_t accepted;
  int32_t pcg_iterations;  /* total over all LM iterations */
  int32_t status;          /* 0 max_iters, 1 ftol, 2 xtol, 3 gtol, <0 ba_status */
  double initial_sse;      /* sum r^2 at entry == the reference's "Initial Cost" (:165) */
  double final_sse;        /* sum r^2 at exit  == "Final Cost" (:176) */
  double initial_cost;     /* 0.5 * sum rho(r^2) */
  double final_cost;
  double final_lambda;
  double seconds_total;    /* wall time of the solve loop */
  double seconds_linearize;
  double seconds_pcg;
  double seconds_update;
} ba_summary;

/* One record per LM iteration of the last ba_solve ("metrics / logging": the reference only
 * prints one line per run, src/bundle_adjuster.py:183-184; benchmarks and the drop-in's JSON metrics sink want the
 * trajectory).  Kept on the host, costs nothing on the device. */
typedef struct ba_iter_record {
  int32_t iteration;       /* 1-based */
  int32_t accepted;        /* 1 = step taken */
  int32_t pcg_iterations;  /* of this LM iteration */
  int32_t reserved;
  double cost;             /* 0.5 sum rho(r^2) before the step */
  double cost_trial;       /* ... at the trial point */
  double sse_trial;        /* sum r^2 at the trial point */
  double lambda;           /* damping the step was computed with */
  double gain_ratio;       /* actual / predicted decrease */
  double step_norm;        /* |dx| */
  double seconds;          /* wall time of this iteration on the host clock */
} ba_iter_record;

/* Per-kernel event timing collected when ba_options.profile = 1. */
#define BA_PROFILE_SLOTS 16
typedef struct ba_profile {
  int32_t launches[BA_PROFILE_SLOTS];          /* every launch */
  double total_ms[BA_PROFILE_SLOTS];
  int32_t working_launches[BA_PROFILE_SLOTS];  /* launches that did their work: PCG kernels exit at once */
  double working_ms[BA_PROFILE_SLOTS];         /* after convergence; those (< half the slot's longest) are left out */
} ba_profile;
/* slot ids */
enum ba_kernel_slot {
  BA_K_CAM_PREPARE = 0, BA_K_RESIDUAL = 1, BA_K_LINEARIZE_CAM = 2, BA_K_LINEARIZE_PT = 3,
  BA_K_POINT_INVERT = 4, BA_K_SCHUR_PT = 5, BA_K_SCHUR_CAM = 6, BA_K_PCG_UPDATE = 7,
  BA_K_PRECOND = 8, BA_K_BACKSUB = 9, BA_K_MISC = 10, BA_K_ALLREDUCE = 11,
  BA_K_SCHUR_PT_BACKSUB = 12,  /* launches of the PCG point pass that found PCG finished and went on as the back substitution */
  BA_K_TRACKS = 13,            /* ba_time_kernel only: the kernels of the last ba_triangulate_tracks call, with its options */
  BA_K_RESECT = 14,            /* ba_time_kernel only: the kernel of the last ba_resect call, with its options and masks */
  BA_K_RESECT_RANSAC = 15      /* ba_time_kernel only: the three kernels of the last ba_resect_ransac call, likewise */
};

/* Event counters of a handle (ba_get_stat): which implementation served the window-sized solves, how often the
 * multi-workgroup window solver had to be replaced by the one-workgroup kernel (its workgroups were not resident together:
 * csrc/ba_small_mw.hpp), how often the multi-kernel loop built / kept the Schur-Jacobi preconditioner. */
enum ba_stat {
  BA_STAT_WINDOW_MW_LAUNCHES = 0,   /* launches of k_small_mw (several cooperating workgroups) */
  BA_STAT_WINDOW_LM_LAUNCHES = 1,   /* launches of k_small_lm (one workgroup) */
  BA_STAT_WINDOW_FALLBACKS = 2,     /* k_small_mw gave up at a barrier and the window was re-solved by k_small_lm */
  BA_STAT_PRECOND_BUILDS = 3,       /* damped systems whose Schur-Jacobi blocks were rebuilt */
  BA_STAT_PRECOND_REUSES = 4,       /* damped systems that kept the previous blocks (ba_options.precond_lag) */
  BA_STAT_BANDED = 5,               /* 1: ba_set_problem found the current problem band-structured (pcg_model_tol's automatic default) */
  BA_STAT_CAP_FLOOR_RAISES = 6,     /* LM iterations whose inner solve ran into pcg_max_iters and raised the damping floor */
  BA_STAT_IPC_EXCHANGES = 7,        /* PCG iterations whose reduced-system product was exchanged through IPC-mapped peer buffers (BA_IPC=1) */
  BA_STAT_PIXELS_F32 = 8,           /* 1: every pixel of the current problem is a float32 value (as cv2 keypoints are) and the
                                       multi-kernel path keeps its two pixel streams as float2, widened on load: same results,
                                       8 bytes per observation and pass less (BA_PIXELS=f64 switches it off) */
  BA_STAT_HELD_PARAMS = 9,          /* held scalar parameters of the current problem (ba_set_held), fixed_cam's whole block included
                                       (6 parameters, or 9 once a camera mask sets a BAL bit); 3 per held point */
  BA_STAT_COUNT = 10,               /* statistics 0 - 9: the set callers of earlier releases size their arrays by */
  BA_STAT_PRIOR_BLOCKS = 10,        /* cameras + points of the calling rank that carry a non-zero prior block (ba_set_priors) */
  BA_STAT_SHARED_GROUPS = 11,       /* groups of two or more cameras that share their intrinsics (ba_set_shared_intrinsics) */
  BA_STAT_SCRATCH_BYTES = 12,       /* device memory of the calls that need no problem (two-view RANSAC, matching, ORB, pose graph, place
                                       recognition, track building), now: it follows the largest call so far, not their sum */
  BA_STAT_SCRATCH_ALLOCS = 13,      /* device allocations the scratch arena has made since ba_create; constant once calls repeat */
  BA_STAT_END = 14                  /* one past the last statistic ba_get_stat answers */
};

const char* ba_last_error(void);
const char* ba_kernel_name(int slot);
/* *value = counter `which` (ba_stat) of the handle since ba_create. */
int ba_get_stat(ba_handle* h, int32_t which, int64_t* value);
/* Test hook: occupies compute units from a SECOND stream of the handle -- n_workgroups workgroups of 256 threads with
 * lds_bytes of LDS each idle for `milliseconds` (at most 2000) of the device's wall clock, then leave.  Returns at once.
 * Lets a test hold the units the window solver's workgroups would need (tests/test_gpu_small.py). */
int ba_debug_occupy(ba_handle* h, int32_t n_workgroups, int32_t lds_bytes, double milliseconds);
/* Test hook: drains the stream and sets every byte of the scratch arena to `byte` (its low 8 bits).  The calls that use the
 * arena promise to read nothing they did not upload, clear or compute themselves; a test fills the arena with 0xff and with
 * 0x00 and expects the same results. */
int ba_debug_scratch_fill(ba_handle* h, int32_t byte);
/* Test hook: one array of the layout ba_set_problem built (the two observation orderings, their offsets, windows, grid
 * scalars), copied to out; `which` as listed in csrc/ba_hip.hip.  Lets a test compare the device build of large problems
 * (csrc/ba_setup.hpp) with the host build (BA_SETUP=host) element by element. */
int ba_debug_layout(ba_handle* h, int32_t which, void* out, int64_t capacity, int64_t* n);
/* Batched two-view triangulation + cheirality test: replaces VisualOdometryPipeline._triangulate_points,
 * src/pipeline.py:315-336 (cv2.triangulatePoints on P1 = K [I|0], P2 = K [R_rel|t_rel], division by (w + 1e-6),
 * z > 0 in both cameras).  K, R_rel row-major 3x3; pts1 / pts2 double[n][2] pixels in the two views; xyz double[n][3]
 * in the first camera's frame (EVERY point, kept or not); valid uint8[n] = the cheirality mask of :328-334.
 * Needs no ba_set_problem. */
int ba_triangulate(ba_handle* h, const double K[9], const double R_rel[9], const double t_rel[3], int64_t n,
                   const double* pts1, const double* pts2, double* xyz, uint8_t* valid);
/* N-view triangulation and filtering of whole tracks: the step between two adjustments of an SfM / SLAM loop (adjust ->
 * re-triangulate -> filter by angle, depth and reprojection error -> adjust; COLMAP's Retriangulate / FilterPoints3D, the point
 * culling of OpenMVG and ORB-SLAM; no reference counterpart: src/pipeline.py only triangulates pairs, see ba_triangulate).
 * Every point is triangulated from ALL of its observations and the handle's CURRENT cameras, which are treated as known:
 * held masks, fixed_cam, priors and shared-intrinsics groups play no part, and the handle's points are not read.
 *   intr   NULL: the pinhole with the handle's K4; else (f, k1, k2)[Nc] of the BAL camera, as in ba_residuals_bal
 *   xyz double[Np][3], status uint8[Np] (ba_track_status), angle_deg, rms_px, max_px double[Np]: the caller's point order;
 *   any may be NULL
 * Per point: (1) bearings -- pinhole ((u - cx) / fx, (v - cy) / fy, 1); BAL: the radial model inverted by Newton (r_d = |uv| / f,
 * r (1 + k1 r^2 + k2 r^4) = r_d from r = r_d; at most 25 steps to |dr| <= 1e-15 r; no convergence or a derivative <= 0 on the
 * way makes the track DEGENERATE), ray (p0, p1, -1).  (2) The homogeneous N-view DLT on the rows x (R2 X + t2) - (R0 X + t0),
 * y (R2 X + t2) - (R1 X + t1), centred on the mean camera centre of the track's observations, through the ten fp64 sums of
 * A^T A and a 4 x 4 Jacobi eigen-solve, w >= 0; |w| <= 1e-12 |X_h| or a non-finite entry: DEGENERATE.  (3) At most refine_iters
 * Marquardt-damped Gauss-Newton steps on the track's own cost 0.5 sum f_scale^2 rho((r / f_scale)^2) (IRLS with the weights
 * the solve uses; damping from 1e-4, / 10 after a step that does not raise the cost, * 10 after one that does, which is
 * dropped but counted; "does not raise" is cost_trial <= cost (1 + 1e-12), the rounding of the two sums; stop at
 * |dx| <= 1e-14 |X|); a 3 x 3 matrix that is not positive definite: DEGENERATE.  (4) At the final
 * point: angle_deg, the largest angle over all pairs of views between the unit vectors from the point to the two camera
 * centres (COLMAP's triangulation angle); rms_px = sqrt(sum |r_i|^2 / n_obs); max_px = the largest |r_i|.  (5) status = the first
 * failing test in enum order: FEW_VIEWS fewer than two DISTINCT cameras (no observation, one, or several by one camera: xyz and
 * the measures are NaN); DEGENERATE as above (found in (1) or (2): xyz and the measures are NaN; in (3): the last accepted point
 * and its measures); BEHIND a view with depth <= min_depth; LOW_ANGLE angle_deg < min_angle_deg; HIGH_ERROR max_px >
 * max_reproj_px.  For BEHIND, LOW_ANGLE, HIGH_ERROR and OK xyz and the measures are written.
 * write_points = 1 stores xyz of the OK points that are NOT held (ba_set_held) into the handle's current points, as if
 * ba_set_params had been called with the current cameras and the merged points (the linearisation is forgotten; masks,
 * priors, groups stay); write_points = 0 leaves the handle exactly as found.
 * BA_ERR_STATE before ba_set_problem / ba_set_params; BA_ERR_INVALID for an unknown loss, f_scale <= 0, refine_iters < 0,
 * reserved0 != 0.  Multi-rank jobs: the call is local to the calling rank's shard (its points, all cameras), no collective;
 * points are rank-local, so write_points = 1 is a rank-local write that every rank may make.  Pinned on two ranks
 * (tests/test_gpu_multirank_local.py): a handle with a communicator returns the bits of a plain handle on the same shard. */
enum ba_track_status { BA_TRACK_OK = 0, BA_TRACK_FEW_VIEWS = 1, BA_TRACK_DEGENERATE = 2,
                       BA_TRACK_BEHIND = 3, BA_TRACK_LOW_ANGLE = 4, BA_TRACK_HIGH_ERROR = 5 };
typedef struct ba_track_options {
  int32_t loss;            /* ba_loss of the refinement */
  int32_t refine_iters;    /* most damped Gauss-Newton steps; 0 = the linear solution only */
  double f_scale;
  double min_angle_deg;    /* <= 0: no test */
  double max_reproj_px;    /* <= 0: no test; compared with the track's LARGEST per-observation error */
  double min_depth;        /* a view fails when depth <= min_depth */
  int32_t write_points;
  int32_t reserved0;       /* must be 0 */
} ba_track_options;
int ba_default_track_options(ba_track_options* opts);   /* linear, 20, 1.0, 0, 0, 0.0, 0 */
int ba_triangulate_tracks(ba_handle* h, const double* intr, const ba_track_options* opts, double* xyz, uint8_t* status,
                          double* angle_deg, double* rms_px, double* max_px);
/* Resection: the pose of every selected camera from the points it sees, the mirror image of ba_triangulate_tracks (COLMAP's
 * image registration, OpenMVG's resection, the tracking / relocalisation pose of ORB-SLAM; no reference counterpart).  The
 * points are the handle's CURRENT points and are treated as known: held masks, fixed_cam, priors and shared-intrinsics groups
 * play no part in the estimate.  No RANSAC and no minimal solver: a linear start on all observations, then a robust refinement.
 * (ba_resect_ransac below is the call for raw matches: minimal samples, consensus, then this refinement on the consensus set.)
 *   intr      NULL: the pinhole with the handle's K4; else (f, k1, k2)[Nc] of the BAL camera, as in ba_triangulate_tracks;
 *             read, never changed
 *   cam_sel   uint8[Nc] or NULL = every camera: which cameras to resect.  A camera that is not selected gets its current
 *             pose in poses, status OK, n_inliers 0 and NaN measures.
 *   pt_known  uint8[Np] in the caller's point order, or NULL = every point: which points count as known
 *   poses double[Nc][6] (rvec | t), status uint8[Nc] (ba_resect_status), n_inliers int32[Nc], rms_px, max_px double[Nc]; any
 *   may be NULL
 * Per selected camera, over its n observations of known points: (1) bearings as in ba_triangulate_tracks (the BAL radial
 * model inverted by Newton); an observation whose bearing fails is dropped from n and is never an inlier.  (2) The start:
 * INIT_CURRENT the handle's pose (n >= 3), INIT_DLT (n >= 6) the DLT on the rows x (p3.X~) - p1.X~ = 0, y (p3.X~) - p2.X~ = 0
 * with X~ = ((X - mean) / sigma, 1), sigma^2 = mean |X - mean|^2 / 3 (Hartley normalisation, from centred values).  The 12 x 12
 * matrix is not formed: with S = sum X~X~^T, Sx = sum x X~X~^T, Sy = sum y X~X~^T, Sq = sum (x^2 + y^2) X~X~^T (forty fp64
 * sums), eliminating p1, p2 leaves M = Sq - Sx S^-1 Sx - Sy S^-1 Sy (4 x 4); p3 is its eigenvector of the smallest eigenvalue
 * (cyclic Jacobi), p1 = S^-1 Sx p3, p2 = S^-1 Sy p3.  S is factorised by a Cholesky of S / n: a pivot <= 1e-8 (coplanar,
 * collinear or coincident points) or a non-finite entry is DEGENERATE.  With A the left 3 x 3 of [p1; p2; p3] and b its last
 * column: P changes sign if det A < 0; R = U V^T of A's SVD; t = b / mean(singular values), then t <- sigma t - R mean;
 * sigma_3 <= 1e-6 sigma_1 is DEGENERATE; rvec is the quaternion log map of R (as in ba_transform).  Below the counts above the
 * status is FEW_POINTS.  For FEW_POINTS and a DEGENERATE start the pose is the current one, n_inliers 0 and the measures NaN.
 * (3) At most refine_iters Marquardt-damped Gauss-Newton steps on 0.5 sum f_scale^2 rho((r / f_scale)^2) over the six pose
 * parameters in the additive coordinates rvec | t, with the analytic Jacobian and IRLS weights of the solve: (H + lambda diag H)
 * dx = -g by a 6 x 6 Cholesky (a pivot <= 0: DEGENERATE with the last accepted pose and its measures); lambda from 1e-4, / 10
 * (floor 1e-12) after a step that does not raise the cost (cost_trial <= cost (1 + 1e-12)), * 10 after one that does, which is
 * dropped but counted; stop at |dx| <= 1e-14 |x|.  An observation behind the camera at a pass's pose is left out of that pass's
 * sums.  (4) At the final pose: inliers are the observations in front with |r_i| <= max_reproj_px; rms_px and max_px are taken
 * over the inliers, or over all observations in front when there are none.  (5) status = the first failing test in enum order:
 * FEW_POINTS, DEGENERATE as above; BEHIND more than half of the n observations are behind; FEW_INLIERS n_inliers <
 * min_inliers; HIGH_ERROR rms_px > max_rms_px.
 * write_cams = 1 stores the pose of every camera that is selected, OK, not fixed_cam and has none of the held bits 0-5 set
 * (ba_set_held), and leaves the handle exactly as ba_set_params(merged cameras, current points) would (the linearisation is
 * forgotten; masks, groups stay); write_cams = 0 leaves the handle exactly as found.
 * BA_ERR_STATE before ba_set_problem / ba_set_params, and (naming "priors") with write_cams = 1 while ba_set_priors blocks are
 * set: their means were set for the old poses.  BA_ERR_INVALID for an unknown loss or init, f_scale <= 0, refine_iters < 0,
 * min_inliers < 0, reserved0 != 0.  One workgroup per camera, sums in a fixed order and without atomics: results are
 * bit-reproducible from call to call.  Multi-rank jobs: the call is local to the calling rank's shard (all cameras, its
 * observations and points), no collective: a camera is resected from the shard's observations alone.  The cameras are
 * replicated and ba_solve needs them bitwise identical on every rank, so write_cams = 1 is refused when world > 1
 * (BA_ERR_INVALID, naming write_cams and "multi-rank", the handle left as found; a communicator of one rank is not refused):
 * resect with write_cams = 0 and hand every rank the same poses (ba_set_params).  Pinned on two ranks
 * (tests/test_gpu_multirank_local.py). */
enum ba_resect_status { BA_RESECT_OK = 0, BA_RESECT_FEW_POINTS = 1, BA_RESECT_DEGENERATE = 2,
                        BA_RESECT_BEHIND = 3, BA_RESECT_FEW_INLIERS = 4, BA_RESECT_HIGH_ERROR = 5 };
enum ba_resect_init   { BA_RESECT_INIT_DLT = 0, BA_RESECT_INIT_CURRENT = 1 };
typedef struct ba_resect_options {
  int32_t loss;          /* ba_loss of the refinement */
  int32_t refine_iters;  /* most damped Gauss-Newton steps; 0 = the start only */
  double  f_scale;
  int32_t init;          /* ba_resect_init */
  int32_t min_inliers;   /* FEW_INLIERS below this; default 6 */
  double  max_reproj_px; /* inlier test on |r_i|; <= 0: every observation in front of the camera is an inlier */
  double  max_rms_px;    /* HIGH_ERROR when the inliers' rms exceeds it; <= 0: no test */
  double  min_depth;     /* an observation is "behind" when its depth (sign of the model: +z pinhole, -z BAL) <= min_depth */
  int32_t write_cams;
  int32_t reserved0;     /* must be 0 */
} ba_resect_options;
int ba_default_resect_options(ba_resect_options* opts);   /* linear, 20, 1.0, DLT, 6, 0, 0, 0.0, 0 */
int ba_resect(ba_handle* h, const double* intr, const ba_resect_options* opts, const uint8_t* cam_sel, const uint8_t* pt_known,
              double* poses, uint8_t* status, int32_t* n_inliers, double* rms_px, double* max_px);
/* RANSAC resection: the pose of every selected camera from raw matches, a share of which may be wrong (the reference's
 * estimate_pose_pnp: cv2.solvePnPRansac; the image registration of COLMAP, OpenMVG, ORB-SLAM).  intr, cam_sel, pt_known, poses,
 * status (ba_resect_status), n_inliers, rms_px, max_px and the rule for a camera that is not selected are ba_resect's.
 *   obs_inlier  uint8[n_obs] in the caller's observation order (that of ba_residuals), or NULL: 1 for the observations of the
 *               final consensus set -- the inliers counted in n_inliers -- and 0 for every other one: observations of cameras
 *               that are not selected, of points that are not known, those whose bearing failed, and those of a camera whose
 *               status is FEW_POINTS or DEGENERATE without a pose.  What a pipeline deletes before the next solve.
 * Per selected camera, over its n usable observations (point known, bearing exists), indexed 0 .. n - 1 in the handle's
 * camera-ordered list (within a camera: ascending in the handle's internal point number -- the caller's point index while the
 * camera table fits the point passes' LDS, DESIGN.md section 3 -- which is the caller's order only when that ascends in the point):
 * (1) n < 4: FEW_POINTS (three points reproduce themselves; a fourth chooses among P3P's solutions).
 * (2) Hypothesis h = 0 .. n_hyp - 1 draws three distinct indices.  mix(z) is the splitmix64 finaliser: z ^= z >> 30;
 * z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31.  With G = 0x9E3779B97F4A7C15 and everything
 * modulo 2^64: k = mix(mix(mix(seed + G) + camera) + h), draw_d = mix(k + (d + 1) G) for d = 0, 1, 2, and
 * i_d = floor(draw_d (n - d) / 2^64).  Then i_1 += 1 if i_1 >= i_0; i_2 += 1 if i_2 >= min(i_0, i_1), and again if then
 * i_2 >= max(i_0, i_1).  No state is carried between hypotheses and nothing is retried: the samples are a pure function of
 * (seed, camera index, h, n).
 * (3) P3P on the three unit rays ((x, y, 1) of the bearing, normalised, towards the scene) and points, by Lambda Twist (Persson &
 * Nordberg 2018): a cubic (closed form and four Newton steps), the eigen-decomposition of a singular symmetric 3 x 3 (cyclic
 * Jacobi), two quadratics, three Newton steps on the three cosine-law equations per root, in fp64.  Up to four poses, numbered
 * 2 * plane + root; a pose is kept when its three depths are > min_depth.  A triple with |d12 x d13| <= 1e-6 max |d_ij|^2
 * (collinear or coincident), a vanishing cubic term or no real solution makes the hypothesis void.
 * (4) Every pose is scored on all n observations through the camera model's own projection: sum of min(|r_i|^2, thr^2), thr =
 * max_reproj_px, an observation at depth <= min_depth costs thr^2.  The lowest cost wins; ties go to the lower h, then to the
 * lower pose number.  Every hypothesis void: DEGENERATE with the current pose, 0 inliers and NaN measures.
 * (5) lo_rounds times: the consensus set = the usable observations in front of the camera with |r_i| <= thr at the round's
 * starting pose; ba_resect's step (3) on that set only (loss, f_scale, refine_iters apply within it).  An empty set ends the
 * rounds; a failed 6 x 6 pivot gives DEGENERATE with the last accepted pose and its measures.
 * (6) ba_resect's steps (4) and (5) at the final pose with max_reproj_px = thr.
 * write_cams as in ba_resect (the same merge, the same state afterwards, refused with BA_ERR_STATE naming "priors" while priors
 * are set).  BA_ERR_STATE before ba_set_problem / ba_set_params.  BA_ERR_INVALID, naming the field: n_hyp outside 1 .. 4096,
 * lo_rounds < 0, max_reproj_px not > 0, an unknown loss, f_scale not > 0, refine_iters < 0, min_inliers < 0.  Results are
 * bit-reproducible from call to call (fixed-order sums, no atomics, one lexicographic arg-min).  Multi-rank jobs: local to the
 * calling rank's shard, no collective; obs_inlier covers the shard's observations in the shard's order; write_cams = 1 is
 * refused when world > 1 as in ba_resect (BA_ERR_INVALID naming write_cams and "multi-rank").  Pinned on two ranks
 * (tests/test_gpu_multirank_local.py). */
typedef struct ba_ransac_options {
  int32_t  n_hyp;          /* minimal samples per camera, 1 .. 4096; default 256 */
  int32_t  lo_rounds;      /* rounds of (consensus at the current pose, refinement on it); default 2; 0 = the best raw hypothesis */
  uint64_t seed;           /* default 0 */
  double   max_reproj_px;  /* consensus and inlier threshold; must be > 0; default 4.0 */
  int32_t  loss;           /* ba_loss of the refinement ON THE CONSENSUS SET; default linear */
  int32_t  refine_iters;   /* per round; default 20 */
  double   f_scale;        /* default 1.0 */
  int32_t  min_inliers;    /* default 6 */
  int32_t  write_cams;     /* as ba_resect */
  double   max_rms_px;     /* as ba_resect; <= 0: no test */
  double   min_depth;      /* as ba_resect */
} ba_ransac_options;
int ba_default_ransac_options(ba_ransac_options* opts);   /* 256, 2, 0, 4.0, linear, 20, 1.0, 6, 0, 0.0, 0.0 */
int ba_resect_ransac(ba_handle* h, const double* intr, const ba_ransac_options* opts, const uint8_t* cam_sel, const uint8_t* pt_known,
                     double* poses, uint8_t* status, int32_t* n_inliers, double* rms_px, double* max_px, uint8_t* obs_inlier);
/* Two-view relative pose: R | t of the second view against the first from raw pixel matches, a share of which may be wrong (the
 * reference's estimate_pose: cv2.findEssentialMat(RANSAC, 0.999, 3.0) then cv2.recoverPose).  Convention x2 ~ K (R x1 + t), P1 =
 * K [I | 0], |t| = 1: what comes back goes straight into ba_triangulate.  Needs no ba_set_problem and leaves a resident problem
 * untouched; the staging buffers live on the handle and are reused.  n_pairs pairs in one call; pair p owns the matches
 * pair_off[p] .. pair_off[p + 1] - 1 of pts1 / pts2 (double[.][2], pixels).  K is the pinhole matrix (fx, fy > 0, no skew, last row
 * 0 0 1), shared by both views and all pairs; users of the BAL camera pass undistorted bearings with K = I and max_epi_px in
 * normalised units.  Outputs, any of them NULL: R double[n_pairs][9] row-major, t double[n_pairs][3], status uint8
 * (ba_relpose_status), n_inliers, rms_px, parallax_deg, best_hyp int32 (the winning hypothesis, -1 when there is none),
 * match_inlier uint8[pair_off[n_pairs]].  n_pairs = 0 is a no-op.
 * Per pair with n matches:
 * (0) x~ = ((u - cx) / fx, (v - cy) / fy, 1) in both views; fbar = (fx + fy) / 2, thr = max_epi_px / fbar.
 * (1) n < 6: FEW_MATCHES (five matches reproduce themselves; a sixth chooses among the solutions); R = I, t = 0.
 * (2) Hypothesis h = 0 .. n_hyp - 1 draws five distinct indices with ba_resect_ransac's generator: k = mix(mix(mix(seed + G) +
 * pair) + h), draw_d = mix(k + (d + 1) G) for d = 0 .. 4, i_d = floor(draw_d (n - d) / 2^64), then i_d is raised by one for each
 * earlier index that is <= it, the earlier indices taken in ascending order.  A pure function of (seed, pair index in the
 * call, h, n); nothing is retried.
 * (3) Five-point solver (Nister 2004, the polynomial route, fp64).  The rows kron((x2~), (x1~)) form A (5 x 9); Gauss-Jordan, the
 * pivot of each row its largest entry among the columns not used yet, gives the null-space basis N0 .. N3 (free column k: N_k = 1
 * there, minus the reduced row entries at the pivot columns), E = x N0 + y N1 + z N2 + N3; a pivot <= 1e-12 times the largest
 * entry of A voids the hypothesis.  The nine entries of E E^T E - tr(E E^T) E / 2 and det E are ten cubics in (x, y, z), a 10 x 20
 * matrix with the columns x3 y3 x2y xy2 x2z x2 y2z y2 xyz xy | xz2 xz x yz2 yz y z3 z2 z 1, built by polynomial products;
 * Gauss-Jordan on the first ten columns with row pivoting (a pivot <= 1e-12 of the column's largest magnitude over the ten rows:
 * void).  Rows 4 - z 5, 6 - z 7, 8 - z 9 form B(z), 3 x 3 on (x, y, 1), degrees 3, 3, 4; det B(z) has degree 10.  Its real roots
 * inside the Cauchy bound B = 1 + max |c_i / c_10| (not finite: void): the roots of each derivative, from the ninth down, split
 * [-B, B] into intervals of which every one with a sign change is bisected 64 times; then two Newton steps on the polynomial,
 * kept inside the bracket.  At most ten roots, numbered by ascending z: the slot.  Per root (x, y, 1) is the longest cross
 * product of two rows of B(z) (third component 0: void slot), polished by two Gauss-Newton steps of (x, y, z) on the ten
 * eliminated rows (3 x 3 normal equations); E has unit Frobenius norm; a non-finite entry voids the slot.
 * (4) Every E is scored on all n matches: sum of min(r^2, thr^2), r = x2~^T E x1~ / sqrt((E x1~)_0^2 + (E x1~)_1^2 + (E^T x2~)_0^2
 * + (E^T x2~)_1^2) (Sampson), a zero denominator costs thr^2.  The lowest (cost, 10 h + slot) wins, ties go to the lower key.
 * Every slot void: DEGENERATE, R = I, t = 0, 0 inliers, NaN measures, best_hyp = -1.
 * (5) E = U diag V^T (one-sided Jacobi; u3 = u1 x u2, v3 = v1 x v2, so det U = det V = +1).  R_a = U W V^T, R_b = U W^T V^T, W =
 * [0 -1 0; 1 0 0; 0 0 1], t = +-u3; candidates (R_a, +t), (R_a, -t), (R_b, +t), (R_b, -t).  The depths of lambda2 x2~ = lambda1 R
 * x1~ + t in least squares (2 x 2; none when the Gram determinant is <= 1e-24 |a|^2 |b|^2).  The matches with |r| <= thr at the
 * winning E vote for every candidate that puts both depths in (0, max_depth]; most votes win, ties go to the lower number; no
 * vote at all: BEHIND with candidate 0 and its measures.  (Matches of a pure rotation have no finite depth: BEHIND unless
 * max_depth <= 0.)
 * (6) lo_rounds times: the consensus set = the matches with |r| <= thr and both depths in range at the round's starting pose, r
 * from E = [t]x R; an empty set ends the rounds.  Then at most refine_iters Marquardt-damped Gauss-Newton steps on 0.5 sum r^2
 * over the set in five local parameters, R <- exp([w]x) R, t <- normalise(t + tau1 b1 + tau2 b2), b1 = normalise(e_k x t) with k the
 * index of the smallest |t_k|, b2 = t x b1; analytic Jacobian; damping, acceptance and lambda limits as ba_resect's step (3); |dx| <=
 * 1e-14 ends it; a 5 x 5 Cholesky pivot <= 0: DEGENERATE with the last accepted pose and its measures.
 * (7) At the final pose: match_inlier = |r| <= thr with both depths in range, n_inliers their count, rms_px = fbar sqrt(mean r^2)
 * and parallax_deg = the mean angle between R x1~ and x2~ over them (NaN without inliers).  Status: the first failing test in
 * enum order; FEW_INLIERS: n_inliers < min_inliers; LOW_PARALLAX: min_parallax_deg > 0 and parallax_deg below it.
 * BA_ERR_INVALID, naming the field: K not as above, n_pairs outside 0 .. 65535, n_hyp outside 1 .. 4096, lo_rounds < 0, max_epi_px
 * not > 0, refine_iters < 0, min_inliers < 0, pair_off[0] != 0, a decreasing pair_off.  Results are bit-reproducible from call
 * to call, and a pair's result depends on its index in the call (the samples) but not on the other pairs.  Local to the rank. */
enum ba_relpose_status { BA_RELPOSE_OK = 0, BA_RELPOSE_FEW_MATCHES = 1, BA_RELPOSE_DEGENERATE = 2,
                         BA_RELPOSE_BEHIND = 3, BA_RELPOSE_FEW_INLIERS = 4, BA_RELPOSE_LOW_PARALLAX = 5 };
typedef struct ba_relpose_options {
  int32_t  n_hyp;            /* minimal samples per pair, 1 .. 4096; default 256 */
  int32_t  lo_rounds;        /* rounds of (consensus, refinement); default 2; 0 = the best raw hypothesis, decomposed */
  uint64_t seed;             /* default 0 */
  double   max_epi_px;       /* Sampson threshold in pixels, > 0; default 3.0 (the reference's) */
  int32_t  refine_iters;     /* per round; default 20 */
  int32_t  min_inliers;      /* default 8 */
  double   min_parallax_deg; /* <= 0: no test; default 0 */
  double   max_depth;        /* a match votes / is in front when both depths are in (0, max_depth], unit = |t| = 1;
                                <= 0: no upper limit; default 50 (cv2.recoverPose's distanceThresh) */
} ba_relpose_options;
int ba_default_relpose_options(ba_relpose_options* opts);   /* 256, 2, 0, 3.0, 20, 8, 0.0, 50.0 */
int ba_relative_pose(ba_handle* h, const double K[9], int32_t n_pairs, const int64_t* pair_off, const double* pts1, const double* pts2,
                     const ba_relpose_options* opts, double* R, double* t, uint8_t* status, int32_t* n_inliers, double* rms_px,
                     double* parallax_deg, int32_t* best_hyp, uint8_t* match_inlier);
/* Two-view homography: the plane-induced H of raw pixel matches, a share of which may be wrong, and the poses it decomposes
 * into -- the planar model next to ba_relative_pose's essential one (cv2.findHomography(RANSAC) then cv2.decomposeHomographyMat;
 * the H half of ORB-SLAM's initialiser and of COLMAP's two-view geometry).  Exactly coplanar matches admit two essential matrices
 * of zero Sampson cost, so a planar scene is decided here and not there.  K, n_pairs, pair_off, pts1, pts2, the staging buffers
 * on the handle and the rule that no problem is needed or touched are ba_relative_pose's.  Convention x2~ ~ H~ x1~ with H~ / d2 = R +
 * (t / d) n^T: x2 ~ K (R x1 + t), the plane n . X = d in the first view's frame, |t| = |n| = 1, d2 the middle singular value.
 * Outputs, any of them NULL: H double[n_pairs][9] row-major, in PIXELS (p2 ~ H p1), unit Frobenius norm, det > 0; status uint8
 * (ba_homography_status), n_inliers, rms_px, best_hyp int32 (the winning hypothesis, -1 when there is none), match_inlier
 * uint8[pair_off[n_pairs]], n_pose int32, and per pair TWO poses, the better first: R double[n_pairs][2][9], t and normal
 * double[n_pairs][2][3], t_over_d double[n_pairs][2] (|t| / d before t was scaled to 1), votes int32[n_pairs][2], pose_cost
 * double[n_pairs][2].  n_pairs = 0 is a no-op.
 * Per pair with n matches:
 * (0) x~ = ((u - cx) / fx, (v - cy) / fy, 1) in both views; fbar = (fx + fy) / 2, thr = max_px / fbar.
 * (1) n < 5: FEW_MATCHES (four matches reproduce themselves); H = I, no pose.
 * (2) Hypothesis h = 0 .. n_hyp - 1 draws four distinct indices with ba_relative_pose's generator, d = 0 .. 3, and the same raising
 * rule.  A triple of the four with |d12 x d13| <= 1e-6 max |d_ij|^2 in either image (collinear or coincident) voids the hypothesis.
 * (3) Closed form, fp64, one lane per hypothesis, no elimination: per image M = [a b c] (the first three points as homogeneous
 * columns), lambda = adj(M) d (d the fourth), B = M diag(lambda); H~ = B2 adj(B1), scaled to unit Frobenius norm and det > 0.
 * |det| <= 1e-12 at unit norm, a non-finite entry, or a sample point with (H~ x1~)_2 <= 0 (cv2's orientation check) voids it.
 * (4) Every H~ is scored on all n matches: f = |pi(H~ x1~) - x2~|^2, b = |pi(adj(H~) x2~) - x1~|^2, the cost is the sum of min(f,
 * thr^2) + min(b, thr^2), a non-positive third component costs thr^2.  The lowest (cost, h) wins.  Every hypothesis void:
 * DEGENERATE, H = I, 0 inliers, NaN measures, best_hyp = -1, n_pose = 0.
 * (5) lo_rounds times: the consensus set = the matches with f <= thr^2, b <= thr^2 and both third components positive at the
 * round's starting H~; an empty set ends the rounds.  Then at most refine_iters Marquardt-damped Gauss-Newton steps on 0.5 sum
 * (|r_f|^2 + |r_b|^2) over the set (a trial H~ at which a third component of a match of the set is not positive is rejected:
 * its cost counts as infinite) in the eight local
 * parameters of H~ <- H~ (I + D), D = [p0 p1 p2; p3 p4 p5; p6 p7 -(p0 + p4)] traceless; to first order the backward residual sees
 * (I - D) H~^-1; both Jacobians analytic; after a step H~ (I + D) is formed exactly and renormalised as in (3).  Damping, acceptance
 * and lambda limits as ba_resect's step (3); |dx| <= 1e-14 ends it; an 8 x 8 Cholesky pivot <= 0 (or a non-finite step):
 * DEGENERATE with the last accepted H~ and its measures.
 * (6) At the final H~: match_inlier = the consensus test of (5), n_inliers their count, rms_px = fbar sqrt(mean (f + b) / 2) over
 * them (NaN without inliers); H = K H~ K^-1 at unit Frobenius norm, det > 0.
 * (7) H~ = U diag(d1, d2, d3) V^T (one-sided Jacobi; u3 = u1 x u2, v3 = v1 x v2, so det U = det V = +1 and d1 >= d2 >= d3 > 0).
 * (d1 - d3) / d2 <= min_translation (it equals |t| / d): ROTATION, one pose R = U V^T with t = 0, normal = 0, t_over_d = the ratio,
 * n_pose = 1.  Otherwise Faugeras & Lustman's (1988) candidates of the case d' = +d2: a1 = sqrt((d1^2 - d2^2) / (d1^2 - d3^2)), a3 =
 * sqrt((d2^2 - d3^2) / (d1^2 - d3^2)), cos = (d2^2 + d1 d3) / ((d1 + d3) d2), sin = e sqrt((d1^2 - d2^2) (d2^2 - d3^2)) / ((d1 + d3) d2),
 * R = U [cos 0 -sin; 0 1 0; sin 0 cos] V^T, t = U (a1, 0, -e a3), n = V (a1, 0, e a3), e = +1 (pose number 0) or -1 (number 1),
 * t_over_d = (d1 - d3) / d2; the other two candidates flip both t and n, and of each such couple the one with n . x1~ > 0 for more
 * inliers than n . x1~ < 0 is kept (a tie keeps the one above).  An inlier votes for a pose when both depths of lambda2 x2~ =
 * lambda1 R x1~ + t (ba_relative_pose's step 5) lie in (0, max_depth] and n . x1~ > 0.  pose_cost is the MSAC cost of the squared
 * Sampson distance of [t]x R on all matches with threshold thr (ba_relative_pose's step 4).  The poses are ordered by votes
 * descending, then pose_cost ascending, then number; n_pose counts those with at least one vote.  AMBIGUOUS when the second
 * pose's votes are >= ambiguity_ratio times the first's (ORB-SLAM's rule); both poses are returned either way.
 * (8) Status: the first failing test in enum order; FEW_INLIERS: n_inliers < min_inliers.  A status other than FEW_MATCHES or a
 * DEGENERATE of step (4) comes with the final H, its measures and its decomposition.
 * BA_ERR_INVALID, naming the field: K not as in ba_relative_pose, n_pairs outside 0 .. 65535, n_hyp outside 1 .. 4096, lo_rounds < 0,
 * max_px not > 0, refine_iters < 0, min_inliers < 0, ambiguity_ratio outside [0, 1], min_translation negative or NaN, pair_off[0]
 * != 0, a decreasing pair_off.  Results are bit-reproducible from call to call, and a pair's result depends on its index in the
 * call (the samples) but not on the other pairs.  Local to the rank. */
enum ba_homography_status { BA_HOMOGRAPHY_OK = 0, BA_HOMOGRAPHY_FEW_MATCHES = 1, BA_HOMOGRAPHY_DEGENERATE = 2,
                            BA_HOMOGRAPHY_FEW_INLIERS = 3, BA_HOMOGRAPHY_ROTATION = 4, BA_HOMOGRAPHY_AMBIGUOUS = 5 };
typedef struct ba_homography_options {
  int32_t  n_hyp;            /* minimal samples per pair, 1 .. 4096; default 256: at an inlier share of 0.5 all of them miss with
                                probability (1 - 0.5^4)^256 = 7e-8 */
  int32_t  lo_rounds;        /* rounds of (consensus, refinement); default 2; 0 = the best raw hypothesis, decomposed */
  uint64_t seed;             /* default 0 */
  double   max_px;           /* threshold on each transfer error in pixels, > 0; default 3.0 */
  int32_t  refine_iters;     /* per round; default 20 */
  int32_t  min_inliers;      /* default 8 */
  double   max_depth;        /* a match votes when both depths are in (0, max_depth], unit = |t| = 1; <= 0: no upper limit; default 50 */
  double   ambiguity_ratio;  /* in [0, 1]; default 0.75 */
  double   min_translation;  /* ROTATION when (d1 - d3) / d2 = |t| / d is not above it; default 0.024 */
} ba_homography_options;
int ba_default_homography_options(ba_homography_options* opts);   /* 256, 2, 0, 3.0, 20, 8, 50.0, 0.75, 0.024 */
int ba_homography(ba_handle* h, const double K[9], int32_t n_pairs, const int64_t* pair_off, const double* pts1, const double* pts2,
                  const ba_homography_options* opts, double* H, uint8_t* status, int32_t* n_inliers, double* rms_px, int32_t* best_hyp,
                  uint8_t* match_inlier, int32_t* n_pose, double* R, double* t, double* normal, double* t_over_d, int32_t* votes,
                  double* pose_cost);
/* Sim(3) from 3D-3D matches: the similarity between two camera frames from matched map points, a share of which may be
 * wrong -- the measurement of a loop edge of ba_pose_graph (ORB-SLAM's Sim3Solver + OptimizeSim3 in ComputeSim3; COLMAP's
 * similarity LO-RANSAC).  X1[k] and X2[k], double[pair_off[n_pairs]][3], are the same physical point in the CAMERA frame of view
 * 1 and of view 2 (z forward, the pinhole convention); the model is X2 ~ s R X1 + t, and stored as rvec | t | s it is the meas of
 * a pose-graph edge (1 -> 2), S_2 o S_1^-1.  K, n_pairs, pair_off, the staging buffers on the handle and the rule that no problem
 * is needed or touched are ba_relative_pose's; K's principal point is not used (no pixels are passed).
 * Outputs, any of them NULL: sim double[n_pairs][7] rvec | t | s, R double[n_pairs][9] row-major, status uint8 (ba_sim3_status),
 * n_inliers, rms_px, best_hyp int32 (the winning hypothesis, -1 when there is none), match_inlier uint8[pair_off[n_pairs]],
 * hessian double[n_pairs][49].  n_pairs = 0 is a no-op.
 * Per pair with n correspondences:
 * (0) x(X) = (X_x / X_z, X_y / X_z); fbar = (fx + fy) / 2, thr = max_px / fbar.  The images are the projections of the points
 * themselves, x1_k = x(X1_k), x2_k = x(X2_k), as in ORB-SLAM's solver.  A correspondence with a non-finite coordinate or z <= 0 in
 * its own frame is invalid: never an inlier, it costs 2 thr^2 under every model, and a sample that draws it is void.
 * (1) n < 4: FEW_MATCHES (three correspondences reproduce themselves); the identity (rvec = t = 0, s = 1, R = I), no inliers, NaN
 * rms_px, a zero hessian, best_hyp = -1.
 * (2) Hypothesis h = 0 .. n_hyp - 1 draws three distinct indices with ba_relative_pose's generator, d = 0 .. 2, item = the pair.
 * A triple with |d12 x d13| <= 1e-6 max |d_ij|^2 in either frame (3D vectors: collinear or coincident) is void.
 * (3) The closed form of ba_align on the three points with unit weights, fp64, one lane per hypothesis: the centroids mu_a,
 * mu_b, the centred Sigma = mean (b - mu_b)(a - mu_a)^T = U D V^T (one-sided Jacobi), R = U diag(1, 1, det U det V) V^T with the
 * third left vector formed as u1 x u2, s = tr(D diag(1, 1, det U det V)) / mean |a - mu_a|^2 (1 when with_scale = 0), t = mu_b - s R
 * mu_a.  Void when s is not finite or not positive, or the second singular value is <= 1e-12 times the first.
 * (4) Every model is scored on all n: f = |x(s R X1 + t) - x2|^2, b = |x(R^T (X2 - t) / s) - x1|^2, the cost is the sum of min(f,
 * thr^2) + min(b, thr^2), a non-positive transformed depth costs thr^2 on its side.  The lowest (cost, h) wins.  Every hypothesis
 * void: DEGENERATE with the outputs of (1).
 * (5) lo_rounds times: the consensus set = the valid correspondences with f <= thr^2, b <= thr^2 and both transformed depths
 * positive at the round's starting model; fewer than three end the rounds.  Then (a) the closed form of (3) on the whole set,
 * centred before Sigma is formed; it replaces the starting model only if its cost (b) over the set is lower (a void one never
 * does).  (b) At most refine_iters Marquardt-damped Gauss-Newton steps on 0.5 sum (|r_f|^2 + |r_b|^2) over the set in the seven
 * local parameters of ba_pose_graph, R <- exp(d omega) R, t <- t + d t, s <- s exp(d sigma) (six without scale: d sigma = 0), both
 * Jacobians analytic (x does not see the 1 / s of the backward map: r_b does not move with d sigma).  A trial model at which a
 * transformed depth of a member of the set is not positive is rejected: its cost counts as infinite.  Damping, acceptance and
 * lambda limits as ba_resect's step (3); |dx| <= 1e-14 ends it; a 7 x 7 Cholesky pivot <= 0 (or a non-finite step): DEGENERATE with
 * the last accepted model and its measures.
 * (6) At the final model: match_inlier = the consensus test of (5), n_inliers their count, rms_px = fbar sqrt(mean (f + b) / 2)
 * over them (NaN without inliers); hessian = fbar^2 J^T J of (5b)'s residuals over the final inliers in (d omega, d t, d sigma),
 * row-major and bit-symmetric (row and column 6 are zero without scale): the information of the model in pixels^-2, see
 * posegraph.edge_information; sim's rvec is the log map of R (|rvec| <= pi).
 * (7) Status: the first failing test in enum order; FEW_INLIERS: n_inliers < min_inliers.
 * BA_ERR_INVALID, naming the field: K not as in ba_relative_pose, n_pairs outside 0 .. 65535, n_hyp outside 1 .. 4096, lo_rounds < 0,
 * refine_iters < 0, min_inliers < 0, max_px not > 0, with_scale not 0 or 1, pair_off[0] != 0, a decreasing pair_off.  Results are
 * bit-reproducible from call to call, and a pair's result depends on its index in the call (the samples) but not on the other
 * pairs.  Local to the rank. */
enum ba_sim3_status { BA_SIM3_OK = 0, BA_SIM3_FEW_MATCHES = 1, BA_SIM3_DEGENERATE = 2, BA_SIM3_FEW_INLIERS = 3 };
typedef struct ba_sim3_options {
  int32_t  n_hyp;            /* minimal samples per pair, 1 .. 4096; default 256: at an inlier share of 0.5 all of them miss with
                                probability (1 - 0.5^3)^256 = 1e-15 */
  int32_t  lo_rounds;        /* rounds of (consensus, closed form, refinement); default 2; 0 = the best raw hypothesis */
  uint64_t seed;             /* default 0 */
  double   max_px;           /* threshold on each reprojection error in pixels, > 0; default 4.0 */
  int32_t  refine_iters;     /* per round; default 20 */
  int32_t  min_inliers;      /* default 8 */
  int32_t  with_scale;       /* 1: Sim(3); 0: SE(3), every s exactly 1 (stereo / RGB-D maps); default 1 */
  int32_t  reserved0;
} ba_sim3_options;
int ba_default_sim3_options(ba_sim3_options* opts);   /* 256, 2, 0, 4.0, 20, 8, 1 */
int ba_sim3(ba_handle* h, const double K[9], int32_t n_pairs, const int64_t* pair_off, const double* X1, const double* X2,
            const ba_sim3_options* opts, double* sim, double* R, uint8_t* status, int32_t* n_inliers, double* rms_px, int32_t* best_hyp,
            uint8_t* match_inlier, double* hessian);
/* Two-view fundamental matrix: the F of raw pixel matches of an UNCALIBRATED pair, a share of which may be wrong -- the one
 * two-view model that needs no K (cv2.findFundamentalMat(FM_RANSAC); the F half of COLMAP's uncalibrated two-view geometry).
 * Convention p2^T F p1 = 0 in pixels, what ba_match_guided's epipolar gate takes.  n_pairs, pair_off, pts1, pts2, the staging
 * buffers on the handle and the rule that no problem is needed or touched are ba_relative_pose's; there is no K.
 * Outputs, any of them NULL: F double[n_pairs][9] row-major, in PIXELS, unit Frobenius norm, its largest-magnitude entry positive
 * (the first in row-major order of equal ones); status uint8 (ba_fundamental_status), n_inliers, rms_px, best_hyp int32 (the
 * winning hypothesis, -1 when there is none), match_inlier uint8[pair_off[n_pairs]], epipole1 and epipole2 double[n_pairs][3]: F
 * e1 = 0 and F^T e2 = 0, homogeneous pixels at unit length, the largest-magnitude component positive (the first of equal ones;
 * an epipole at infinity has a third component near 0).  n_pairs = 0 is a no-op.
 * Per pair with n matches:
 * (0) n < 8: FEW_MATCHES (seven matches reproduce themselves under up to three F; an eighth chooses).  The row of a pair without
 * a model, here and in every DEGENERATE below that says so: F = 0 (all nine entries: not a fundamental matrix, where
 * ba_homography's H = I would be a rank-3 one), n_inliers = 0, rms_px = NaN, best_hyp = -1, epipole1 = epipole2 = 0, no match an
 * inlier.
 * (1) Hartley normalisation, per image over ALL n matches: c = the centroid, s = sqrt(2) / mean |p - c|; q = p - c are centred
 * pixels, x~ = (s q, 1) normalised ones, S = diag(s, s, 1).  A mean distance that is zero or not finite in either image:
 * DEGENERATE, the row of (0).  Sums in a fixed order, no atomics.
 * (2) Hypothesis h = 0 .. n_hyp - 1 draws seven distinct indices with ba_relative_pose's generator, d = 0 .. 6, and the same raising
 * rule.  Seven-point solver, fp64, one lane per hypothesis: the rows kron(x2~, x1~) form A (7 x 9); Gauss-Jordan by rows, the
 * pivot of row r its largest entry among the columns not used yet (the first of equal ones); a pivot <= 1e-12 times the FIRST
 * pivot, or not finite, voids the hypothesis (rank below 7).  The pivot column of row r changes places with the column at place
 * r, which leaves the two free columns at places 7 and 8; they give the null vectors: N_k = 1 at its free column, 0 at the other,
 * minus the reduced rows' entries at the pivot columns; F1 = N of place 7, F2 = N of place 8.  det(a F1 + (1 - a) F2) = c3 a^3 + c2 a^2 + c1 a + c0 with D = F1 - F2, c0 = det F2, c1 = tr(adj(F2) D), c2 = tr(adj(D)
 * F2), c3 = det D.  |c3| <= 1e-12 max(|c0|, |c1|, |c2|) (F1 - F2 itself is singular: a root at infinity, the others ill-scaled in
 * a) or a non-finite coefficient voids the hypothesis.  Its real roots inside the Cauchy bound B = 1 + max |c_i / c3|: the real
 * critical points (discriminant c2^2 - 3 c3 c1 > 0) split [-B, B] into intervals of which every one with a sign change is bisected
 * 64 times, then two Newton steps kept inside the bracket.  At most three roots, numbered by ascending a: the slot.  F~ = a F1 +
 * (1 - a) F2 at unit Frobenius norm; a non-finite entry voids the slot.
 * (3) Every F~ is scored on all n matches in centred pixels with F_c = S2 F~ S1: the sum of min(d^2, max_epi_px^2), d^2 = (q2^T F_c
 * q1)^2 / ((F_c q1)_x^2 + (F_c q1)_y^2 + (F_c^T q2)_x^2 + (F_c^T q2)_y^2) (Sampson; it does not change under translation, so it is the
 * pixel distance), a zero denominator costs max_epi_px^2.  The lowest (cost, 3 h + slot) wins, ties go to the lower key.  Every
 * slot void: DEGENERATE, the row of (0).
 * (4) lo_rounds times: the consensus set = the matches with d^2 <= max_epi_px^2 at the round's starting F~ (a zero denominator is
 * never in, here and in (5)); fewer than 8 end the rounds.  F~ = U diag(d1, d2, d3) V^T (one-sided Jacobi; u3 = u1 x u2, v3 = v1 x v2, so det U = det V = +1), sigma = d2 / d1, and
 * the model is U diag(1, sigma, 0) V^T (a non-finite entry: DEGENERATE with the round's starting F~ and its measures).  Then at
 * most refine_iters Marquardt-damped Gauss-Newton steps on 0.5 sum d^2 (signed Sampson distances in centred pixels) over the set
 * in the seven local parameters of that orthonormal representation, U <- U exp([a]x), V <- V exp([b]x), sigma <- sigma + ds
 * (ba_relative_pose's chart with the singular-value ratio freed); analytic Jacobian; damping, acceptance and lambda limits as
 * ba_resect's step (3); |dx| <= 1e-14 ends it; a 7 x 7 Cholesky pivot <= 0 (or a non-finite step): DEGENERATE with the last
 * accepted model and its measures.  The round ends with F~ = U diag(1, sigma, 0) V^T at unit Frobenius norm.  With lo_rounds = 0
 * the best raw hypothesis is measured as it is.
 * (5) At the final F~: match_inlier = d^2 <= max_epi_px^2, n_inliers their count, rms_px = sqrt(mean d^2) over them (NaN without
 * inliers); F = T2^T F_c T1, T = [1 0 -cx; 0 1 -cy; 0 0 1], normalised and signed as above; the epipoles from F~ = U diag V^T
 * again: e1 = T1^-1 S1^-1 v3, e2 = T2^-1 S2^-1 u3.
 * (6) Status: the first failing test in enum order; FEW_INLIERS: n_inliers < min_inliers.
 * BA_ERR_INVALID, naming the field: n_pairs outside 0 .. 65535, n_hyp outside 1 .. 4096, lo_rounds < 0, max_epi_px not > 0,
 * refine_iters < 0, min_inliers < 0, pair_off[0] != 0, a decreasing pair_off.  Pixels that are not finite are not refused (the
 * sibling calls do not either): they make their pair DEGENERATE in step (1).  Results are bit-reproducible from call to call,
 * and a pair's result depends on its index in the call (the samples) but not on the other pairs.  Local to the rank.
 * Not offered: adaptive stopping, PROSAC, an eight-point refit, a degeneracy test for planes (run ba_homography beside it:
 * pose_estimator.estimate_uncalibrated), radial distortion, pose recovery from F. */
enum ba_fundamental_status { BA_FUNDAMENTAL_OK = 0, BA_FUNDAMENTAL_FEW_MATCHES = 1, BA_FUNDAMENTAL_DEGENERATE = 2,
                             BA_FUNDAMENTAL_FEW_INLIERS = 3 };
typedef struct ba_fundamental_options {
  int32_t  n_hyp;            /* minimal samples per pair, 1 .. 4096; default 1024, not the siblings' 256: a seven-point sample at an
                                inlier share of 0.5 is clean with probability 0.5^7 = 1 / 128, so all of 256 miss with probability
                                (1 - 0.5^7)^256 = 0.13, all of 1024 with 3e-4, all of 2048 with 1e-7 */
  int32_t  lo_rounds;        /* rounds of (consensus, refinement); default 2; 0 = the best raw hypothesis */
  uint64_t seed;             /* default 0 */
  double   max_epi_px;       /* Sampson threshold in pixels, > 0; default 3.0 */
  int32_t  refine_iters;     /* per round; default 20 */
  int32_t  min_inliers;      /* default 16 */
} ba_fundamental_options;
int ba_default_fundamental_options(ba_fundamental_options* opts);   /* 1024, 2, 0, 3.0, 20, 16 */
int ba_fundamental(ba_handle* h, int32_t n_pairs, const int64_t* pair_off, const double* pts1, const double* pts2,
                   const ba_fundamental_options* opts, double* F, uint8_t* status, int32_t* n_inliers, double* rms_px, int32_t* best_hyp,
                   uint8_t* match_inlier, double* epipole1, double* epipole2);
/* Descriptor matching: brute-force Hamming 2-nearest-neighbours of binary descriptors with Lowe's ratio test, the step that
 * produces the matches ba_relative_pose starts from (the reference's BruteForceMatcher.match: cv2.BFMatcher(NORM_HAMMING,
 * crossCheck=False).knnMatch(des1, des2, k=2), then m.distance < 0.75 n.distance).  Needs no ba_set_problem and leaves a resident
 * problem untouched; the staging buffers live on the handle and are reused.  Local to the rank.
 * Inputs: desc is uint8[set_off[n_sets]][desc_bytes], set s owns the rows set_off[s] .. set_off[s + 1] - 1; every set is uploaded
 * once per call, however many pairs use it.  Pair p matches every descriptor of set pair_query[p] (the queries) against set
 * pair_train[p]; a set may be matched against itself.  desc_bytes is a multiple of 8 in 8 .. 64 (ORB 32, BRISK 64); a caller
 * with another length pads both sides with equal bytes, which adds nothing to any distance.
 * Outputs, any of them NULL, by row: row row_off[p] + i belongs to query i of pair p; row_off int64[n_pairs + 1] is the exclusive
 * prefix sum of the pairs' query-set sizes, computed and written by the library.  best, second, dist1, dist2 int32[rows], good
 * uint8[rows], n_good int32[n_pairs].
 * Per pair with nq queries and nt train descriptors: d(i, j) = popcount of the XOR of the two rows.  The train descriptors of
 * query i are ordered by the key (d(i, j), j): ties go to the lower index.  best / dist1 are the first entry of that order,
 * second / dist2 the second; nt = 0: best = second = dist1 = dist2 = -1; nt = 1: second = dist2 = -1.  This is the order cv2's
 * knnMatch leaves by inserting the neighbours in index order (crossCheck=False); cv2 is not part of this project's test
 * environment, so equality with cv2 on ties rests on its source and is NOT verified.
 * good[i] = 1 if and only if all of: best >= 0; ratio <= 0, or second >= 0 and (double)dist1 < ratio * (double)dist2 in fp64
 * exactly as written (with nt < 2 and a ratio test nothing is good, as the reference returns an empty list then);
 * max_distance < 0, or dist1 <= max_distance; mutual = 0, or i is the first query under the key (d(i', best), i') over all
 * queries i' of the pair (i is the best query of its best train descriptor, ties to the lower query; NOT cv2's crossCheck, which
 * drops the ratio test's second neighbour).  n_good[p] = the number of good queries of pair p.
 * n_pairs = 0, empty sets and empty query sets are no-ops with well-formed outputs (row_off written, n_good zero).
 * BA_ERR_INVALID, naming the field: desc_bytes not as above; n_sets or n_pairs outside 0 .. 65535; ratio not finite; set_off NULL,
 * set_off[0] != 0, a decreasing set_off, a set of more than 2^20 descriptors; desc NULL with descriptors to read; pair_query /
 * pair_train NULL with n_pairs > 0 or an index outside 0 .. n_sets - 1.  A refused call leaves the handle usable.
 * Results are pure integer arithmetic and bit-reproducible; a pair's rows do not depend on the other pairs of the call, nor on
 * how the library splits the train set over workgroups (csrc/ba_match.hpp).  Not offered: k > 2; uint8 descriptors under the L2
 * distance (SIFT) are ba_match_l2's, candidate masks ba_match_guided's (both below). */
typedef struct ba_match_options {
  double  ratio;         /* keep a query when (double)d1 < ratio * (double)d2, in fp64 exactly as written; <= 0: no ratio test; default 0.75 */
  int32_t max_distance;  /* keep only d1 <= max_distance; < 0: no test; default -1 */
  int32_t mutual;        /* 1: keep (i, j) only if i is also the best query of train j under the same order; default 0 */
} ba_match_options;      /* 16 bytes */
int ba_default_match_options(ba_match_options* opts);    /* 0.75, -1, 0 */
int ba_match_descriptors(ba_handle* h, int32_t desc_bytes, int32_t n_sets, const int64_t* set_off, const uint8_t* desc,
                         int32_t n_pairs, const int32_t* pair_query, const int32_t* pair_train, const ba_match_options* opts,
                         int64_t* row_off, int32_t* best, int32_t* second, int32_t* dist1, int32_t* dist2,
                         uint8_t* good, int32_t* n_good);
/* L2 descriptor matching: exact brute-force 2-nearest-neighbours of uint8 descriptors under the squared Euclidean distance with
 * Lowe's ratio test -- SIFT and RootSIFT as COLMAP stores them (128 uint8 per keypoint), learned descriptors quantised the same
 * way.  The surface is ba_match_descriptors' with another metric: sets, pairs, rows, row_off, the outputs (any of them NULL), the
 * -1 conventions for nt = 0 and nt = 1, the empty cases and every refusal are as there, word for word, with messages that name
 * ba_match_l2 (n_sets and n_pairs outside 0 .. 65535 and a set of more than 2^20 descriptors included); ba_match_options is reused
 * unchanged.  Needs no ba_set_problem and leaves a resident problem untouched.  Local to the rank.
 * desc_bytes is a multiple of 32 in 32 .. 256; other values are refused by name.  A caller with another length pads both sides
 * with equal bytes, which adds nothing to any distance.
 * d(i, j) = sum_k (q_ik - t_jk)^2 over the bytes taken as unsigned 0 .. 255, an int32 (at 256 bytes at most 256 * 255^2 =
 * 16 646 400 < 2^24); dist1 / dist2 are this SQUARED distance.  The train rows of query i are ordered by the key (d(i, j), j):
 * ties go to the lower index.  best / dist1 are the first entry of that order, second / dist2 the second.
 * good[i] = 1 if and only if all of: best >= 0; ratio <= 0, or second >= 0 and (double)dist1 < (ratio * ratio) * (double)dist2 in
 * fp64 exactly as written (Lowe's test on the distances, stated on the squares: a zero dist2 never passes, and with nt < 2 and a
 * ratio test nothing is good); max_distance < 0, or dist1 <= max_distance (in squared units); mutual = 0, or i is the first query
 * under the key (d(i', best), i') over all queries i' of the pair, as in ba_match_descriptors under this metric's order.
 * n_good[p] = the number of good queries of pair p.
 * Results are pure integer arithmetic (int8 matrix cores, csrc/ba_match_l2.hpp) and bit-reproducible; a pair's rows do not
 * depend on the other pairs of the call, nor on how the library splits the work.  Equality with cv2.BFMatcher(NORM_L2) on ties
 * is NOT verified (cv2 is not part of this project's test environment).  Not offered: float inputs on the device, k > 2,
 * geometric gates with this metric, cosine or arccos ratio tests, more than one rank. */
int ba_match_l2(ba_handle* h, int32_t desc_bytes, int32_t n_sets, const int64_t* set_off, const uint8_t* desc,
                int32_t n_pairs, const int32_t* pair_query, const int32_t* pair_train, const ba_match_options* opts,
                int64_t* row_off, int32_t* best, int32_t* second, int32_t* dist1, int32_t* dist2,
                uint8_t* good, int32_t* n_good);
/* Guided descriptor matching: ba_match_descriptors over the train rows a geometric GATE admits -- the second matching pass of a
 * pipeline once geometry is known (ORB-SLAM's SearchByProjection / SearchForTriangulation, COLMAP's guided matching).  Sets,
 * pairs, rows, row_off, the key (distance, index), ties, -1 and every refusal are ba_match_descriptors' (messages name
 * ba_match_guided); what is added: xy float32[set_off[n_sets]][2], the keypoint position of every descriptor row (as cv2's
 * KeyPoint.pt), and per call ONE gate kind, options.gate:
 *   BA_GATE_WINDOW    window float32[rows][3] = (px, py, r) per query row in row_off order: the predicted position of the query
 *                     in the train image and a radius.  With (x, y) the train row's xy, all widened to double:
 *                     dx = x - px, dy = y - py; gate(i, j) iff r >= 0 && dx*dx + dy*dy <= r*r.  A negative radius disables
 *                     the query (a point behind the camera or outside the image).
 *   BA_GATE_EPIPOLAR  F double[n_pairs][9] row-major with x_train^T F x_query = 0.  With (x1, y1) the query row's own xy and
 *                     (x, y) the train row's: l0 = (F00*x1 + F01*y1) + F02, l1 and l2 alike from rows 1 and 2;
 *                     n = l0*l0 + l1*l1; e = (l0*x + l1*y) + l2; gate(i, j) iff n > 0 && e*e <= (max_epi_px*max_epi_px) * n.
 *                     One-sided: the train keypoint against the query's line.
 * The gate is evaluated in fp64, every operation rounded on its own as written (no fused multiply-add), so an IEEE double
 * evaluation of the same expressions decides every case identically, border cases included.  A NaN anywhere (xy, window) fails
 * the comparison and so the gate; non-finite xy / window values are not refused.
 * Results: the 2-NN of query i is taken over { j : gate(i, j) } under the same key; n_cand int32[rows] is that set's size.  good
 * as in ba_match_descriptors with one change: with single = 1 a query with best >= 0 and second < 0 passes the ratio test (a
 * search window often holds one keypoint; max_distance is the guard then).  mutual: (i, j) is kept only if i is the lowest
 * (distance, index) among the queries i' with gate(i', j) -- the same predicate.  Results are bit-reproducible and do not
 * depend on the other pairs of the call nor on the split of the train set.  Any output may be NULL.
 * BA_ERR_INVALID in addition, naming the field: xy NULL with rows present; gate not 1 or 2; single not 0 / 1; WINDOW: window NULL
 * with query rows present; EPIPOLAR: F NULL with n_pairs > 0, a non-finite entry of F, max_epi_px not finite or negative.
 * Not offered: both gates in one call, a symmetric epipolar distance, scale / octave gates, candidate lists. */
enum { BA_GATE_WINDOW = 1, BA_GATE_EPIPOLAR = 2 };
typedef struct ba_guided_options {
  double  ratio;         /* as ba_match_options; default 0.75 */
  int32_t max_distance;  /* as ba_match_options; default -1 */
  int32_t mutual;        /* as ba_match_options, under the gate; default 0 */
  int32_t gate;          /* BA_GATE_WINDOW or BA_GATE_EPIPOLAR; no default: 0 is refused */
  int32_t single;        /* 1: a query whose gate admits exactly one train row passes the ratio test; default 1 */
  double  max_epi_px;    /* EPIPOLAR: largest distance of the train keypoint from the query's epipolar line; default 3.0 */
} ba_guided_options;     /* 32 bytes */
int ba_default_guided_options(ba_guided_options* opts);    /* 0.75, -1, 0, 0, 1, 3.0 */
int ba_match_guided(ba_handle* h, int32_t desc_bytes, int32_t n_sets, const int64_t* set_off, const uint8_t* desc, const float* xy,
                    int32_t n_pairs, const int32_t* pair_query, const int32_t* pair_train, const ba_guided_options* opts,
                    const float* window, const double* F, int64_t* row_off, int32_t* best, int32_t* second, int32_t* dist1,
                    int32_t* dist2, uint8_t* good, int32_t* n_good, int32_t* n_cand);
/* ORB feature extraction: the step that produces keypoints and descriptors from a grey image, what the reference's
 * ORBExtractor.extract (cv2.ORB_create(nfeatures = 3000).detectAndCompute) does on the host.  This is ORB BY THE PUBLISHED
 * ALGORITHM -- multi-scale FAST-9, Harris ranking, intensity-centroid orientation, steered BRIEF on a blurred pyramid -- and NOT
 * bit-parity with cv2: neither keypoints nor descriptors are claimed to equal cv2's, and the default test pattern is not
 * OpenCV's learned one (a caller who has that table passes it as `pattern`; descriptors match only descriptors made with the
 * same pattern).  Every stage is integer arithmetic, or fp64 with every operation rounded on its own, so the definition below
 * decides every case, border cases included.  Needs no problem; a resident problem is not touched.
 * images uint8[n_images][height][width], row-major and contiguous, one common size.  Per-keypoint outputs have a stride of
 * n_features rows per image: image b owns rows b n_features .. b n_features + n_kp[b] - 1, rows beyond are not written.  Any
 * output may be NULL.  xy float32[..][2], size, angle, response float32[..], octave int32[..], level_xy int32[..][2], cs
 * double[..][2], desc uint8[..][32].
 * LEVELS (ba_orb_levels, L = n_levels): s_0 = 1, s_l = s_(l-1) * scale_factor (repeated multiplication); w_l = rint(W / s_l),
 *   h_l = rint(H / s_l), fp64 division, rint half-to-even.  Quotas: f = 1.0 / scale_factor, p = f^L by repeated multiplication,
 *   d = n_features * (1 - f) / (1 - p); for l < L - 1: n_l = min(rint(d), n_features - sum of the quotas below l), d = d * f;
 *   n_(L-1) = n_features - sum; L = 1: n_0 = n_features.  The quotas sum to n_features for every input (the min binds only for a
 *   small n_features, where the roundings alone would add up to more), so n_kp[b] <= n_features.  A level with w_l <= 2 edge or h_l <= 2 edge has no interior and gives no keypoint (and none above it is built).
 * PYRAMID: level l from level l - 1 by fixed-point bilinear interpolation: ratio = (double)w_(l-1) / (double)w_l, sx = (x + 0.5) *
 *   ratio - 0.5 (each operation rounded), x0 = floor(sx), fx = sx - x0, x1 = x0 + 1, both clamped to [0, w_(l-1) - 1], fx = 0 if x0
 *   was clamped; a1 = rint(fx * 2048), a0 = 2048 - a1; rows likewise; pixel = (sum of the four a_y a_x I + (1 << 21)) >> 22.
 * FAST-9: the radius-3 ring in the order (0,-3) (1,-3) (2,-2) (3,-1) (3,0) (3,1) (2,2) (1,3) (0,3) (-1,3) (-2,2) (-3,1) (-3,0)
 *   (-3,-1) (-2,-2) (-1,-3); score = max over the 16 arcs of 9 contiguous ring pixels of max(min(ring - v), min(v - ring)); a
 *   corner iff score > fast_threshold; it survives iff its score is strictly greater than that of each of its 8 neighbours
 *   (non-corners count 0).  Candidates: survivors with edge <= x < w_l - edge, edge <= y < h_l - edge (neighbours outside
 *   still suppress).
 * STAGE 1, per image and level: of more than 2 n_l candidates the first 2 n_l under (score descending, raster index y w_l + x
 *   ascending).
 * HARRIS at each kept corner, over the offsets -3 .. 3 in x and y: Ix = 2 (I(x+1,y) - I(x-1,y)) + (I(x+1,y-1) - I(x-1,y-1)) +
 *   (I(x+1,y+1) - I(x-1,y+1)), Iy likewise; a = sum Ix^2, b = sum Iy^2, c = sum Ix Iy; Hs = 25 (a b - c^2) - (a + b)^2 in int64
 *   (k = 0.04 without rounding).
 * STAGE 2: the first n_l under (Hs descending, raster index ascending); output order: level ascending, then that order.
 *   response = (float)(((double)Hs / 25.0) / 2598919616160000.0)   (7140^4).
 * ORIENTATION on the unblurred level image over the circular patch of half-widths umax[|v|] = 15 15 15 15 14 14 14 13 13 12 11
 *   10 9 8 6 3 (|v| = 0 .. 15): m10 = sum u I, m01 = sum v I (integers); angle = atan2(m01, m10) in degrees in [0, 360), float32
 *   (the one output not defined to the bit: it goes through atan2); r = sqrt((double)(m10^2 + m01^2)), c = m10 / r, s = m01 / r,
 *   (c, s) = (1, 0) when both moments are 0; cs returns (c, s).
 * BLUR: separable, integer weights 18 34 49 54 49 34 18 (sum 256): the row pass keeps the exact 16-bit sum, the column pass
 *   gives (sum g t + 32768) >> 16.  With edge_threshold >= 25 no value within 3 pixels of a border is read.
 * DESCRIPTOR: pattern row i = (x1, y1, x2, y2); each point maps to u = rint(px c - py s), v = rint(px s + py c) (fp64, products and
 *   sums rounded separately, rint half-to-even); bit i % 8 of byte i / 8 = B(x + u1, y + v1) < B(x + u2, y + v2), B the blurred
 *   level image.
 * OUTPUTS: xy = (float)((double)x_l * s_l) and likewise y; size = (float)(31.0 * s_l); octave = l; level_xy = (x_l, y_l).
 * An image too small to have an interior is no error: it returns zero keypoints.  Two calls give bit-equal outputs.
 * BA_ERR_INVALID, naming the field: scale_factor not in (1, 2], n_features < 1 or > 65536, n_levels outside 1 .. 16,
 * edge_threshold < 25, fast_threshold outside 1 .. 254; images NULL with n_images > 0; height or width not positive; a pattern
 * coordinate outside -15 .. 15; n_images < 0; a batch beyond the cap: n_images > 1024, height * width > 2^26, or n_images *
 * height * width > 2^28.  A refused call leaves the handle usable.
 * Not offered: cv2's learned pattern, WTA_K 3 / 4, the FAST score type, firstLevel, masks, images of different sizes in one
 * call, a quadtree distribution of keypoints, colour conversion. */
typedef struct ba_orb_options {
  double  scale_factor;    /* > 1, <= 2; default 1.2 */
  int32_t n_features;      /* 1 .. 65536; default 3000 */
  int32_t n_levels;        /* 1 .. 16; default 8 */
  int32_t edge_threshold;  /* >= 25; default 31 */
  int32_t fast_threshold;  /* 1 .. 254; default 20 */
} ba_orb_options;          /* 24 bytes */
int ba_default_orb_options(ba_orb_options* opts);    /* 1.2, 3000, 8, 31, 20 */
/* The default test pattern, int8[256][4] = (x1, y1, x2, y2): BRIEF's "G II" sampling within +-13 (csrc/ba_orb.hpp).  Host only. */
int ba_orb_default_pattern(int8_t* pattern);
/* The level sizes, scales and quotas of the definition above, n_levels entries each; any output may be NULL.  Host only. */
int ba_orb_levels(const ba_orb_options* opts, int32_t height, int32_t width, int32_t* level_w, int32_t* level_h,
                  double* level_scale, int32_t* level_quota);
int ba_orb_extract(ba_handle* h, int32_t n_images, int32_t height, int32_t width, const uint8_t* images, const int8_t* pattern,
                   const ba_orb_options* opts, int32_t* n_kp, float* xy, float* size, float* angle, float* response,
                   int32_t* octave, int32_t* level_xy, double* cs, uint8_t* desc);
/* Measurement hook: enable = 1 makes every later ba_orb_extract on the handle record events around its stages on the stream,
 * enable = 0 stops that, enable = -1 leaves the switch as it is; ms (may be NULL) receives the BA_ORB_STAGES stage times of the last timed call that reached the
 * device, in milliseconds: upload, pyramid, FAST, stage-1 selection, Harris and ranking, blur, orientation and descriptors,
 * download.  Results do not depend on it. */
enum { BA_ORB_STAGES = 8 };
int ba_orb_stage_times(ba_handle* h, int32_t enable, double* ms);
/* Pyramidal Lucas-Kanade (KLT) point tracking: known points of image a are followed into image b without detecting or matching
 * anything -- what a visual-odometry front end does between keyframes (cv2.calcOpticalFlowPyrLK, VINS, SVO, OpenVINS; no
 * reference counterpart: its pipeline extracts and matches every frame), and, started at a matched keypoint (`guess`), the
 * refinement of an ORB match to a fraction of a pixel.  The results feed pts1 / pts2 of ba_relative_pose, ba_homography and
 * ba_fundamental, edge_a / edge_b of ba_build_tracks and uv of ba_set_problem.  This is LUCAS-KANADE BY THE DEFINITION BELOW, NOT
 * cv2's output; the defaults are cv2's (21 x 21 window, maxLevel 3, criteria (30, 0.01), minEigThreshold 1e-4) and one rule
 * differs on purpose: a point must lie INSIDE the image, 0 <= x <= w - 1, at every level it is iterated on, where cv2 lets the
 * window's corner leave the image by a window.  Sums are integers; everything else is fp64 with every operation rounded on its
 * own, so the definition decides every case.  Needs no problem; a resident problem is not touched; device memory is the scratch
 * arena's.
 * images uint8[n_images][height][width], row-major and contiguous, one common size.  Pair k = (image a, image b) = pairs[k] owns
 * the points pt_off[k] .. pt_off[k + 1] - 1; prev float32[.][2] are pixels (x, y) of image a, guess (or NULL: prev) the starts in
 * image b.  Outputs (any may be NULL): next float32[.][2], status uint8[.] (ba_klt_status), err float32[.], fb_err float32[.].
 * LEVELS (ba_klt_levels): n = 2 half_window + 1; w_0 = W, h_0 = H; level l + 1 exists while l < max_level and min((w_l + 1) / 2,
 *   (h_l + 1) / 2) >= n (integer division) and has that size; L is the top level.
 * PYRAMID, once for every image a pair with points names: P_(l+1)(x, y) = (sum over i, j = -2 .. 2 of g_i g_j P_l(r(2x + j),
 *   r(2y + i)) + 128) >> 8, g = 1 4 6 4 1; r reflects without repeating the border: -1 -> 1, -2 -> 2, n -> n - 2, n + 1 -> n - 3.
 * GRADIENTS of a level, integer Scharr, not normalised: Ix = 3 (P(x+1,y-1) - P(x-1,y-1)) + 10 (P(x+1,y) - P(x-1,y)) + 3 (P(x+1,y+1)
 *   - P(x-1,y+1)), Iy its transpose; coordinates clamped to the image.
 * WINDOW SAMPLE S(A, c, shift) of a level array A (P, Ix or Iy) at the top-left corner c (fp64): ix = floor(c.x), a = c.x - ix, rows
 *   likewise iy, b; w00 = rint((1 - a) * (1 - b) * 16384), w01 = rint(a * (1 - b) * 16384), w10 = rint((1 - a) * b * 16384), w11 =
 *   16384 - w00 - w01 - w10 (rint half to even, every product rounded); element (i, j), i, j = 0 .. n - 1, is (w00 A(ix+j, iy+i) +
 *   w01 A(ix+j+1, iy+i) + w10 A(ix+j, iy+i+1) + w11 A(ix+j+1, iy+i+1) + (1 << (shift - 1))) >> shift, an arithmetic shift, every
 *   coordinate clamped to the image.
 * PER POINT: p = prev widened to fp64.  !(0 <= p.x && p.x <= W - 1 && 0 <= p.y && p.y <= H - 1) (so a NaN too) is OUT with
 *   next = prev.  q = (guess or p) / 2^L.  For l = L .. 0:
 *   1. c = p / 2^l - half_window; T = S(P_a, c, 9) (the intensity times 32), Gx = S(Ix_a, c, 14), Gy = S(Iy_a, c, 14); A11 = sum Gx^2,
 *      A12 = sum Gx Gy, A22 = sum Gy^2 exact in int64, then fp64; D = A11 * A22 - A12 * A12; e = (A11 + A22 - sqrt((A11 - A22) *
 *      (A11 - A22) + 4 * (A12 * A12))) / (2 * n * n) / 1048576.  If !(D > 0) or e < min_eig: at l = 0 the status is FLAT with next =
 *      (float)q; at l > 0 the level is skipped, q <- 2 q.
 *   2. For it = 0 .. max_iters - 1: if q is not inside [0, w_l - 1] x [0, h_l - 1] the level ends, at l = 0 with status OUT;
 *      d = S(P_b, q - half_window, 9) - T; b1 = sum d Gx, b2 = sum d Gy exact in int64; delta = ((A12 * b2 - A22 * b1) / D,
 *      (A12 * b1 - A11 * b2) / D); q <- q + delta; stop if delta.x^2 + delta.y^2 <= eps^2; if it > 0, |delta.x + prevdelta.x| < 0.01
 *      and |delta.y + prevdelta.y| < 0.01 (an oscillation): q <- q - 0.5 delta and stop.
 *   3. At l > 0: q <- 2 q.
 *   At the end, status still OK: q outside the level-0 image is OUT; otherwise err = (float)(sum |S(P_b, q - half_window, 9) - T| /
 *   (32.0 * n * n)), T of level 0.  next = (float)q for every status but an OUT start.  err is NaN unless the status is OK or
 *   FB_FAIL.
 * FORWARD-BACKWARD CHECK (fb_max_px > 0): every OK point is tracked back from image b to image a from (double)next with no guess
 *   -- exactly what a second call with the roles swapped returns; fb_err = (float)sqrt(dx^2 + dy^2) of that result against prev;
 *   the status becomes FB_FAIL when the backward status is not OK or the fp64 distance exceeds fb_max_px.  fb_err is NaN where
 *   the backward pass did not run or did not end OK.
 * n_pairs = 0 or no points is a no-op.  Two calls give bit-equal outputs.
 * BA_ERR_INVALID, naming the field: half_window outside 1 .. 15, max_level outside 0 .. 8, max_iters outside 1 .. 100, eps or
 * min_eig negative or NaN, fb_max_px NaN; height or width not positive or min(W, H) < n; n_images outside 0 .. 1024, height *
 * width > 2^26 or n_images * height * width > 2^28 (ORB's caps); n_pairs outside 0 .. 65535; pt_off[0] != 0 or a decreasing
 * pt_off; more than 2^24 points; an image index out of range; images or prev NULL when there are points.  A refused call leaves
 * the handle usable.
 * Not offered: affine or illumination-compensating LK, rectangular windows, OPTFLOW_LK_GET_MIN_EIGENVALS as the error measure,
 * detection of new corners to track (ORB's keypoints are the corners), images of different sizes in one call, more than one
 * rank, a helper that turns tracks over a sequence into ba_build_tracks edges. */
typedef struct ba_klt_options {
  int32_t half_window;     /* 1 .. 15: the window is n x n, n = 2 half_window + 1; default 10 */
  int32_t max_level;       /* 0 .. 8: the most pyramid levels above the image; default 3 */
  int32_t max_iters;       /* 1 .. 100 iterations per level; default 30 */
  int32_t reserved;        /* 0 */
  double  eps;             /* >= 0: an iteration that moves by at most eps ends the level; default 0.01 */
  double  min_eig;         /* >= 0: the smallest normalised eigenvalue a level is tracked on; default 1e-4 */
  double  fb_max_px;       /* > 0: forward-backward check with this bound in pixels; default 0 (off) */
} ba_klt_options;          /* 40 bytes */
enum ba_klt_status { BA_KLT_OK = 0, BA_KLT_OUT = 1, BA_KLT_FLAT = 2, BA_KLT_FB_FAIL = 3 };
int ba_default_klt_options(ba_klt_options* opts);    /* 10, 3, 30, 0.01, 1e-4, 0 */
/* The levels of the definition above: n_levels = L + 1 and that many sizes; any output may be NULL (level_w, level_h: room for
 * 9).  Checks every option as ba_track_klt does.  Host only. */
int ba_klt_levels(const ba_klt_options* opts, int32_t height, int32_t width, int32_t* n_levels, int32_t* level_w, int32_t* level_h);
int ba_track_klt(ba_handle* h, int32_t n_images, int32_t height, int32_t width, const uint8_t* images, int32_t n_pairs,
                 const int32_t* pairs, const int64_t* pt_off, const float* prev, const float* guess, const ba_klt_options* opts,
                 float* next, uint8_t* status, float* err, float* fb_err);
/* Measurement hook, as ba_orb_stage_times: enable = 1 makes every later ba_track_klt on the handle record events around its
 * stages on the stream, 0 stops that, -1 leaves the switch as it is; ms (may be NULL) receives the BA_KLT_STAGES stage times of the
 * last timed call that reached the device, in milliseconds: upload, pyramid, tracking, download.  Results do not depend on it. */
enum { BA_KLT_STAGES = 4 };
int ba_klt_stage_times(ba_handle* h, int32_t enable, double* ms);
/* Similarity transform of the reconstruction and robust alignment to reference positions: the step after an adjustment that
 * moves the result into the frame its user needs (georegistration onto GPS / surveyed camera positions or ground-control
 * points -- COLMAP's model_aligner; the comparison of two gauge-free solves; re-centring / re-scaling).  No reference
 * counterpart.  Conventions: X' = s R X + t, R row-major 3x3, s > 0.  A world-to-camera pose (R_c, t_c) becomes
 * R_c' = R_c R^T, t_c' = s t_c - R_c' t: camera-frame coordinates are s times the old ones and both camera models divide by
 * depth, so every residual is unchanged and f, k1, k2 / K4 are not touched.  rvec' is the log map of R_c R^T through the unit
 * quaternion (Shepperd's choice of the largest of trace and diagonal entries, w >= 0, theta = 2 atan2(|v|, w)), exact to
 * rounding at every angle from 0 to pi.
 * Precision: fp64 in a far-away frame costs residual precision (|t| = 5e6 at s = 1 moves residuals by ~3e-7 px, |t| <= 100 by
 * ~2e-12 px): subtract a local origin from UTM-like references.
 * ba_transform applies the similarity to EVERY point and camera of the handle's current parameters, held ones included (a
 * change of frame is not an adjustment); masks, fixed_cam and shared-intrinsics groups stay and hold the new values.  It
 * leaves the handle exactly as ba_set_params(transformed cameras, transformed points) would.  BA_ERR_STATE before
 * ba_set_problem / parameters, and (naming "priors") while ba_set_priors blocks are set: their means live in the old frame,
 * so align first and set priors afterwards.  BA_ERR_INVALID for s not finite or <= 0, max |R R^T - I| > 1e-9, det R < 0, a
 * non-finite t.  A refused call leaves the handle as found.  Multi-rank jobs: local to the rank, no collective; every rank
 * must pass the same similarity -- the replicated cameras then stay bitwise identical, the points are rank-local.  Pinned on
 * two ranks (tests/test_gpu_multirank_local.py). */
typedef struct ba_similarity { double s; double R[9]; double t[3]; } ba_similarity;

int ba_get_centres(ba_handle* h, double* centres);            /* double[Nc][3]: -R_c^T t_c of the current cameras */
int ba_transform(ba_handle* h, const ba_similarity* sim);

/* ba_align: the similarity that brings a_i = the current camera centres (where cam_ref is given), then the current points
 * (where pt_ref is given, the caller's point order) onto the reference positions b_i.  A NULL weight vector is all ones;
 * w_i = 0 means "no reference" (that row may hold NaN and enters no sum); a negative or non-finite weight is BA_ERR_INVALID.
 * Weighted Umeyama with the current weights u_i: centroids mu_a, mu_b; Sigma = sum u_i (b_i - mu_b)(a_i - mu_a)^T / W from
 * sums centred in a second pass (which also recovers what the first pass's rounding left out of mu_b); Sigma = U D V^T, R = U diag(1, 1, det U det V) V^T; s = tr(D diag(...)) / var_a (1 when
 * with_scale = 0); t = mu_b - s R mu_a.  Then `iters` rounds of u_i = w_i rho'(w_i d_i^2 / f_scale^2), d_i = |b_i - (s R a_i + t)|,
 * rho' of the solve's losses, each followed by the same closed form.  n_used = correspondences with w_i > 0; rms and max over
 * those, of the unweighted d_i at the final similarity; cam_err / pt_err = d_i, NaN without a reference.
 * status TOO_FEW: n_used < 3.  DEGENERATE: W = 0, var_a = 0, second singular value <= 1e-12 x the first (coincident or
 * collinear positions), or a non-finite sum.  In both cases the call returns BA_OK, sim is the identity, rms, max and the
 * errors are NaN and nothing is applied even with apply = 1.
 * BA_ERR_INVALID for an unknown loss, f_scale <= 0, iters < 0, both reference arrays NULL; BA_ERR_STATE as ba_transform
 * (the priors refusal only with apply = 1).  All rounds run on the device without a host synchronisation in between; the sums
 * use no atomics and a fixed order: results are bit-reproducible from call to call.  Local to the rank, no collective:
 * callers of multi-rank jobs align on camera references, which are replicated -- cam_ref alone gives every rank the same
 * similarity, and apply = 1 then moves every rank's cameras alike.  pt_ref sees the rank's own points: with apply = 1 and
 * world > 1 it is refused (BA_ERR_INVALID naming apply, pt_ref and "multi-rank", the handle left as found); estimate with
 * apply = 0 and pass every rank one similarity (ba_transform).  Pinned on two ranks (tests/test_gpu_multirank_local.py). */
enum ba_align_status { BA_ALIGN_OK = 0, BA_ALIGN_TOO_FEW = 1, BA_ALIGN_DEGENERATE = 2 };
typedef struct ba_align_options {
  int32_t loss;        /* ba_loss, ONE rho per correspondence, on its 3-D distance */
  int32_t iters;       /* IRLS re-weightings after the least-squares fit; 0 = least squares only */
  double  f_scale;     /* in the unit of the reference positions */
  int32_t with_scale;  /* 1: similarity; 0: rigid, s = 1 */
  int32_t apply;       /* 1: ba_transform(h, result) in the same call when status is OK */
} ba_align_options;
typedef struct ba_align_result {
  ba_similarity sim; double rms; double max; int32_t n_used; int32_t status;
} ba_align_result;
int ba_default_align_options(ba_align_options* o);            /* linear, 10, 1.0, 1, 0 */
int ba_align(ba_handle* h, const ba_align_options* opts,
             const double* cam_ref, const double* cam_w,      /* [Nc][3], [Nc]; either pair may be NULL */
             const double* pt_ref,  const double* pt_w,       /* [Np][3], [Np] */
             ba_align_result* out, double* cam_err, double* pt_err);   /* errors may be NULL */

/* ba_pose_graph: Sim(3) pose-graph optimisation -- the step between a loop closure and the global adjustment that spreads
 * accumulated drift over the keyframes (ORB-SLAM's OptimizeEssentialGraph, g2o's EdgeSim3).  It needs no ba_set_problem and
 * leaves a resident problem, its parameters and the trace of its last solve untouched; staging lives on the handle and is
 * reused; local to the rank, no collective.
 * Nodes  poses double[n][7] = rvec(3) | t(3) | s: the world-to-node similarity x_k = s_k R_k X + t_k, s_k > 0, R_k = exp(rvec_k).
 *        A camera of the handle is the node rvec | t | 1.
 * Edges  edge_i, edge_j int32[m], i != j, duplicates and either order allowed; meas double[m][7] = rvec_ij | t_ij | s_ij, the
 *        measured S_j o S_i^-1, i.e. x_j = s_ij R_ij x_i + t_ij (ba_relative_pose's and ba_similarity's convention); info
 *        double[m][49] row-major, symmetric, positive SEMIdefinite (a rotation-only edge is a block with zeros elsewhere), the
 *        inverse covariance of the seven residuals below; NULL = identity.
 * Residual  with s_r = s_j / s_i, R_r = R_j R_i^T, t_r = t_j - s_r R_r t_i:
 *             e = [ log(R_ij^T R_r) ; t_r - t_ij ; ln(s_r / s_ij) ]                                     (7)
 *        log = the Shepperd-quaternion log map, exact from 0 to pi.  The decoupled chart on purpose, not the Lie logarithm of
 *        Sim(3).  chi2_e = e^T info e, z_e = chi2_e / f_scale^2, cost = 0.5 f_scale^2 sum_e rho(z_e): ONE rho per edge, any of
 *        the five losses, solved by IRLS with w_e = rho'(z_e).  *_sse of the summary = sum chi2_e.
 * Local parameters of node k, d = (d_omega, d_t, d_sigma): R_k <- exp(d_omega) R_k, t_k <- t_k + d_t, s_k <- s_k exp(d_sigma); rvec_k is
 *        written back through the log map.  A_e = de/dd_i, B_e = de/dd_j analytic in fp64 (csrc/ba_posegraph.hpp).
 *        H = sum w_e [A B]^T info [A B], g = sum w_e [A B]^T info e.
 * Held   identity row / column, zero gradient, values returned bit-equal: every node marked in held uint8[n] (NULL: none), every
 *        d_sigma when with_scale = 0, every free node without an incident edge.  with_scale = 0 demands every s_k and s_ij to be
 *        exactly 1.0 and leaves them exactly 1.0.  No gauge is demanded: as in ba_solve the damping carries a free gauge.
 * LM     ba_solve's rules: damping matrix D = max(diag H, 1e-12), gain ratio against the model decrease of the damped, inexactly
 *        solved system, Nielsen's update with the floor of capped inner solves, acceptance, ftol / xtol / gtol over the free
 *        parameters only (|x| over the stored rvec | t | s of the free entries), the status codes of ba_summary.
 * Inner  PCG on the block-sparse H + lambda D, preconditioned by its 7 x 7 diagonal blocks (Cholesky per node); pcg_tol /
 *        pcg_max_iters / pcg_min_iters as in ba_options; verdicts on the device, the host looks once per batch of iterations.
 * Outputs (any may be NULL)  poses_out double[n][7]; summary; edge_chi2 / edge_weight double[m] = chi2_e and w_e at the returned
 *        poses.  n = 0 or m = 0: poses copied, zero cost, status gtol.  Every sum has a fixed order and there are no
 *        floating-point atomics: two calls give the same bits.
 * BA_ERR_INVALID, naming the field: negative n or m, edge_i == edge_j, an index outside 0 .. n-1, a non-finite entry, s <= 0,
 *        |rvec| > pi + 1e-9, info not symmetric to 1e-12 relative or not positive semidefinite, an unknown loss, f_scale <= 0,
 *        negative counts or tolerances, the with_scale = 0 rule.  A refused call leaves the handle as found.
 * BA_ERR_NUMERIC: a non-finite initial cost, or a damped diagonal block that is not positive definite. */
typedef struct ba_posegraph_options {
  int32_t loss;            /* ba_loss; default linear */
  int32_t max_iters;       /* 50 */
  double f_scale;          /* 1.0, in the unit of sqrt(chi2) */
  double ftol, xtol, gtol; /* 1e-5, 1e-5, 1e-8 (ba_default_options) */
  double initial_lambda;   /* 1e-4 */
  double pcg_tol;          /* 0.1 */
  int32_t pcg_max_iters;   /* 200 */
  int32_t pcg_min_iters;   /* 1 */
  int32_t with_scale;      /* 1: Sim(3); 0: SE(3), every s stays exactly 1 */
  int32_t reserved0;       /* must be 0 */
} ba_posegraph_options;
int ba_default_posegraph_options(ba_posegraph_options* o);
int ba_pose_graph(ba_handle* h, int32_t n, const double* poses, int32_t m, const int32_t* edge_i, const int32_t* edge_j,
                  const double* meas, const double* info, const uint8_t* held, const ba_posegraph_options* opts,
                  double* poses_out, ba_summary* summary, double* edge_chi2, double* edge_weight);
/* The per-iteration records of the last ba_pose_graph on this handle (as ba_get_trace for ba_solve). */
int ba_pose_graph_trace(ba_handle* h, ba_iter_record* out, int32_t capacity, int32_t* n);
/* The inspection entry (as ba_linearize / ba_schur_system for the solve): at the given poses, the residuals e double[m][7],
 * the Jacobians A, B double[m][49] row-major, the dense row-major (7n)^2 H + lambda D with the held rows in it (identity) and
 * g double[7n]; opts gives loss, f_scale and with_scale.  Any output may be NULL.  Refuses 7 n > 4096 (BA_ERR_INVALID, naming n). */
int ba_pose_graph_system(ba_handle* h, int32_t n, const double* poses, int32_t m, const int32_t* edge_i, const int32_t* edge_j,
                         const double* meas, const double* info, const uint8_t* held, const ba_posegraph_options* opts,
                         double lambda, double* e, double* A, double* B, double* H, double* g);
/* Place recognition: which earlier image does a new one revisit (the loop_i, loop_j ba_pose_graph takes as given), and which
 * image pairs of a collection are worth matching at all.  A binary bag of words as in DBoW2 (ORB-SLAM's loop detection) and
 * COLMAP's vocabulary-tree matcher: a vocabulary tree over the descriptors, one sparse vector per image, an L1 score between
 * vectors.  Three calls, none of which needs ba_set_problem or touches a resident problem; the vocabulary IS resident on the
 * handle: set by ba_vocab_train or ba_vocab_set, read by ba_bow_transform.  Local to the rank.  Everything is integer arithmetic
 * (one log on the host for the idf weights), so results are bit-reproducible and independent of how the library tiles the work.
 * Descriptor sets are given as in ba_match_descriptors: desc uint8[set_off[n_sets]][desc_bytes], desc_bytes a multiple of 8 in
 * 8 .. 64, n_sets in 0 .. 65535; one set is one image.
 *
 * ba_vocab_train: hierarchical k-majority over all rows (rows < 2^24).  The root (node 0, depth 0, descriptor all zero) holds
 * every row.  A node at depth d < levels with m >= min_split member rows is split:
 *   seeds      slot j in 0 .. branching - 1 starts from the descriptor of the member row x with the smallest key
 *              (draw(seed, d, j, x) & ~0xFFFFFF) | x, draw = ba_resect_ransac's counter-based generator (splitmix64 chained four
 *              times) with (camera, hypothesis, draw number) = (d, j, x) and x the row's index in desc.  A slot whose row an earlier
 *              slot of the node drew is void: it takes part in no assignment and stays empty.
 *   iteration  at most iters times: (1) every member goes to the slot with the smallest (Hamming distance to the slot's centre,
 *              slot) among the slots that are not void; (2) stop if no member's slot changed; (3) the centre of every non-empty
 *              slot becomes the bitwise majority of its members, bit = 1 iff 2 * count >= size (a tie is 1, DBoW2's rule); an
 *              empty slot keeps its centre.
 *   closing    members are assigned once more to the final centres; the non-empty slots become the node's children in slot order,
 *              their descriptors the centres.  With fewer than two non-empty slots the node stays a leaf.
 * Nodes with m < min_split and nodes at depth `levels` are leaves.  Nodes are numbered breadth-first by (parent, slot), so a
 * node's children are contiguous; the leaves are the WORDS, numbered in node order.  idf_q[i] = floor(ln(N / N_i) * 4096 + 0.5),
 * N = n_sets, N_i the number of sets with a row in word i (computed on the host in double; 0 where N_i = 0).
 * Outputs (any may be NULL): train_word int32[rows], the word of every row (equal to ba_bow_transform's desc_word of the same rows);
 * n_nodes, n_words.  BA_ERR_INVALID, naming the field: the set arguments as in ba_match_descriptors, rows >= 2^24, an option out
 * of range.  Cost and layout: csrc/ba_bow.hpp, DESIGN.md 4r.
 *
 * ba_vocab_size: the resident vocabulary's numbers (all 0 when there is none); branching and levels are the training options,
 * or, after ba_vocab_set, the largest n_child and the tree's depth.  ba_vocab_get: child0, n_child, word_of_node int32[n_nodes]
 * (child0 = -1, n_child = 0 at a leaf; word_of_node = -1 at an inner node), node_desc uint8[n_nodes][desc_bytes], idf_q
 * int32[n_words]; any may be NULL; BA_ERR_STATE without a vocabulary.  ba_vocab_set uploads a saved or hand-made tree; BA_ERR_INVALID
 * naming the violation unless: walking the nodes in order, the children of the inner nodes are breadth-first contiguous (child0
 * of the first inner node is 1, each next inner node's follows the previous one's children); every node but the root is the
 * child of exactly one node (the children end at n_nodes); n_child is 0 at a leaf and 2 .. 32 at an inner node; depth <= 8;
 * 0 <= idf_q <= 131071 (so that no vector entry overflows 63 bits).
 *
 * ba_bow_transform: a row descends from the root, at each inner node to the child with the smallest (Hamming distance, slot), down
 * to a leaf: its word.  Per set, with c_i the number of its rows in word i: a_i = c_i * idf_q[i] (weighting BA_BOW_TF_IDF) or
 * c_i * 4096 (BA_BOW_TF, for a vocabulary trained on one set), A = sum a_i, v_i = (a_i << 30) / A in 64-bit integer division;
 * entries with v_i = 0 are dropped and A = 0 gives an empty vector.  Outputs (any may be NULL): desc_word int32[rows]; the CSR
 * vec_off int64[n_sets + 1], vec_word (ascending within a set) and vec_val int32[], for which the caller provides `rows` entries.
 * A set's vector does not depend on the other sets of the call.  BA_ERR_STATE without a vocabulary; BA_ERR_INVALID: desc_bytes not
 * the vocabulary's, a set of more than 65536 rows, weighting not 0 / 1, the set arguments as above.
 *
 * ba_bow_score: score(q, j) = sum over the common words of min(vq_i, vd_i), an integer in 0 .. 2^30; for L1-normalised
 * non-negative vectors this equals 1 - |v_q - v_d|_1 / 2 (DBoW2's L1 score) in units of 2^-30.  Queries and database are CSRs
 * as ba_bow_transform writes them (words ascending within a vector, values >= 0 that sum to at most 2^30; otherwise BA_ERR_INVALID).
 * db_end int32[nq] or NULL: query q is scored against the database entries j < db_end[q] only (clamped to 0 .. nd; NULL: all) -- a
 * SLAM front end passes its own index minus a gap, an image list scored against itself passes q.  Outputs (any may be NULL):
 * top_idx, top_score int32[nq][top_k], top_k in 1 .. 64: the admitted entries with score > 0 ordered by (score descending, index
 * ascending), padded with -1 / 0; score int32[nq][nd], the dense matrix, 0 where not admitted.
 * Not offered: other weightings and norms (L2, chi-square, KL, dot product), DBoW2's direct index (desc_word lets a caller build
 * one), k-means++ seeding, float descriptors, DBoW2's text / binary vocabulary files, temporal consistency checks, vocabularies
 * spread over ranks. */
typedef struct ba_vocab_options {
  int32_t  branching;    /* k, 2 .. 32; default 10 */
  int32_t  levels;       /* L, 1 .. 8; default 6 */
  int32_t  iters;        /* k-majority iterations per level, >= 1; default 10 */
  int32_t  min_split;    /* fewest members a node must have to be split, >= 2; 0 (default) means 2 * branching */
  uint64_t seed;         /* seed of the row draws; default 0 */
} ba_vocab_options;      /* 24 bytes */
enum { BA_BOW_TF_IDF = 0, BA_BOW_TF = 1 };
int ba_default_vocab_options(ba_vocab_options* opts);    /* 10, 6, 10, 0, 0 */
int ba_vocab_train(ba_handle* h, int32_t desc_bytes, int32_t n_sets, const int64_t* set_off, const uint8_t* desc,
                   const ba_vocab_options* opts, int32_t* train_word, int32_t* n_nodes, int32_t* n_words);
int ba_vocab_size(ba_handle* h, int32_t* desc_bytes, int32_t* n_nodes, int32_t* n_words, int32_t* branching, int32_t* levels);
int ba_vocab_get(ba_handle* h, int32_t* child0, int32_t* n_child, uint8_t* node_desc, int32_t* word_of_node, int32_t* idf_q);
int ba_vocab_set(ba_handle* h, int32_t desc_bytes, int32_t n_nodes, const int32_t* child0, const int32_t* n_child,
                 const uint8_t* node_desc, const int32_t* idf_q);
int ba_bow_transform(ba_handle* h, int32_t desc_bytes, int32_t n_sets, const int64_t* set_off, const uint8_t* desc,
                     int32_t weighting, int32_t* desc_word, int64_t* vec_off, int32_t* vec_word, int32_t* vec_val);
int ba_bow_score(ba_handle* h, int32_t nq, const int64_t* q_off, const int32_t* q_word, const int32_t* q_val, int32_t nd,
                 const int64_t* d_off, const int32_t* d_word, const int32_t* d_val, const int32_t* db_end, int32_t top_k,
                 int32_t* top_idx, int32_t* top_score, int32_t* score);

/* Feature tracks from pairwise matches: which keypoints of which images are one 3D point.  The step between the verified
 * matches of the image pairs (ba_match_descriptors / ba_match_guided; match_inlier of ba_fundamental, ba_relative_pose,
 * ba_homography) and the (cam_idx, pt_idx, uv) lists ba_triangulate_tracks and ba_set_problem start from.  Replaces the
 * per-keyframe dict bookkeeping of the reference (src/pipeline.py, _add_new_keyframe and _add_new_keyframe_exhaustive: the
 * last_kf_obs_lookup / kf_obs_lookup parts), OpenMVG's TracksBuilder, COLMAP's correspondence graph.  Needs the handle only:
 * it neither reads nor touches a resident problem.  Local to the rank, no collective.  Integer arithmetic throughout.
 *
 * A node is a keypoint: node = kp_off[image] + keypoint, kp_off int64[n_images + 1] ascending from 0, N = kp_off[n_images]
 * < 2^31.  An edge e is one match between nodes edge_a[e] and edge_b[e]; edge_keep[e] == 0 (edge_keep may be NULL: keep all)
 * removes it, and a removed edge's ends are not examined.  A kept edge whose ends lie in one image (a == b included) is ignored
 * and counted.  Duplicates and either orientation are allowed.
 *
 * Every output but counts[6] and counts[7] is a function of the SET of kept edges: not of their order, their orientation,
 * their multiplicity, the launch grid or the order in which atomics are served (counts[6] counts edges, duplicates included).
 *   node_label[v]   the smallest node of v's connected component over the kept edges (v itself when isolated).
 *   A component of at least two nodes is a candidate track; it has a conflict when two of its nodes lie in one image.
 *     BA_TRACKS_DROP   the whole component is no track (OpenMVG's track filter).
 *     BA_TRACKS_FIRST  the smallest node of every image stays, the image's other nodes get no track.  The kept nodes are then
 *                      the track EVEN THOUGH THEY NEED NOT BE CONNECTED BY KEPT EDGES ANY MORE: the dropped node may have been
 *                      the only link between them.
 *   A candidate with fewer than min_length kept nodes is no track.
 *   Tracks are numbered by ascending label (the label is always a member: a track's first member); members are listed by
 *   ascending node, i.e. by ascending image.  track_off int64[tracks + 1] / track_node int32[members] are the CSR (the caller
 *   provides N / 2 + 2 and N entries).  node_track[v] = the track of v or -1.  node_status[v]: enum ba_trackbuild_status --
 *   IN_TRACK; ISOLATED (no kept edge to another image); CONFLICT (DROP: every node of a conflicting component; FIRST: the nodes
 *   that were not the smallest of their image); SHORT (a node kept by the conflict policy whose component has fewer than
 *   min_length kept nodes).
 *   counts int64[8]: tracks, track members, components of at least two nodes, components with a conflict, nodes dropped for
 *   a conflict, components dropped as short, same-image edges ignored, hook rounds run.  The hook-round count is a diagnostic:
 *   it is the ONE value that may differ between two calls on the same input.
 * max_rounds: the components come from rounds of (link roots, flatten).  A lane of the linking kernel leaves only when the two
 * ends of its edge have one root or its own link went in, so after the first round every edge is inside one tree and the second
 * finds nothing to link: two rounds, in whatever order atomics are served.  0 means the library's cap, ceil(log2 max(N, 2)) + 2,
 * a net well above that.  Hitting the cap returns BA_ERR_INTERNAL naming max_rounds, outputs unspecified.
 * BA_ERR_INVALID, naming the argument: a NULL pointer other than edge_keep; n_images < 0; kp_off not starting at 0 or
 * decreasing; N >= 2^31; n_edges < 0 or above 2^36; min_length < 2; conflict not 0 / 1; max_rounds < 0; a kept edge with an end
 * outside [0, N) -- found on the device, the message names the smallest such edge.  n_edges == 0 and N == 0 are valid: no tracks.
 * Not offered: splitting a conflicting component by cutting weak edges, a cap on track length, per-edge weights, tracks
 * across ranks, a persistent incrementally updated forest (the call is stateless: an existing map passes its tracks as chain
 * edges next to the new matches).  Kernels, cost and layout: csrc/ba_trackbuild.hpp, DESIGN.md 4v. */
typedef struct ba_trackbuild_options {
  int32_t min_length;   /* 2: fewest members (= distinct images) of a track */
  int32_t conflict;     /* 0 = BA_TRACKS_DROP, 1 = BA_TRACKS_FIRST */
  int32_t max_rounds;   /* 0 = the library's cap */
  int32_t reserved;
} ba_trackbuild_options;   /* 16 bytes */
enum { BA_TRACKS_DROP = 0, BA_TRACKS_FIRST = 1 };
enum ba_trackbuild_status { BA_TRACKBUILD_IN_TRACK = 0, BA_TRACKBUILD_ISOLATED = 1, BA_TRACKBUILD_CONFLICT = 2, BA_TRACKBUILD_SHORT = 3 };
int ba_default_trackbuild_options(ba_trackbuild_options* opts);    /* 2, BA_TRACKS_DROP, 0, 0 */
int ba_build_tracks(ba_handle* h, int32_t n_images, const int64_t* kp_off, int64_t n_edges, const int32_t* edge_a,
                    const int32_t* edge_b, const uint8_t* edge_keep, const ba_trackbuild_options* opts, int32_t* node_label,
                    int32_t* node_track, uint8_t* node_status, int64_t* track_off, int32_t* track_node, int64_t* counts);

/* Copies up to `capacity` records of the last ba_solve into out (may be NULL to ask for the count only);
 * *n = number of LM iterations recorded. */
int ba_get_trace(ba_handle* h, ba_iter_record* out, int32_t capacity, int32_t* n);

/* Device / handle -------------------------------------------------------------------- */
int ba_device_count(int* n);
int ba_create(int device_id, ba_handle** out);   /* replaces BundleAdjuster.__init__ state, :20-22 */
int ba_destroy(ba_handle* h);
int ba_synchronize(ba_handle* h);

/* Multi-GPU: one process per GPU; rank 0 makes the id, the host side ships the 128 bytes
 * to the other ranks (bench.py uses torch.distributed's store), every rank calls init.
 * With world == 1 nothing is loaded.  No reference counterpart. */
int ba_comm_unique_id(void* id128);
int ba_comm_init(ba_handle* h, int rank, int world, const void* id128);

/* Problem upload: replaces the dict/list gather of _gather_local_data (:195-218) and the
 * 0/1 jac_sparsity of _prepare_sparsity_matrix (:74-120) -- the library derives its own
 * camera-sorted and point-sorted orderings once.  In a multi-rank job each rank passes
 * ITS shard of points/observations (pt_idx local to the shard) and ALL cameras. */
int ba_set_problem(ba_handle* h, int32_t n_cams, int32_t n_pts, int64_t n_obs,
                   const int32_t* cam_idx, const int32_t* pt_idx, const double* uv,
                   const double K4[4], int32_t fixed_cam);
/* Held parameters: unknowns that keep their values through ba_solve / ba_solve_bal (Ceres' constant parameter blocks and
 * subset parameterisations, g2o's setFixed; no reference counterpart beyond fixed_cam, src/bundle_adjuster.py:141-143).
 *   cam_held uint16[Nc] or NULL: a bit set over the camera's block columns -- bits 0-2 rvec, 3-5 t (the caller's additive
 *            coordinates, as the columns of ba_linearize's blocks), and under the BAL model bit 6 f, 7 k1, 8 k2
 *   pt_held  uint8[Np]  or NULL: nonzero = all three coordinates of the point are held
 * A held parameter ends bit-equal to its input; it has zero rows and columns in Hcc | bc (and Hpp = bp = 0 for a held point)
 * as reported by ba_linearize*, identity ones in the damped system, ba_schur_system's S and the preconditioner, and a zero
 * right-hand side (ba_schur_system's g) and step.  A held point keeps its observations: they enter the cost and the cameras'
 * blocks.  The stopping tests see the free parameters only (gtol: max |g| over free entries; xtol: |x| and |dx| over free
 * entries).  fixed_cam holds its camera in addition to the masks; its block, unlike the masks' entries, keeps its share of
 * xtol's |x| (with or without masks: |x| of a solve with fixed_cam alone counts every camera).  The masks belong to the
 * handle: they survive ba_set_params and repeated solves; ba_set_problem clears them, and so does ba_set_held(h, NULL, NULL).
 * Bits 9-15 are refused here; bits 6-8 by the pinhole solve / linearisation that meets them (BA_ERR_INVALID).
 * Multi-rank jobs: cam_held covers ALL cameras and must be the same on every rank (the caller's obligation); pt_held is
 * per shard, in the shard's local point order. */
int ba_set_held(ba_handle* h, const uint16_t* cam_held, const uint8_t* pt_held);
/* Shared intrinsics: cameras that are ONE physical camera (Ceres / COLMAP / g2o: the same intrinsics block passed to many
 * observations; no reference counterpart).  BAL solves only.
 *   cam_group int32[Nc] or NULL: cameras with the same label >= 0 share ONE f, k1, k2; -1 = the camera's own.
 * Labels are arbitrary non-negative int32; a label below -1 is refused (BA_ERR_INVALID, naming the camera).  A group of one
 * member is an ungrouped camera.  The groups belong to the handle like the held masks and priors: they survive ba_set_params
 * and repeated solves; ba_set_problem clears them, and so does a NULL argument or an assignment in which no group has two
 * members.  BA_STAT_SHARED_GROUPS = groups with two or more members.
 * ba_solve_bal then adjusts y = (6 pose entries per camera, 3 entries per group, 3 per ungrouped camera) with x = E y, E
 * replicating a group's entries into every member: the damped reduced system is (E^T S E) y = E^T g, the Marquardt diagonal of
 * a shared entry the sum of the members' (floored per camera), the preconditioner a member's 6 x 6 pose block and the SUM of
 * the members' 3 x 3 intrinsics blocks (no coupling), and gain ratio, gtol, xtol and the trace's step_norm are those of the y
 * problem (a shared entry counts once).  On entry ba_solve_bal refuses with BA_ERR_INVALID, naming the first offending camera:
 * members whose intr rows are not bit-equal; members whose held bits 6-8 differ; fixed_cam inside a group (fixed_cam holds the
 * whole 9-parameter block, which contradicts a free shared block: hold the camera's pose with ba_set_held bits 0-5 instead).
 * On exit the members' intr rows are bit-equal.  nb = 9 priors on members simply add: the sum of the members' blocks is the
 * group's prior.
 * With groups set: ba_solve and ba_linearize (pinhole) refuse, as they do for held bits 6-8; ba_covariance refuses by name
 * (covariances of shared intrinsics are not offered); ba_linearize_bal, ba_schur_system, ba_residuals_bal and ba_prior_cost
 * keep reporting per-camera quantities -- E^T of them (the sum over a group's members) is the caller's.
 * Multi-rank jobs: cam_group covers ALL cameras and must be the same on every rank, like cam_held; the group sums run on the
 * all-reduced product in a fixed order, so every rank computes the same bits.  The in-kernel IPC exchange (BA_IPC=1) is not
 * used by such solves: the base transport serves them and BA_STAT_IPC_EXCHANGES stays 0. */
int ba_set_shared_intrinsics(ba_handle* h, const int32_t* cam_group);
/* Gaussian priors: soft knowledge of camera blocks and points (Ceres residual blocks on one parameter block, g2o unary
 * edges, GTSAM PriorFactor, ground-control points; no reference counterpart).  The objective ba_solve / ba_solve_bal
 * minimise becomes
 *   cost(x) = 0.5 sum_i f_scale^2 rho((r_i / f_scale)^2)  +  0.5 sum_c (x_c - mu_c)^T L_c (x_c - mu_c)  +  0.5 sum_p (X_p - mu_p)^T L_p (X_p - mu_p)
 * with x_c the caller's additive coordinates rvec | t (| f k1 k2), the ones ba_linearize, ba_set_held and ba_covariance
 * speak.  L is an information matrix (inverse covariance): symmetric positive SEMIdefinite, so a prior on t alone is a block
 * with zeros elsewhere.  A block of zeros is "no prior"; its mean is not read.  The robust loss is never applied to the
 * prior terms.
 *   nb        6 (rvec | t) or 9 (rvec | t | f k1 k2: BAL solves only)
 *   cam_mean  double[Nc][nb]             cam_info double[Nc][nb (nb + 1) / 2]  packed upper triangles, Hcc's order
 *   pt_mean   double[Np][3]              pt_info  double[Np][6]  Hpp's order; both in the caller's point order
 * Either pair may be NULL.  The priors belong to the handle like the held masks: they survive ba_set_params and repeated
 * solves; ba_set_problem clears them, and so does ba_set_priors with both pairs NULL or with every block zero.
 * Refused with BA_ERR_INVALID, naming the first offending camera or point: a non-finite entry in a block, or in the mean of a
 * non-zero block; a block that is not positive semidefinite (smallest eigenvalue below -1e-12 times the largest); nb other
 * than 6 / 9.  nb = 9 priors are refused by the pinhole solve / linearisation that meets them; nb = 6 priors on a BAL solve
 * are fine (the intrinsics get none).
 * With priors set: ba_linearize*, ba_schur_system and ba_covariance report the system the solve uses -- Hcc += L_c,
 * bc += L_c (x_c - mu_c), Hpp += L_p, bp += L_p (X_p - mu_p), ahead of the held zeroing and of the damping (the Marquardt
 * diagonal, the Schur-Jacobi blocks and the gain ratio's model all see H + L); a held parameter's prior only adds its
 * constant to the cost, the fixed camera's block stays zero.  ba_covariance: Sigma = (H_free + L_free)^-1 -- a prior can
 * fix the gauge that the observations leave free; a free point seen from one camera only is an ordinary point once it
 * carries a non-zero prior.  ba_summary.initial_cost / final_cost, the trace's cost / cost_trial and the ftol test are the
 * TOTAL objective; initial_sse / final_sse / sse_trial and everything ba_residuals* returns stay reprojection-only.  gtol
 * sees the total gradient; xtol is untouched.  A window-sized problem with priors takes the multi-kernel path (see
 * ba_options.small_solver): the window kernels do not know priors.
 * Multi-rank jobs: the camera arrays cover ALL cameras and must be the same on every rank (counted once); the point arrays
 * are per shard, in the shard's local point order.
 * Not offered: information that couples two cameras or a camera and a point (a dense marginalisation prior), and a prior on
 * the camera CENTRE -R^T t (a nonlinear factor of its own, not a quadratic in these coordinates). */
int ba_set_priors(ba_handle* h, int32_t nb, const double* cam_mean, const double* cam_info, const double* pt_mean,
                  const double* pt_info);
/* The two prior sums of the objective at the current parameters (intr: (f, k1, k2)[Nc] for nb = 9 priors, else NULL; either
 * output may be NULL).  Multi-rank: the camera sum as on one rank, the point sum of the calling rank's shard. */
int ba_prior_cost(ba_handle* h, const double* intr, double* cam_cost, double* pt_cost);
int ba_set_params(ba_handle* h, const double* cams, const double* pts);
int ba_get_params(ba_handle* h, double* cams, double* pts);
/* 3x3 rotation matrices of the current cameras, double[Nc][9] row-major: the
 * cv2.Rodrigues(rvec) of _update_map (:235-236). */
int ba_get_rotations(ba_handle* h, double* R);

/* Multi-rank write-back: after ba_solve every rank holds its own shard's points; this fills
 * pts_all double[n_total][3] with the points of ALL shards on every rank (the calling rank's
 * shard sits at [p_begin, p_begin + n_pts)); a collective, call it on every rank.  With one rank
 * it is ba_get_params' point copy.  Lets an SPMD BundleAdjuster.run finish _update_map (:239-240)
 * on every rank. */
int ba_allgather_points(ba_handle* h, int64_t p_begin, int64_t n_total, double* pts_all);

/* K1: residual vector in the caller's observation order == _cost_function (:24-72).
 * r may be NULL.  sse = sum r^2 (":165"), cost = 0.5 sum rho(r^2) for `loss`. */
int ba_residuals(ba_handle* h, int32_t loss, double f_scale, double* r, double* sse, double* cost);

/* K1 for the BAL 9-parameter camera [rvec | t | f k1 k2] (grail.cs.washington.edu/projects/bal; SURVEY.md 8f row 2;
 * the reference has no counterpart: its only camera is cv2.projectPoints(..., distCoeffs=None), :67): cameras (rvec, t)
 * and points as set by ba_set_params, intr double[Nc][3] = (f, k1, k2) per camera, pixels relative to the image
 * centre, the camera looking down -z.  Same row order and outputs as ba_residuals. */
int ba_residuals_bal(ba_handle* h, const double* intr, int32_t loss, double f_scale, double* r, double* sse, double* cost);

/* K2 for the BAL camera (parity hook, like ba_linearize): block normal equations at the current parameters with the 2x9
 * camera block [d/d rvec (additive) | d/d t | d/d f | d/d k1 | d/d k2].  Outputs (any may be NULL):
 *   Hcc double[Nc][45]  upper triangle of Jc^T w Jc, row-major (00 01 .. 08 11 .. 88);  bc double[Nc][9]  Jc^T w r
 *   Hpp double[Np][6], bp double[Np][3] as ba_linearize.  The fixed camera's blocks are zero.  In a multi-rank job Hcc | bc
 *   are all-reduced like ba_linearize's, Hpp | bp are the calling rank's shard. */
int ba_linearize_bal(ba_handle* h, const double* intr, int32_t loss, double f_scale, double* Hcc, double* bc, double* Hpp,
                     double* bp);

/* The solve step for the BAL 9-parameter camera: the SAME kernels and host loop as ba_solve, instantiated for the second
 * camera model of csrc/ba_models.hpp (BalCam; kernels in csrc/ba_kernels.hpp are templates over the model): LM + Schur
 * complement + matrix-free PCG with 9x9 camera blocks, device-side PCG / LM verdicts, speculated linearisation;
 * preconditioner BA_PRECOND_JACOBI (damped 9x9 camera blocks) or Schur-Jacobi (their Schur complements: the default).
 * Same damping / gain-ratio / stopping rules, options, summary and trace as ba_solve; jacobian_precision is honoured (1 = BASELINE config 5's "fp32 Jacobian + fp64 solve"); small_solver is ignored
 * (the window solver is built for the reference's pinhole only).  Multi-rank jobs are supported exactly as in ba_solve
 * (landmark shards, the same all-reduces; fold sizes follow the 9-parameter blocks).  Cameras (rvec, t) and points are the
 * handle's (ba_set_params before, ba_get_params after); intr double[Nc][3] = (f, k1, k2) per camera is read AND updated.
 * fixed_cam of ba_set_problem is honoured (-1: no camera held; the damping carries the gauge), and so are the masks of
 * ba_set_held, bits 6-8 included: a held intrinsic comes back in intr unchanged, bit for bit; and the groups of
 * ba_set_shared_intrinsics (see there for what is refused on entry). */
int ba_solve_bal(ba_handle* h, double* intr, const ba_options* opts, ba_summary* sum);

/* K2/K3: linearise at the current parameters.  Outputs (any may be NULL):
 *   Hcc double[Nc][21]  upper triangle of Jc^T w Jc, row-major (00 01 .. 05 11 .. 55)
 *   bc  double[Nc][6]   Jc^T w r
 *   Hpp double[Np][6]   upper triangle of Jp^T w Jp (00 01 02 11 12 22)
 *   bp  double[Np][3]   Jp^T w r
 * The fixed camera's blocks are zero.  Replaces the finite-difference Jacobian scipy
 * builds from jac_sparsity (scipy/optimize/_numdiff.py:628-705). */
int ba_linearize(ba_handle* h, int32_t loss, double f_scale,
                 double* Hcc, double* bc, double* Hpp, double* bp);

/* K4 test hook: the reduced camera system of one LM iteration, formed and applied as ba_solve does it.
 * Linearises at the current parameters (loss, f_scale), damps at lambda and returns
 *   g    = -(bc - W (Hpp+lam Dp)^-1 bp)                         double[Nc][NB]
 *   minv = the PCG preconditioner blocks, packed upper triangles  double[Nc][NH]
 *   sv   = S v for n_vec vectors v (double[n_vec][Nc][NB]), S = (Hcc+lam Dc) - W (Hpp+lam Dp)^-1 W^T,
 *          in the PCG loop's launch form (fp32 Jacobian blocks when jacobian_precision = 1)
 * precond: 0 Jacobi, 1 Schur-Jacobi, 2 Schur-Jacobi blocks built at lambda_prev and kept (ba_options.precond_lag).
 * intr == NULL: the pinhole camera (NB 6, NH 21); else (f, k1, k2)[Nc] of the BAL camera (NB 9, NH 45), the handle
 * staying in the pinhole layout afterwards.  The fixed camera's and held rows of S are identity, their g entries zero.
 * g, minv may be NULL. */
int ba_schur_system(ba_handle* h, const double* intr, int32_t loss, double f_scale, double lambda, int32_t precond,
                    double lambda_prev, int32_t jacobian_precision, int32_t n_vec, const double* v, double* sv,
                    double* g, double* minv);

/* Marginal covariances of the cameras and points at the current parameters (normally right after ba_solve / ba_solve_bal;
 * Ceres' Covariance, g2o's computeMarginals, GTSAM's Marginals; no reference counterpart).  H = J^T diag(w) J is the
 * Gauss-Newton matrix of `loss` / f_scale (the IRLS weights of the solve, no damping, unit pixel noise: multiply by
 * 2 cost / (m - n), m residuals and n free parameters, for the variance estimated from the fit).  Free parameters are those
 * neither fixed_cam nor the ba_set_held masks hold; Sigma = (H_free)^-1, and held parameters get rows and columns that are
 * exactly 0.0 (the covariance conditional on the held values, like Ceres' constant blocks).  Computed through the Schur
 * complement S = U - W V^-1 W^T (held rows identity, as in ba_schur_system), Sigma_cams = S^-1 formed densely on the device,
 * Sigma_p = V_p^-1 + V_p^-1 (sum_{i,j in obs(p)} W_i^T Sigma[c_i, c_j] W_j) V_p^-1.  Held points are left out of S, their
 * Sigma_p is 0.  A free point seen from one camera only (one observation, or several by the same camera) has an
 * unobservable depth: it is left out of S with its observations (their information about the camera is exactly what
 * marginalising the point removes) and its Sigma_p is NaN.
 *   intr     NULL: the pinhole (NB 6, NH 21); else (f, k1, k2)[Nc] of the BAL camera (NB 9, NH 45), as in ba_schur_system
 *   rcond    rank test: a Cholesky pivot d_k <= rcond * S_kk (S's own diagonal entry) of S, or of the 3x3 V_p of a free
 *            point seen from two or more cameras, fails the call with BA_ERR_NUMERIC; ba_last_error() names the first
 *            camera and parameter (and says the gauge must be fixed: 6 pose dof + scale for the pinhole with fixed_cam,
 *            7 for a BAL problem with nothing held) or the first point.  rcond <= 0: the library default, 1e-10
 *            (DESIGN.md 4e).  Nothing is written on failure.
 *   cam_cov  double[Nc][NH]   packed upper triangles of the cameras' diagonal blocks, Hcc's order
 *   pt_cov   double[Np][6]    the points' 3x3 blocks, Hpp's order
 *   cam_full double[N][N]     N = NB Nc, row-major: the whole camera covariance, cross-camera blocks included
 * Any output may be NULL.  Refused: BA_ERR_STATE before ba_set_params; BA_ERR_INVALID in a multi-rank job, for N > 16384
 * (the dense matrix, 2 GiB of fp64, is allocated for the call and released before it returns), for ba_schur_system's
 * argument errors (loss, f_scale, BAL mask bits on the pinhole).  The handle is left as it was found (parameters, masks,
 * intrinsics; a later ba_solve gives bit-identical results).  S is assembled with fp64 atomics: the covariances are not
 * bitwise reproducible run to run. */
int ba_covariance(ba_handle* h, const double* intr, int32_t loss, double f_scale, double rcond, double* cam_cov, double* pt_cov,
                  double* cam_full);

/* K2-K7: the whole LM / Schur / PCG loop on the device; replaces the
 * scipy.optimize.least_squares call at src/bundle_adjuster.py:170-174. */
int ba_default_options(ba_options* opts);
int ba_solve(ba_handle* h, const ba_options* opts, ba_summary* summary);
int ba_get_profile(ba_handle* h, ba_profile* out);
int ba_reset_profile(ba_handle* h);

/* Bench hook: run one kernel `reps` times back to back on the solver stream between two
 * HIP events and return the mean duration in microseconds (state left as it was).  BA_K_TRACKS: every kernel of the last
 * ba_triangulate_tracks call (BA_ERR_STATE without one since ba_set_problem), at the current cameras.  BA_K_RESECT: the same
 * for the last ba_resect call (its write-back is not repeated), and BA_K_RESECT_RANSAC for the last ba_resect_ransac call. */
int ba_time_kernel(ba_handle* h, int slot, int reps, double* mean_us);

#ifdef __cplusplus
}
#endif
#endif /* BA_HIP_H */
