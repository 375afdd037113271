// Similarity transform of the reconstruction and robust alignment to reference positions (ba_transform, ba_align,
// ba_get_centres): the step after an adjustment that moves the result into the frame its user needs -- georegistration
// onto GPS / ground control (COLMAP's model_aligner), the comparison of two gauge-free solves.  Stand-alone fp64 kernels:
// they read and write the handle's parameter sets and none of the LM / Schur / PCG kernels.
//
// Conventions: X' = s R X + t, R row-major; a world-to-camera pose (R_c, t_c) becomes R_c' = R_c R^T, t_c' = s t_c - R_c' t,
// so camera-frame coordinates are s times the old ones and every residual (both models divide by depth) is unchanged.
//
//   log map      rvec' of R_c R^T through the unit quaternion picked by the largest of trace and diagonal entries (Shepperd),
//                w >= 0, theta = 2 atan2(|v|, w), rvec = v theta / |v| (2 v / w below |v| = 1e-10).  The acos(trace) / skew
//                form loses 2e-5 near pi; this one round-trips to 1e-15 at every angle.
//   transform    a thread per point slot (parameter set `cur` -> set 0, the table's other words 0 as ba_set_params leaves
//                them), a thread per camera (rvec | t of set 0), then k_cam_prepare's work on set 0.  A record whose status is
//                not OK makes all three no-ops: nothing on the device changes, and the host leaves the handle's state alone.
//   alignment    weighted Umeyama in two reduction passes: A = W, sum u a, sum u b (7 sums) -> centroids; B = the nine sums of
//                u (b - mu_b)(a - mu_a)^T and sum u |a - mu_a|^2, centred (references in UTM are 5e6 with metre-sized
//                structure), and the three of u (b - mu_b): a centroid at 5e6 is known to its ulp, 9e-10, from pass A; that
//                centred sum is what is left of it (lo), and the distances of the IRLS weights use mu_b + lo unrounded --
//                without it the ulp reaches every weight (f_scale 0.15) and the non-convex losses amplify it to 1e-8 in R
//                between two summation orders.  A one-wave kernel folds the per-workgroup partials in index order, runs a one-sided Jacobi SVD of
//                the 3 x 3 Sigma (jacobi_svd<3, 24> of ba_linalg.hpp) and writes s, R, t and the status into the
//                device record the next pass reads.  IRLS rounds recompute u_i = w_i rho'(w_i d_i^2 / f_scale^2) inside pass A.
//                A last pass writes the errors d_i and folds their sum of squares and maximum.
// Sums: a grid-stride loop in a fixed order, wave_total_dpp inside a wave, the four waves through LDS in wave order, one
// partial row per workgroup, no atomics: results are bit-reproducible from call to call.  The grid depends on the
// correspondence count alone.
#pragma once
#include "ba_kernels.hpp"
#include "ba_linalg.hpp"

namespace ba {

enum : int { SIM_OK = 0, SIM_TOO_FEW = 1, SIM_DEGENERATE = 2 };
constexpr int SIM_THREADS = 256;      // threads per workgroup of the reduction passes (four waves)
constexpr int SIM_WAVES = SIM_THREADS / 64;
constexpr int SIM_MAX_BLOCKS = 128;   // most workgroups of a pass (= most partial rows the one-wave fold reads)
constexpr int SIM_PART = 13;          // doubles per partial row: pass A uses 7, pass B 13, the error pass 2
constexpr double SIM_RANK_TOL = 1e-12;

struct SimRec {
  double s, R[9], t[3];
  double mu_a[3], mu_b[3], W;
  double lo[3];             // what the first pass's rounding left out of mu_b: sum u (b - mu_b) / W, from the second pass
  double rms, max;
  int status, pad;
};

// rho'(z) of the solve's losses (ba_loss), z >= 0
__device__ inline double sim_rho_prime(const int loss, const double z) {
  if (loss == LOSS_HUBER) return z <= 1.0 ? 1.0 : 1.0 / sqrt(z);
  if (loss == LOSS_SOFT_L1) return 1.0 / sqrt(1.0 + z);
  if (loss == LOSS_CAUCHY) return 1.0 / (1.0 + z);
  if (loss == LOSS_ARCTAN) return 1.0 / (1.0 + z * z);
  return 1.0;
}

// ---- transform ------------------------------------------------------------------------------------------------------
__global__ void k_sim_set(const SimRec v, SimRec* __restrict__ rec) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *rec = v;
}

// (src and dst are the same table when set 0 is current: no __restrict__ on the pair)
__global__ void k_sim_transform_points(const SimRec* __restrict__ rec, const double* src, int n_pts, double* dst) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pts) return;
  if (rec->status != SIM_OK) return;
  const double* q = src + PT * (size_t)p;
  const double X0 = q[0], X1 = q[1], X2 = q[2];
  const double s = rec->s;
  const double Y0 = s * (rec->R[0] * X0 + rec->R[1] * X1 + rec->R[2] * X2) + rec->t[0];
  const double Y1 = s * (rec->R[3] * X0 + rec->R[4] * X1 + rec->R[5] * X2) + rec->t[1];
  const double Y2 = s * (rec->R[6] * X0 + rec->R[7] * X1 + rec->R[8] * X2) + rec->t[2];
  double* o = dst + PT * (size_t)p;
  o[0] = Y0; o[1] = Y1; o[2] = Y2;
  o[3] = 0; o[4] = 0; o[5] = 0; o[6] = 0; o[7] = 0;
}

// cs: the camera state of set `cur` (R_c, t_c); cams_dst: rvec | t of set 0
__global__ void k_sim_transform_cams(const SimRec* __restrict__ rec, const double* __restrict__ cs, int n_cams,
                                     double* __restrict__ cams_dst) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_cams || rec->status != SIM_OK) return;
  const double* st = cs + CS * (size_t)c;
  double Rn[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) Rn[3 * i + j] = st[3 * i] * rec->R[3 * j] + st[3 * i + 1] * rec->R[3 * j + 1] + st[3 * i + 2] * rec->R[3 * j + 2];
  double rv[3];
  sim_log_map(Rn, rv);
  const double s = rec->s, t0 = rec->t[0], t1 = rec->t[1], t2 = rec->t[2];
  double* o = cams_dst + 6 * (size_t)c;
  o[0] = rv[0]; o[1] = rv[1]; o[2] = rv[2];
  o[3] = s * st[9] - (Rn[0] * t0 + Rn[1] * t1 + Rn[2] * t2);
  o[4] = s * st[10] - (Rn[3] * t0 + Rn[4] * t1 + Rn[5] * t2);
  o[5] = s * st[11] - (Rn[6] * t0 + Rn[7] * t1 + Rn[8] * t2);
}

// k_cam_prepare<Pinhole> of set 0 behind the two kernels above, when the record is OK
__global__ void k_sim_cam_prepare(const SimRec* __restrict__ rec, const double* __restrict__ cams, const double* __restrict__ intr,
                                  double* __restrict__ cs, double* __restrict__ camA, int n_cams) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_cams || rec->status != SIM_OK) return;
  camera_state(cams + 6 * c, cs + CS * c);
  Pinhole::table_row(cs + CS * c, intr + 3 * (size_t)c, camA + Pinhole::TA * (size_t)c);
}

// ---- correspondences ------------------------------------------------------------------------------------------------
// a = camera centres -R_c^T t_c of the first n_cam cameras, then the points in the caller's order (through the slot table)
__global__ void k_sim_gather(const double* __restrict__ cs, int n_cam, const double* __restrict__ ptab, const int* __restrict__ slot,
                             int n_pt, double* __restrict__ a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_cam + n_pt) return;
  double* o = a + 3 * (size_t)i;
  if (i < n_cam) {
    cam_centre(cs + CS * (size_t)i, o);
  } else {
    const double* q = ptab + PT * (size_t)slot[i - n_cam];
    o[0] = q[0]; o[1] = q[1]; o[2] = q[2];
  }
}

// v[0 .. NS) summed over the workgroup into out[0 .. NS): DPP inside a wave, the waves through LDS in wave order
template <int NS>
__device__ __forceinline__ void sim_block_sums(const double (&v)[NS], double* __restrict__ lds, double* __restrict__ out) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    const double t = wave_total_dpp(v[j]);
    if (lane == 0) lds[wv * NS + j] = t;
  }
  __syncthreads();
  if (threadIdx.x < NS) {
    double s = lds[threadIdx.x];
#pragma unroll
    for (int k = 1; k < SIM_WAVES; ++k) s += lds[k * NS + threadIdx.x];
    out[threadIdx.x] = s;
  }
}

// d_i^2 = |b_i - (s R a_i + t)|^2 at the record's similarity, whose t = mu_b - s R mu_a, evaluated in the centred form
// |((b_i - mu_b) - lo) - s R (a_i - mu_a)|^2: the same number without the rounding a far-away t puts on it (|t| = 5e6 has an ulp of
// 1e-9, which would reach the IRLS weights of every round)
__device__ __forceinline__ double sim_dist2(const SimRec* __restrict__ rec, const double* __restrict__ a, const double* __restrict__ b) {
  const double s = rec->s;
  const double x0 = a[0] - rec->mu_a[0], x1 = a[1] - rec->mu_a[1], x2 = a[2] - rec->mu_a[2];
  const double e0 = ((b[0] - rec->mu_b[0]) - rec->lo[0]) - s * (rec->R[0] * x0 + rec->R[1] * x1 + rec->R[2] * x2);
  const double e1 = ((b[1] - rec->mu_b[1]) - rec->lo[1]) - s * (rec->R[3] * x0 + rec->R[4] * x1 + rec->R[5] * x2);
  const double e2 = ((b[2] - rec->mu_b[2]) - rec->lo[2]) - s * (rec->R[6] * x0 + rec->R[7] * x1 + rec->R[8] * x2);
  return e0 * e0 + e1 * e1 + e2 * e2;
}

// pass A: the round's weights u (irls = 0: u = w; else w rho'(w d^2 / f_scale^2) at the record's similarity), W, sum u a, sum u b
__global__ void __launch_bounds__(SIM_THREADS)
k_sim_pass_a(const SimRec* __restrict__ rec, int n, const double* __restrict__ a, const double* __restrict__ b,
             const double* __restrict__ w, int irls, int loss, double inv_f2, double* __restrict__ u, double* __restrict__ part) {
  __shared__ double lds[SIM_WAVES * 7];
  if (rec->status != SIM_OK) return;
  double v[7] = {0, 0, 0, 0, 0, 0, 0};
  for (int i = blockIdx.x * SIM_THREADS + threadIdx.x; i < n; i += gridDim.x * SIM_THREADS) {
    const double wi = w[i];
    double ui = 0.0;
    if (wi > 0.0) {
      const double* ai = a + 3 * (size_t)i;
      const double* bi = b + 3 * (size_t)i;
      ui = irls ? wi * sim_rho_prime(loss, wi * sim_dist2(rec, ai, bi) * inv_f2) : wi;
      v[0] += ui;
      v[1] += ui * ai[0]; v[2] += ui * ai[1]; v[3] += ui * ai[2];
      v[4] += ui * bi[0]; v[5] += ui * bi[1]; v[6] += ui * bi[2];
    }
    u[i] = ui;
  }
  sim_block_sums<7>(v, lds, part + SIM_PART * (size_t)blockIdx.x);
}

// fold of pass A: centroids into the record
__global__ void __launch_bounds__(64) k_sim_centroid(const double* __restrict__ part, int n_blocks, SimRec* __restrict__ rec) {
  __shared__ double sh[8];
  if (rec->status != SIM_OK) return;
  if (threadIdx.x < 7) {
    double s = 0.0;
    for (int k = 0; k < n_blocks; ++k) s += part[SIM_PART * (size_t)k + threadIdx.x];
    sh[threadIdx.x] = s;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  bool fin = true;
  for (int j = 0; j < 7; ++j) fin = fin && sim_finite(sh[j]);
  const double W = sh[0];
  if (!fin || !(W > 0.0)) { rec->status = SIM_DEGENERATE; return; }
  rec->W = W;
  for (int j = 0; j < 3; ++j) { rec->mu_a[j] = sh[1 + j] / W; rec->mu_b[j] = sh[4 + j] / W; }
}

// pass B: the centred sums  u (b - mu_b)(a - mu_a)^T (row-major, 9), u |a - mu_a|^2 and u (b - mu_b) (3)
__global__ void __launch_bounds__(SIM_THREADS)
k_sim_pass_b(const SimRec* __restrict__ rec, int n, const double* __restrict__ a, const double* __restrict__ b,
             const double* __restrict__ u, double* __restrict__ part) {
  __shared__ double lds[SIM_WAVES * 13];
  if (rec->status != SIM_OK) return;
  const double ma0 = rec->mu_a[0], ma1 = rec->mu_a[1], ma2 = rec->mu_a[2];
  const double mb0 = rec->mu_b[0], mb1 = rec->mu_b[1], mb2 = rec->mu_b[2];
  double v[13] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = blockIdx.x * SIM_THREADS + threadIdx.x; i < n; i += gridDim.x * SIM_THREADS) {
    const double ui = u[i];
    if (ui > 0.0) {
      const double* ai = a + 3 * (size_t)i;
      const double* bi = b + 3 * (size_t)i;
      const double x0 = ai[0] - ma0, x1 = ai[1] - ma1, x2 = ai[2] - ma2;
      const double y0 = ui * (bi[0] - mb0), y1 = ui * (bi[1] - mb1), y2 = ui * (bi[2] - mb2);
      v[0] += y0 * x0; v[1] += y0 * x1; v[2] += y0 * x2;
      v[3] += y1 * x0; v[4] += y1 * x1; v[5] += y1 * x2;
      v[6] += y2 * x0; v[7] += y2 * x1; v[8] += y2 * x2;
      v[9] += ui * (x0 * x0 + x1 * x1 + x2 * x2);
      v[10] += y0; v[11] += y1; v[12] += y2;
    }
  }
  sim_block_sums<13>(v, lds, part + SIM_PART * (size_t)blockIdx.x);
}

// The closed form from the centred sums sh (Sigma W row-major, var_a W, lo W) and the record's W, mu_a, mu_b:
// Sigma = U D V^T, R = U diag(1, 1, det U det V) V^T, s = tr(D diag) / var_a, t = (mu_b - s R mu_a) + lo, written into the record;
// else the record's status becomes DEGENERATE.  The third left vector is formed as u1 x u2 (a rank-2 Sigma -- coplanar
// positions -- has none of its own): with u3 = det(U) (u1 x u2), R = u1 v1^T + u2 v2^T + det(V) (u1 x u2) v3^T.
__host__ __device__ inline void sim_closed_form(const double* __restrict__ sh, int with_scale, SimRec* __restrict__ rec) {
  bool fin = true;
  for (int j = 0; j < 13; ++j) fin = fin && sim_finite(sh[j]);
  const double W = rec->W;
  const double var_a = sh[9] / W;
  if (!fin || !(var_a > 0.0)) { rec->status = SIM_DEGENERATE; return; }
  double U[3][3], V[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) U[i][j] = sh[3 * i + j] / W;
  jacobi_svd<3, 24>(U, V);
  double n2[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) n2[k] = U[0][k] * U[0][k] + U[1][k] * U[1][k] + U[2][k] * U[2][k];
  sim_order<0, 1>(U, V, n2); sim_order<1, 2>(U, V, n2); sim_order<0, 1>(U, V, n2);
  const double d0 = sqrt(n2[0]), d1 = sqrt(n2[1]), d2 = sqrt(n2[2]);
  if (!(d1 > SIM_RANK_TOL * d0)) { rec->status = SIM_DEGENERATE; return; }
  double u1[3], u2[3], u3[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) { u1[k] = U[k][0] / d0; u2[k] = U[k][1] / d1; }
  u3[0] = u1[1] * u2[2] - u1[2] * u2[1];
  u3[1] = u1[2] * u2[0] - u1[0] * u2[2];
  u3[2] = u1[0] * u2[1] - u1[1] * u2[0];
  const double detV = V[0][0] * (V[1][1] * V[2][2] - V[1][2] * V[2][1]) - V[0][1] * (V[1][0] * V[2][2] - V[1][2] * V[2][0]) +
                      V[0][2] * (V[1][0] * V[2][1] - V[1][1] * V[2][0]);
  const double sV = detV >= 0.0 ? 1.0 : -1.0;
  const double sU = (u3[0] * U[0][2] + u3[1] * U[1][2] + u3[2] * U[2][2]) >= 0.0 ? 1.0 : -1.0;
  double R[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) R[3 * i + j] = u1[i] * V[j][0] + u2[i] * V[j][1] + sV * u3[i] * V[j][2];
  const double s = with_scale ? (d0 + d1 + sU * sV * d2) / var_a : 1.0;
  bool ok = sim_finite(s) && s > 0.0;
  for (int j = 0; j < 9; ++j) ok = ok && sim_finite(R[j]);
  if (!ok) { rec->status = SIM_DEGENERATE; return; }
  rec->s = s;
  for (int j = 0; j < 9; ++j) rec->R[j] = R[j];
  for (int i = 0; i < 3; ++i) {
    rec->lo[i] = sh[10 + i] / W;
    rec->t[i] = (rec->mu_b[i] - s * (R[3 * i] * rec->mu_a[0] + R[3 * i + 1] * rec->mu_a[1] + R[3 * i + 2] * rec->mu_a[2])) + rec->lo[i];
  }
}

// fold of pass B (partial rows in index order) and the closed form, one wave
__global__ void __launch_bounds__(64) k_sim_solve(const double* __restrict__ part, int n_blocks, int with_scale, SimRec* __restrict__ rec) {
  __shared__ double sh[13];
  if (rec->status != SIM_OK) return;
  if (threadIdx.x < 13) {
    double s = 0.0;
    for (int k = 0; k < n_blocks; ++k) s += part[SIM_PART * (size_t)k + threadIdx.x];
    sh[threadIdx.x] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) sim_closed_form(sh, with_scale, rec);
}

// the errors d_i at the record's similarity (NaN without a reference, or without a similarity), sum d^2 and max d over w > 0
__global__ void __launch_bounds__(SIM_THREADS)
k_sim_errors(const SimRec* __restrict__ rec, int n, const double* __restrict__ a, const double* __restrict__ b,
             const double* __restrict__ w, double* __restrict__ err, double* __restrict__ part) {
  __shared__ double lds[SIM_WAVES * 2];
  const bool ok = rec->status == SIM_OK;
  const double nan = HY_NAN;
  double v[1] = {0.0};
  double m = 0.0;
  for (int i = blockIdx.x * SIM_THREADS + threadIdx.x; i < n; i += gridDim.x * SIM_THREADS) {
    double d = nan;
    if (ok && w[i] > 0.0) {
      const double d2 = sim_dist2(rec, a + 3 * (size_t)i, b + 3 * (size_t)i);
      d = sqrt(d2);
      v[0] += d2;
      m = nanmax(m, d);
    }
    err[i] = d;
  }
  m = wave_nanmax(m);
  const double t = wave_total_dpp(v[0]);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) { lds[wv] = t; lds[SIM_WAVES + wv] = m; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = lds[0], mm = lds[SIM_WAVES];
    for (int k = 1; k < SIM_WAVES; ++k) { s += lds[k]; mm = nanmax(mm, lds[SIM_WAVES + k]); }
    part[SIM_PART * (size_t)blockIdx.x] = s;
    part[SIM_PART * (size_t)blockIdx.x + 1] = mm;
  }
}

// fold of the error pass; a record that is not OK ends as the identity with NaN measures
__global__ void __launch_bounds__(64) k_sim_finish(const double* __restrict__ part, int n_blocks, int n_used, SimRec* __restrict__ rec) {
  if (threadIdx.x != 0) return;
  const double nan = HY_NAN;
  if (rec->status != SIM_OK) {
    rec->s = 1.0;
    for (int j = 0; j < 9; ++j) rec->R[j] = (j % 4 == 0) ? 1.0 : 0.0;
    rec->t[0] = rec->t[1] = rec->t[2] = 0.0;
    rec->rms = nan; rec->max = nan;
    return;
  }
  double s = 0.0, m = 0.0;
  for (int k = 0; k < n_blocks; ++k) { s += part[SIM_PART * (size_t)k]; m = nanmax(m, part[SIM_PART * (size_t)k + 1]); }
  rec->rms = sqrt(s / (double)n_used);
  rec->max = m;
}

// camera centres -R_c^T t_c, 3 doubles per camera (ba_get_centres)
__global__ void k_sim_centres(const double* __restrict__ cs, int n_cams, double* __restrict__ out) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_cams) return;
  cam_centre(cs + CS * (size_t)c, out + 3 * (size_t)c);
}

}  // namespace ba
