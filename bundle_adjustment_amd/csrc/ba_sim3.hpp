// Sim(3) from 3D-3D matches (ba_sim3): the similarity X2 ~ s R X1 + t between two camera frames from matched map points, a
// share of which may be wrong -- the measurement of a loop edge (ORB-SLAM's Sim3Solver + OptimizeSim3, COLMAP's similarity
// LO-RANSAC).  A fourth user of the hypothesis stage (ba_hypothesis.hpp) with the closed form of ba_similarity.hpp as its
// minimal solver and the chart of ba_pose_graph in its refinement.  Stand-alone kernels: they read the call's own staging
// buffers and nothing of a resident problem.  The images are the projections of the points themselves, x(X) = (X_x, X_y) / X_z.
//
// Two launches per call, for all pairs at once:
//   k_sim3_score  grid (pairs, ceil(n_hyp / 256)): lane = hypothesis.  Sample of three -> flat tests in both frames -> centred
//                 sums -> sim_closed_form (jacobi_svd<3, 24>) -> s R, R, t, s in registers -> the pair's correspondences stream
//                 through LDS in tiles of HY_TILE (X1 | X2 | x1 | x2, ten doubles; x1 = x2 = NaN marks an invalid one); MSAC
//                 cost of the two reprojection errors; the block's lowest (cost, h) by hy_block_best.
//   k_sim3_lo     one workgroup per pair: the lowest (cost, h) over the score blocks, lo_rounds of {consensus bytes; the closed
//                 form on the whole set, kept if it lowers the set's cost; Marquardt-damped Gauss-Newton in (omega, tau, sigma):
//                 R <- exp(omega) R, t <- t + tau, s <- s exp(sigma)}, the measures, the Hessian of the final inlier set, the
//                 status.  The last accepted model and its 36 sums live in LDS.  Sums by rs_block_sums: fixed order, no atomics.
//
// Jacobians (g0, g1 the rows of d x / d Y at Y, that is (1, 0, -p_x) / Y_z and (0, 1, -p_y) / Y_z):
//   forward   Y = s R X1 + t, A = Y - t:    d Y = omega x A + tau + sigma A             -> row  [A x g | g | g . A]
//   backward  Z = R^T (X2 - t) / s:         d Z = [Z]x R^T omega - R^T tau / s - sigma Z -> row  [R (g x Z) | -R g | 0] with Z
//             unscaled (x(Z) does not see s, and the 1 / s of d Z cancels the s of g): the backward residual does not move with sigma.
#pragma once
#include "ba_hypothesis.hpp"
#include "ba_posegraph.hpp"
#include "ba_resect.hpp"
#include "ba_similarity.hpp"

namespace ba {

enum : int { S3_OK = 0, S3_FEW_MATCHES = 1, S3_DEGENERATE = 2, S3_FEW_INLIERS = 3 };
constexpr int S3_THREADS = HY_THREADS;
constexpr int S3_MODEL = 13;                   // R[9] | t[3] | s
constexpr int S3_BEST = 16;                    // doubles per (pair, score block): cost | h | model | one of padding
constexpr int S3_NSUM = 36;                    // a refinement pass: J^T J (28, packed upper) | g (7) | cost
constexpr int S3_OUT = 48;                     // doubles per pair: rvec t s | R[9] | status n_inliers rms best_hyp | J^T J fbar^2 (28)
constexpr int S3_CORR = 10;                    // doubles of a correspondence in the LDS tile: X1 | X2 | x1 | x2
static_assert(S3_THREADS == RS_THREADS, "rs_block_sums folds RS_WAVES waves");

struct Sim3Args : HypArgs {   // thr = max_px / fbar; best: S3_BEST doubles per (pair, score block); out: S3_OUT per pair
  int with_scale;
  const double* X1;        // 3 per correspondence: the point in the first / second camera frame
  const double* X2;
};

// correspondence j: both points and their images; false (and NaN images) for a non-finite coordinate or z <= 0 in its own frame
__device__ __forceinline__ bool s3_load(const Sim3Args& a, const long long j, double (&A)[3], double (&B)[3], double2& x1, double2& x2) {
#pragma unroll
  for (int k = 0; k < 3; ++k) { A[k] = a.X1[3 * j + k]; B[k] = a.X2[3 * j + k]; }
  const bool ok = sim_finite(A[0]) && sim_finite(A[1]) && sim_finite(A[2]) && sim_finite(B[0]) && sim_finite(B[1]) && sim_finite(B[2]) &&
                  A[2] > 0.0 && B[2] > 0.0;
  x1 = ok ? make_double2(A[0] / A[2], A[1] / A[2]) : make_double2(HY_NAN, HY_NAN);
  x2 = ok ? make_double2(B[0] / B[2], B[1] / B[2]) : make_double2(HY_NAN, HY_NAN);
  return ok;
}
__device__ __forceinline__ void s3_identity(double (&M)[S3_MODEL]) {
#pragma unroll
  for (int q = 0; q < 9; ++q) M[q] = (q % 4 == 0) ? 1.0 : 0.0;
  M[9] = M[10] = M[11] = 0.0; M[12] = 1.0;
}
// a triple with |d12 x d13| <= HY_AREA_TOL max |d_ij|^2 (collinear or coincident), 3D
__device__ __forceinline__ bool s3_flat(const double (&p)[3], const double (&q)[3], const double (&r)[3]) {
  const double a0 = q[0] - p[0], a1 = q[1] - p[1], a2 = q[2] - p[2], b0 = r[0] - p[0], b1 = r[1] - p[1], b2 = r[2] - p[2];
  const double c0 = r[0] - q[0], c1 = r[1] - q[1], c2 = r[2] - q[2];
  const double ext = fmax(fmax(a0 * a0 + a1 * a1 + a2 * a2, b0 * b0 + b1 * b1 + b2 * b2), c0 * c0 + c1 * c1 + c2 * c2);
  const double n0 = a1 * b2 - a2 * b1, n1 = a2 * b0 - a0 * b2, n2 = a0 * b1 - a1 * b0;
  return !(sqrt(n0 * n0 + n1 * n1 + n2 * n2) > HY_AREA_TOL * ext) || !sim_finite(ext);
}
// The closed form of DESIGN 4i from the centred sums sh (Sigma W row-major, var_a W, three zeros), the weight W and the
// centroids: sim_closed_form's R = U diag(1, 1, det U det V) V^T, s, t = mu_b - s R mu_a.  false: void (not finite, s <= 0, rank < 2)
__device__ __forceinline__ bool s3_closed(const double (&sh)[13], const double W, const double (&mu_a)[3], const double (&mu_b)[3],
                                          const int with_scale, double (&M)[S3_MODEL]) {
  SimRec rec;
  rec.W = W; rec.status = SIM_OK;
#pragma unroll
  for (int k = 0; k < 3; ++k) { rec.mu_a[k] = mu_a[k]; rec.mu_b[k] = mu_b[k]; }
  sim_closed_form(sh, with_scale, &rec);
  if (rec.status != SIM_OK) return false;
  bool ok = true;
#pragma unroll
  for (int q = 0; q < 9; ++q) M[q] = rec.R[q];
#pragma unroll
  for (int k = 0; k < 3; ++k) { M[9 + k] = rec.t[k]; ok = ok && sim_finite(rec.t[k]); }
  M[12] = rec.s;
  return ok;
}
// step 3 on a sample of three valid correspondences
__device__ __forceinline__ bool s3_solve3(const double (&A)[3][3], const double (&B)[3][3], const int with_scale, double (&M)[S3_MODEL]) {
  if (s3_flat(A[0], A[1], A[2]) || s3_flat(B[0], B[1], B[2])) return false;
  double mu_a[3], mu_b[3], sh[13];
#pragma unroll
  for (int k = 0; k < 3; ++k) { mu_a[k] = ((A[0][k] + A[1][k]) + A[2][k]) / 3.0; mu_b[k] = ((B[0][k] + B[1][k]) + B[2][k]) / 3.0; }
#pragma unroll
  for (int q = 0; q < 13; ++q) sh[q] = 0.0;
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    const double x[3] = {A[p][0] - mu_a[0], A[p][1] - mu_a[1], A[p][2] - mu_a[2]};
    const double y[3] = {B[p][0] - mu_b[0], B[p][1] - mu_b[1], B[p][2] - mu_b[2]};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) sh[3 * i + j] += y[i] * x[j];
    sh[9] += (x[0] * x[0] + x[1] * x[1]) + x[2] * x[2];
  }
  return s3_closed(sh, 3.0, mu_a, mu_b, with_scale, M);
}
// Q = s R
__device__ __forceinline__ void s3_scaled(const double (&M)[S3_MODEL], double (&Q)[9]) {
#pragma unroll
  for (int q = 0; q < 9; ++q) Q[q] = M[12] * M[q];
}
// Y = Q X1 + t and the unscaled Z = R^T (X2 - t)
__device__ __forceinline__ void s3_map(const double (&Q)[9], const double (&M)[S3_MODEL], const double (&A)[3], const double (&B)[3], double (&Y)[3],
                                       double (&Z)[3]) {
  const double d0 = B[0] - M[9], d1 = B[1] - M[10], d2 = B[2] - M[11];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    Y[i] = ((Q[3 * i] * A[0] + Q[3 * i + 1] * A[1]) + Q[3 * i + 2] * A[2]) + M[9 + i];
    Z[i] = (M[i] * d0 + M[3 + i] * d1) + M[6 + i] * d2;
  }
}
// squared forward and backward reprojection errors; pf / pb: the transformed depth is positive
__device__ __forceinline__ void s3_errors(const double (&Q)[9], const double (&M)[S3_MODEL], const double (&A)[3], const double (&B)[3], const double2 x1,
                                          const double2 x2, double& f, double& b, bool& pf, bool& pb) {
  double Y[3], Z[3];
  s3_map(Q, M, A, B, Y, Z);
  const double iy = 1.0 / Y[2], iz = 1.0 / Z[2];
  const double f0 = Y[0] * iy - x2.x, f1 = Y[1] * iy - x2.y, b0 = Z[0] * iz - x1.x, b1 = Z[1] * iz - x1.y;
  f = f0 * f0 + f1 * f1; b = b0 * b0 + b1 * b1;
  pf = Y[2] > 0.0; pb = Z[2] > 0.0;
}
// the consensus test (false for an invalid correspondence: its images are NaN)
__device__ __forceinline__ bool s3_inlier(const double (&Q)[9], const double (&M)[S3_MODEL], const double (&A)[3], const double (&B)[3], const double2 x1,
                                          const double2 x2, const double thr2, double& f, double& b) {
  bool pf, pb;
  s3_errors(Q, M, A, B, x1, x2, f, b, pf, pb);
  return pf && pb && f <= thr2 && b <= thr2;
}

// ------------------------------------------------------------------------------------------------ hypotheses and scores
__global__ void __launch_bounds__(S3_THREADS) k_sim3_score(const Sim3Args a) {
  __shared__ double tile[HY_TILE * S3_CORR];
  __shared__ double red[2 * HY_WAVES];
  const int pair = blockIdx.x, blk = blockIdx.y, tid = threadIdx.x;
  const long long beg = a.off[pair];
  const int n = (int)(a.off[pair + 1] - beg);
  double* out = a.best + S3_BEST * ((size_t)pair * a.n_blk + blk);
  if (n < 4) {                                    // (workgroup-uniform) FEW_MATCHES
    hy_void_block(out);
    return;
  }
  const int h = blk * S3_THREADS + tid;
  bool valid = h < a.n_hyp;
  double M[S3_MODEL], Q[9];
  {
    int idx[3];
    hy_sample(a.seed, pair, valid ? h : 0, n, idx);   // (indices below n for every lane)
    double A[3][3], B[3][3];
    double2 u, v;
#pragma unroll
    for (int k = 0; k < 3; ++k) valid = s3_load(a, beg + idx[k], A[k], B[k], u, v) && valid;
    valid = valid && s3_solve3(A, B, a.with_scale, M);
  }
  if (!valid) s3_identity(M);                     // a void hypothesis runs along on finite numbers
  s3_scaled(M, Q);
  const double thr2 = a.thr * a.thr;
  double cost = 0.0;
  for (int i0 = 0; i0 < n; i0 += HY_TILE) {
    const int m = min(HY_TILE, n - i0);
    __syncthreads();                              // (the readers of the previous tile are done)
    if (tid < m) {
      double A[3], B[3];
      double2 x1, x2;
      s3_load(a, beg + i0 + tid, A, B, x1, x2);
      double2* d = (double2*)(tile + S3_CORR * tid);
      d[0] = make_double2(A[0], A[1]); d[1] = make_double2(A[2], B[0]); d[2] = make_double2(B[1], B[2]); d[3] = x1; d[4] = x2;
    }
    __syncthreads();
    for (int i = 0; i < m; ++i) {                 // every lane reads the same address: an LDS broadcast
      const double2* s = (const double2*)(tile + S3_CORR * i);
      const double2 s0 = s[0], s1 = s[1], s2 = s[2];
      const double A[3] = {s0.x, s0.y, s1.x}, B[3] = {s1.y, s2.x, s2.y};
      double f, b;
      bool pf, pb;
      s3_errors(Q, M, A, B, s[3], s[4], f, b, pf, pb);
      cost += ((pf && f <= thr2) ? f : thr2) + ((pb && b <= thr2) ? b : thr2);   // (NaN images of an invalid one: 2 thr^2)
    }
  }
  double gc, gk;
  const bool mine = hy_block_best(valid ? cost : HY_INF, valid ? (double)h : HY_INF, red, gc, gk);
  if (!(gc < HY_INF)) {
    hy_void_block(out);
    return;
  }
  if (mine) {
    out[0] = gc; out[1] = gk;
#pragma unroll
    for (int q = 0; q < S3_MODEL; ++q) out[2 + q] = M[q];
  }
}

// ------------------------------------------------------------------------------------------------ LO, measures, Hessian
// The sums of a refinement pass over the correspondences flagged in `set` at the model M: the 7 x 7 normal matrix, the gradient
// and 0.5 sum (|r_f|^2 + |r_b|^2) in (omega, tau, sigma); the sigma column is zero without scale.  A member whose transformed
// depth is not positive at this model makes the cost infinite: leaving it out would lower the cost, and the acceptance test
// would then favour a step that pushes points behind a camera.  It cannot happen at a round's starting model (the consensus
// test asks for both depths positive), so it only ever rejects a trial.
__device__ __forceinline__ void s3_pass(const Sim3Args& a, const double (&M)[S3_MODEL], const unsigned char* __restrict__ set, const long long beg,
                                        const int n, double (&acc)[S3_NSUM], double* __restrict__ lds) {
  double Q[9];
  s3_scaled(M, Q);
#pragma unroll
  for (int q = 0; q < S3_NSUM; ++q) acc[q] = 0.0;
  for (int j = (int)threadIdx.x; j < n; j += S3_THREADS) {
    if (!set[beg + j]) continue;
    double A[3], B[3], Y[3], Z[3];
    double2 x1, x2;
    s3_load(a, beg + j, A, B, x1, x2);
    s3_map(Q, M, A, B, Y, Z);
    if (!(Y[2] > 0.0 && Z[2] > 0.0)) { acc[35] = HY_INF; continue; }   // (HY_INF + anything finite stays above every accepted cost)
    const double iy = 1.0 / Y[2], iz = 1.0 / Z[2];
    const double px = Y[0] * iy, py = Y[1] * iy, qx = Z[0] * iz, qy = Z[1] * iz;
    const double r[4] = {px - x2.x, py - x2.y, qx - x1.x, qy - x1.y};
    double J[4][7];
    {
      const double Ab[3] = {Y[0] - M[9], Y[1] - M[10], Y[2] - M[11]};
      const double g[2][3] = {{iy, 0.0, -px * iy}, {0.0, iy, -py * iy}};
      const double w[2][3] = {{iz, 0.0, -qx * iz}, {0.0, iz, -qy * iz}};
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        J[k][0] = Ab[1] * g[k][2] - Ab[2] * g[k][1]; J[k][1] = Ab[2] * g[k][0] - Ab[0] * g[k][2]; J[k][2] = Ab[0] * g[k][1] - Ab[1] * g[k][0];
        J[k][3] = g[k][0]; J[k][4] = g[k][1]; J[k][5] = g[k][2];
        J[k][6] = a.with_scale ? (g[k][0] * Ab[0] + g[k][1] * Ab[1]) + g[k][2] * Ab[2] : 0.0;
        const double c0 = w[k][1] * Z[2] - w[k][2] * Z[1], c1 = w[k][2] * Z[0] - w[k][0] * Z[2], c2 = w[k][0] * Z[1] - w[k][1] * Z[0];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          J[2 + k][i] = (M[3 * i] * c0 + M[3 * i + 1] * c1) + M[3 * i + 2] * c2;
          J[2 + k][3 + i] = -((M[3 * i] * w[k][0] + M[3 * i + 1] * w[k][1]) + M[3 * i + 2] * w[k][2]);
        }
        J[2 + k][6] = 0.0;
      }
    }
#pragma unroll
    for (int q = 0; q < 7; ++q) {
#pragma unroll
      for (int s2 = q; s2 < 7; ++s2) acc[UT(7, q, s2)] += (J[0][q] * J[0][s2] + J[1][q] * J[1][s2]) + (J[2][q] * J[2][s2] + J[3][q] * J[3][s2]);
      acc[28 + q] += (J[0][q] * r[0] + J[1][q] * r[1]) + (J[2][q] * r[2] + J[3][q] * r[3]);
    }
    acc[35] += 0.5 * ((r[0] * r[0] + r[1] * r[1]) + (r[2] * r[2] + r[3] * r[3]));
  }
  rs_block_sums<S3_NSUM>(acc, lds);
}

// R <- exp(omega) R, t <- t + tau, s <- s exp(sigma).  A model that is not finite fails every depth test of s3_pass: the
// trial's cost is infinite and the step is rejected
__device__ __forceinline__ void s3_move(const double (&M)[S3_MODEL], const double (&dx)[7], double (&Y)[S3_MODEL]) {
  double dR[9];
  pg_rodrigues(dx, dR);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) Y[3 * i + j] = (dR[3 * i] * M[j] + dR[3 * i + 1] * M[3 + j]) + dR[3 * i + 2] * M[6 + j];
#pragma unroll
  for (int k = 0; k < 3; ++k) Y[9 + k] = M[9 + k] + dx[3 + k];
  Y[12] = M[12] * exp(dx[6]);
}

// step 5a: the closed form on the whole consensus set (cn members); false: void
__device__ __forceinline__ bool s3_fit_set(const Sim3Args& a, const long long beg, const int n, const double cn, double (&M)[S3_MODEL],
                                           double* __restrict__ lds) {
  double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int j = (int)threadIdx.x; j < n; j += S3_THREADS) {
    if (!a.cons[beg + j]) continue;
#pragma unroll
    for (int k = 0; k < 3; ++k) { v[k] += a.X1[3 * (beg + j) + k]; v[3 + k] += a.X2[3 * (beg + j) + k]; }
  }
  rs_block_sums<6>(v, lds);
  const double mu_a[3] = {v[0] / cn, v[1] / cn, v[2] / cn}, mu_b[3] = {v[3] / cn, v[4] / cn, v[5] / cn};
  double c[10];
#pragma unroll
  for (int q = 0; q < 10; ++q) c[q] = 0.0;
  for (int j = (int)threadIdx.x; j < n; j += S3_THREADS) {   // centred before the products, as DESIGN 4i does
    if (!a.cons[beg + j]) continue;
    double x[3], y[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { x[k] = a.X1[3 * (beg + j) + k] - mu_a[k]; y[k] = a.X2[3 * (beg + j) + k] - mu_b[k]; }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int k = 0; k < 3; ++k) c[3 * i + k] += y[i] * x[k];
    c[9] += (x[0] * x[0] + x[1] * x[1]) + x[2] * x[2];
  }
  rs_block_sums<10>(c, lds);
  double sh[13];
#pragma unroll
  for (int q = 0; q < 13; ++q) sh[q] = q < 10 ? c[q] : 0.0;
  return s3_closed(sh, cn, mu_a, mu_b, a.with_scale, M);
}

// a pair without a model: the identity, no inliers
__device__ __forceinline__ void s3_void(double* __restrict__ o, const int status) {
  if (threadIdx.x != 0) return;
  for (int q = 0; q < S3_OUT; ++q) o[q] = 0.0;
  o[6] = 1.0; o[7] = 1.0; o[11] = 1.0; o[15] = 1.0;
  o[16] = (double)status; o[18] = HY_NAN; o[19] = -1.0;
}

__global__ void __launch_bounds__(S3_THREADS) k_sim3_lo(const Sim3Args a) {
  __shared__ double lds[RS_WAVES * S3_NSUM];
  __shared__ double s_cur[S3_NSUM], s_x[S3_MODEL];   // the refinement's last accepted sums and model
  const int pair = blockIdx.x, tid = threadIdx.x;
  const long long beg = a.off[pair];
  const int n = (int)(a.off[pair + 1] - beg);
  double* o = a.out + S3_OUT * (size_t)pair;
  if (n < 4) { s3_void(o, S3_FEW_MATCHES); return; }   // (workgroup-uniform, like every branch below)
  // the lowest (cost, h) over the score blocks, in block order: the same in every lane
  const double* b = a.best + S3_BEST * (size_t)pair * a.n_blk;
  double gc, gk;
  const int win = hy_winner<S3_BEST>(b, a.n_blk, gc, gk);
  if (!(gc < HY_INF)) { s3_void(o, S3_DEGENERATE); return; }   // every hypothesis void
  const int best = (int)gk;
  double M[S3_MODEL], Q[9];
#pragma unroll
  for (int q = 0; q < S3_MODEL; ++q) M[q] = b[S3_BEST * win + 2 + q];
  const double thr2 = a.thr * a.thr;
  int status = S3_OK;
  // ---- local optimisation
  for (int round = 0; round < a.lo_rounds && status == S3_OK; ++round) {
    s3_scaled(M, Q);
    double cn[1] = {0.0};
    for (int j = tid; j < n; j += S3_THREADS) {   // every lane writes the bytes it reads back in the passes (same stride)
      double A[3], B[3], f, bb;
      double2 x1, x2;
      s3_load(a, beg + j, A, B, x1, x2);
      const unsigned char in = s3_inlier(Q, M, A, B, x1, x2, thr2, f, bb) ? 1 : 0;
      a.cons[beg + j] = in;
      cn[0] += (double)in;
    }
    rs_block_sums<1>(cn, lds);
    if (!(cn[0] >= 3.0)) break;
    double acc[S3_NSUM], Mt[S3_MODEL];
    // the set's sums at the starting model, then (a): the closed form, kept if it lowers the set's cost
    s3_pass(a, M, a.cons, beg, n, acc, lds);
    hy_keep(s_cur, s_x, acc, M);
    if (s3_fit_set(a, beg, n, cn[0], Mt, lds)) {  // (workgroup-uniform: the sums are the same in every lane)
      s3_pass(a, Mt, a.cons, beg, n, acc, lds);
      if (acc[35] < s_cur[35]) hy_keep(s_cur, s_x, acc, Mt);
    }
    // (b): ba_resect's step 3 in the seven local parameters; a pass keeps only the trial model and its own sums in registers
    double lam = 1e-4;
    bool small = false;
    for (int it = 0; it < a.iters && !small; ++it) {
      double dx[7];
#pragma unroll
      for (int q = 0; q < S3_NSUM; ++q) acc[q] = s_cur[q];
      if (!lm_step(acc, lam, !a.with_scale, dx)) { status = S3_DEGENERATE; break; }
      double d2 = 0.0;
      bool fin = true;
#pragma unroll
      for (int q = 0; q < 7; ++q) { d2 += dx[q] * dx[q]; fin = fin && sim_finite(dx[q]); }
      if (!fin) { status = S3_DEGENERATE; break; }
#pragma unroll
      for (int q = 0; q < S3_MODEL; ++q) M[q] = s_x[q];
      s3_move(M, dx, Mt);
      small = sqrt(d2) <= 1e-14;
      s3_pass(a, Mt, a.cons, beg, n, acc, lds);
      if (acc[35] <= s_cur[35] * (1.0 + TRK_COST_SLACK)) {   // (workgroup-uniform)
        hy_keep(s_cur, s_x, acc, Mt);
        lam = fmax(0.1 * lam, 1e-12);
      } else {
        lam *= 10.0;
      }
    }
#pragma unroll
    for (int q = 0; q < S3_MODEL; ++q) M[q] = s_x[q];
  }
  // ---- measures at the final model
  s3_scaled(M, Q);
  double m2[2] = {0.0, 0.0};                      // inliers | sum (f + b)
  for (int j = tid; j < n; j += S3_THREADS) {
    double A[3], B[3], f, bb;
    double2 x1, x2;
    s3_load(a, beg + j, A, B, x1, x2);
    if (!s3_inlier(Q, M, A, B, x1, x2, thr2, f, bb)) continue;
    m2[0] += 1.0; m2[1] += f + bb;
    a.inl[beg + j] = 1;                           // (read back below by the lane that wrote it: same stride)
  }
  rs_block_sums<2>(m2, lds);
  const double rms = m2[0] > 0.0 ? a.fbar * sqrt(0.5 * m2[1] / m2[0]) : HY_NAN;
  if (status == S3_OK && m2[0] < (double)a.min_inliers) status = S3_FEW_INLIERS;
  // ---- fbar^2 J^T J of the final inlier set
  double acc[S3_NSUM];
  s3_pass(a, M, a.inl, beg, n, acc, lds);
  if (tid != 0) return;
  double rv[3];
  sim_log_map(M, rv);
  o[0] = rv[0]; o[1] = rv[1]; o[2] = rv[2]; o[3] = M[9]; o[4] = M[10]; o[5] = M[11]; o[6] = M[12];
  for (int q = 0; q < 9; ++q) o[7 + q] = M[q];
  o[16] = (double)status; o[17] = m2[0]; o[18] = rms; o[19] = (double)best;
  const double f2 = a.fbar * a.fbar;
  for (int q = 0; q < 28; ++q) o[20 + q] = f2 * acc[q];
}

}  // namespace ba
