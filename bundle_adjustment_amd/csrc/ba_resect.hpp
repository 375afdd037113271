// Resection (ba_resect): the pose of every selected camera from the points it sees, the points taken as known -- the
// mirror image of ba_triangulate_tracks (COLMAP's image registration, OpenMVG's resection, the tracking / relocalisation
// pose of ORB-SLAM).  Stand-alone kernels: they read the handle's camera-ordered observation list, point table and camera
// state, and none of the LM / Schur / PCG kernels.
//
// One 256-thread workgroup per camera; lanes stride over the camera's segment of the camera-ordered list.  Every sum is
// wave_total_dpp per wave, then the four wave results through LDS in wave order, read back by every lane: all lanes hold
// the same totals bit for bit, so every decision (eigenvector, pivots, step acceptance, status) is workgroup-uniform and
// the results are reproducible from call to call.  No atomics, no dynamic register indexing.
//
// Per camera, over its observations of known points whose bearing exists (n of them):
//   1 bearings    trk_bearing of ba_tracks.hpp: (x, y) with the ray (x, y, 1) up to sign, both models.
//   2 start       INIT_CURRENT: the handle's pose (n >= 3).  INIT_DLT (n >= 6): the rows x (p3.X~) - p1.X~ = 0,
//                 y (p3.X~) - p2.X~ = 0 with X~ = ((X - mean) / sigma, 1), sigma^2 = mean |X - mean|^2 / 3 from centred values.
//                 The 12 x 12 normal matrix is never formed: its blocks are S = sum X~X~^T, Sx = sum x X~X~^T, Sy, Sq =
//                 sum (x^2 + y^2) X~X~^T (forty sums, two passes of twenty), all divided by n; eliminating p1, p2 leaves
//                 M = Sq - Sx S^-1 Sx - Sy S^-1 Sy, p3 = its eigenvector of the smallest eigenvalue (jacobi_eig),
//                 p1 = S^-1 Sx p3, p2 = S^-1 Sy p3 through the Cholesky factor of S (a pivot <= 1e-8 -- coplanar, collinear
//                 or coincident points -- or a non-finite sum: DEGENERATE).  A = the left 3 x 3 of [p1; p2; p3], sign of P
//                 so that det A > 0, R = U V^T of A's SVD (jacobi_svd), t = b / mean(singular values), then
//                 t <- sigma t - R mean; sigma_3 <= 1e-6 sigma_1: DEGENERATE.  rvec = sim_log_map(R).
//   3 refinement  Marquardt-damped Gauss-Newton on 0.5 sum C^2 rho((r / C)^2) over the six additive parameters rvec | t:
//                 the model's pre-M Jacobian rows (jac_rows), summed, then the congruence with diag(M, I) (M = J_r(rvec) of
//                 camera_state) once per pass; IRLS weights of robust_loss; (H + lam diag H) dx = -g by a 6 x 6 Cholesky (a
//                 pivot <= 0: DEGENERATE with the last accepted pose); lam from 1e-4, / 10 (floor 1e-12) after a step that
//                 does not raise the cost (cost_trial <= cost (1 + 1e-12)), * 10 after one that does; |dx| <= 1e-14 |x| ends
//                 it.  An observation behind the camera at a pass's pose is left out of that pass's sums.
//   4 measures    at the final pose: inliers = observations in front with |r_i| <= max_reproj_px (every one in front when
//                 that is <= 0); rms and max over the inliers, or over all in front when there are none.
//   5 status      the first failing test in enum order (ba_resect_status).
#pragma once
#include "ba_linalg.hpp"
#include "ba_tracks.hpp"

namespace ba {

enum : int { RS_OK = 0, RS_FEW_POINTS = 1, RS_DEGENERATE = 2, RS_BEHIND = 3, RS_FEW_INLIERS = 4, RS_HIGH_ERROR = 5 };
enum : int { RS_INIT_DLT = 0, RS_INIT_CURRENT = 1 };
constexpr int RS_THREADS = 256;
constexpr int RS_WAVES = RS_THREADS / 64;
constexpr int RS_OUT = 10;         // doubles per camera: rvec | t | status | n_inliers | rms | max
constexpr int RS_NSUM = 28;        // a refinement pass: H (21) g (6) cost
constexpr double RS_PIVOT_MIN = 1e-8, RS_RANK_TOL = 1e-6;

struct ResectArgs {
  TrackArgs t;             // what trk_bearing and the passes read: cs, intr, uv (camera order), K4, loss, iters, fscale, max_px, min_depth
  const double* cams;      // rvec | t of the current parameter set
  const double* ptab;
  const int* offk;
  const int* c_pt;
  const unsigned char* known;   // per point slot, or null: every point
  const unsigned char* sel;     // per camera, or null: every camera
  int init, min_inliers;
  double max_rms;
  double* out;             // RS_OUT doubles per camera
};

// pt_known of the caller's point order -> point-slot order
__global__ void k_resect_known(const unsigned char* __restrict__ in, const int* __restrict__ slot, int n_pts, unsigned char* __restrict__ out) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p < n_pts) out[slot[p]] = in[p];
}

// v[0 .. N) summed over the workgroup, the totals in every lane
template <int N>
__device__ __forceinline__ void rs_block_sums(double (&v)[N], double* __restrict__ lds) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  __syncthreads();                               // (the readers of the previous sums are done)
#pragma unroll
  for (int j = 0; j < N; ++j) {
    const double t = wave_total_dpp(v[j]);
    if (lane == 0) lds[wv * N + j] = t;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < N; ++j) v[j] = ((lds[j] + lds[N + j]) + lds[2 * N + j]) + lds[3 * N + j];
}
__device__ __forceinline__ double rs_block_max(double x, double* __restrict__ lds) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  x = wave_max_dpp(x);
  __syncthreads();
  if (lane == 0) lds[wv] = x;
  __syncthreads();
  return fmax(fmax(lds[0], lds[1]), fmax(lds[2], lds[3]));
}

// observation j of the camera: false when its point is not known or its bearing fails
template <class CM>
__device__ __forceinline__ bool rs_obs(const ResectArgs& a, const double (&cam)[CM::CAM], const int j, double (&X)[3], double2& uv,
                                       double& bx, double& by) {
  const int p = a.c_pt[j];
  if (a.known && !a.known[p]) return false;
  const double4 Xd = *(const double4*)(a.ptab + PT * (size_t)p);
  X[0] = Xd.x; X[1] = Xd.y; X[2] = Xd.z;
  uv = a.t.uv[(size_t)j];
  return trk_bearing<CM>(cam, uv, a.t, bx, by);
}

// observation j at the pose in cam: 0 when it is not usable (rs_obs), -1 when its point is behind the camera, 1 when it is in
// front, with its residual and what the Jacobian rows are made of
template <class CM>
__device__ __forceinline__ int rs_residual(const ResectArgs& a, const double (&cam)[CM::CAM], const int j, double& ru, double& rv,
                                           double2& uv, double (&X)[3], typename CM::template Obs<double>& g) {
  double bx, by;
  if (!rs_obs<CM>(a, cam, j, X, uv, bx, by)) return 0;
  const double pz = cam[6] * X[0] + cam[7] * X[1] + cam[8] * X[2] + cam[11];
  if (!((CM::ID == 0 ? pz : -pz) > a.t.min_depth)) return -1;
  CM::template geom<false, double, double>(cam, X[0], X[1], X[2], a.t.fx, a.t.fy, g);
  CM::residual(g, uv.x, uv.y, a.t.fx, a.t.fy, a.t.cx, a.t.cy, ru, rv);
  return 1;
}

// The start of step 2 from the forty sums (sa: S | Sx, sb: Sy | Sq, packed upper 4 x 4 each); false: DEGENERATE
__device__ inline bool rs_dlt_pose(const double (&sa)[20], const double (&sb)[20], const double n, const double (&mean)[3],
                                   const double sigma, double (&x)[6]) {
  const double in = 1.0 / n;
  double S[4][4], Sx[4][4], Sy[4][4], Mq[4][4];
  bool ok = sim_finite(sigma);
#pragma unroll
  for (int q = 0; q < 20; ++q) ok = ok && sim_finite(sa[q]) && sim_finite(sb[q]);
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      S[p][q] = sa[ST(4, p, q)] * in; Sx[p][q] = sa[10 + ST(4, p, q)] * in;
      Sy[p][q] = sb[ST(4, p, q)] * in; Mq[p][q] = sb[10 + ST(4, p, q)] * in;
    }
  // S = L L^T
  double L[4][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    double s = S[j][j];
#pragma unroll
    for (int k = 0; k < 4; ++k) if (k < j) s -= L[j][k] * L[j][k];
    ok = ok && (s > RS_PIVOT_MIN);
    const double l = sqrt(s);
    L[j][j] = l;
#pragma unroll
    for (int i = 0; i < 4; ++i) if (i > j) {
      double t = S[i][j];
#pragma unroll
      for (int k = 0; k < 4; ++k) if (k < j) t -= L[i][k] * L[j][k];
      L[i][j] = t / l;
    }
  }
  if (!ok) return false;
  // Wx = L^-1 Sx, Wy = L^-1 Sy;  M = Sq - Wx^T Wx - Wy^T Wy
  double Wx[4][4], Wy[4][4];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      double tx = Sx[i][q], ty = Sy[i][q];
#pragma unroll
      for (int k = 0; k < 4; ++k) if (k < i) { tx -= L[i][k] * Wx[k][q]; ty -= L[i][k] * Wy[k][q]; }
      Wx[i][q] = tx / L[i][i]; Wy[i][q] = ty / L[i][i];
    }
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < 4; ++k) s += Wx[k][p] * Wx[k][q] + Wy[k][p] * Wy[k][q];
      Mq[p][q] -= s;
    }
  double V[4][4];
  jacobi_eig<4, 16>(Mq, V);
  int best = 0;
  double lo = Mq[0][0];
  if (Mq[1][1] < lo) { lo = Mq[1][1]; best = 1; }
  if (Mq[2][2] < lo) { lo = Mq[2][2]; best = 2; }
  if (Mq[3][3] < lo) { lo = Mq[3][3]; best = 3; }
  double P[3][4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {           // (selection without dynamic register indexing)
    P[2][k] = V[k][0];
    if (best == 1) P[2][k] = V[k][1];
    if (best == 2) P[2][k] = V[k][2];
    if (best == 3) P[2][k] = V[k][3];
  }
  // p1 = L^-T (Wx p3), p2 = L^-T (Wy p3)
  double ux[4], uy[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    ux[i] = Wx[i][0] * P[2][0] + Wx[i][1] * P[2][1] + Wx[i][2] * P[2][2] + Wx[i][3] * P[2][3];
    uy[i] = Wy[i][0] * P[2][0] + Wy[i][1] * P[2][1] + Wy[i][2] * P[2][2] + Wy[i][3] * P[2][3];
  }
#pragma unroll
  for (int i = 3; i >= 0; --i) {
    double tx = ux[i], ty = uy[i];
#pragma unroll
    for (int k = 0; k < 4; ++k) if (k > i) { tx -= L[k][i] * P[0][k]; ty -= L[k][i] * P[1][k]; }
    P[0][i] = tx / L[i][i]; P[1][i] = ty / L[i][i];
  }
  const double det = P[0][0] * (P[1][1] * P[2][2] - P[1][2] * P[2][1]) - P[0][1] * (P[1][0] * P[2][2] - P[1][2] * P[2][0]) +
                     P[0][2] * (P[1][0] * P[2][1] - P[1][1] * P[2][0]);
  const double sg = det < 0.0 ? -1.0 : 1.0;
  double U[3][3], W[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) U[i][j] = sg * P[i][j];
  jacobi_svd<3, 24>(U, W);
  double n2[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) n2[k] = U[0][k] * U[0][k] + U[1][k] * U[1][k] + U[2][k] * U[2][k];
  sim_order<0, 1>(U, W, n2); sim_order<1, 2>(U, W, n2); sim_order<0, 1>(U, W, n2);
  const double d0 = sqrt(n2[0]), d1 = sqrt(n2[1]), d2 = sqrt(n2[2]);
  if (!(d2 > RS_RANK_TOL * d0)) return false;
  double R[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) R[3 * i + j] = (U[i][0] / d0) * W[j][0] + (U[i][1] / d1) * W[j][1] + (U[i][2] / d2) * W[j][2];
  const double sm = (d0 + d1 + d2) / 3.0;
  sim_log_map(R, x);
#pragma unroll
  for (int i = 0; i < 3; ++i)
    x[3 + i] = sigma * (sg * P[i][3] / sm) - (R[3 * i] * mean[0] + R[3 * i + 1] * mean[1] + R[3 * i + 2] * mean[2]);
#pragma unroll
  for (int q = 0; q < 6; ++q) ok = ok && sim_finite(x[q]);
  return ok;
}

// camera state of the pose x into cam (R | t; the intrinsics of a BAL camera stay) and M
template <class CM>
__device__ __forceinline__ void rs_pose(const double (&x)[6], double (&cam)[CM::CAM], double (&M)[9]) {
  double st[CS];
  camera_state(x, st);
#pragma unroll
  for (int q = 0; q < 12; ++q) cam[q] = st[q];
#pragma unroll
  for (int q = 0; q < 9; ++q) M[q] = st[12 + q];
}

// the sums of a refinement pass at the pose in cam / M: H, g (in the additive coordinates rvec | t) and the cost.  CONS (the
// local optimisation of ba_ransac.hpp): over the observations j with cons[j] != 0 only; ba_resect's own passes have no such test
template <class CM, bool CONS = false>
__device__ __forceinline__ void rs_pass(const ResectArgs& a, const double (&cam)[CM::CAM], const double (&M)[9], const int beg,
                                        const int end, double (&acc)[RS_NSUM], double* __restrict__ lds,
                                        const unsigned char* __restrict__ cons = nullptr) {
#pragma unroll
  for (int q = 0; q < RS_NSUM; ++q) acc[q] = 0.0;
  for (int j = beg + (int)threadIdx.x; j < end; j += RS_THREADS) {
    if constexpr (CONS) { if (!cons[j]) continue; }
    double X[3], ru, rv;
    double2 uv;
    typename CM::template Obs<double> g;
    if (rs_residual<CM>(a, cam, j, ru, rv, uv, X, g) <= 0) continue;
    double J0[CM::NB], J1[CM::NB];
    CM::jac_rows(g, X[0], X[1], X[2], J0, J1);
    double w0 = 1.0, w1 = 1.0, t0 = ru * ru, t1 = rv * rv;
    if (a.t.loss != LOSS_LINEAR) {
      robust_loss<true>(a.t.loss, ru, a.t.fscale, t0, w0);
      robust_loss<true>(a.t.loss, rv, a.t.fscale, t1, w1);
    }
#pragma unroll
    for (int p = 0; p < 6; ++p) {
      const double wa0 = w0 * J0[p], wa1 = w1 * J1[p];
#pragma unroll
      for (int q = p; q < 6; ++q) acc[U6(p, q)] += wa0 * J0[q] + wa1 * J1[q];
      acc[21 + p] += wa0 * ru + wa1 * rv;
    }
    acc[27] += t0 + t1;
  }
  rs_block_sums<RS_NSUM>(acc, lds);
  // J = J_preM diag(M, I):  H <- D^T H D, g <- D^T g
  double T[6][6];
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int b = 0; b < 6; ++b)
      T[i][b] = b < 3 ? acc[S6(i, 0)] * M[b] + acc[S6(i, 1)] * M[3 + b] + acc[S6(i, 2)] * M[6 + b] : acc[S6(i, b)];
  double g3[3];
#pragma unroll
  for (int b = 0; b < 3; ++b) g3[b] = M[b] * acc[21] + M[3 + b] * acc[22] + M[6 + b] * acc[23];
#pragma unroll
  for (int p = 0; p < 6; ++p)
#pragma unroll
    for (int q = p; q < 6; ++q)
      acc[U6(p, q)] = p < 3 ? M[p] * T[0][q] + M[3 + p] * T[1][q] + M[6 + p] * T[2][q] : T[p][q];
#pragma unroll
  for (int b = 0; b < 3; ++b) acc[21 + b] = g3[b];
}

// a camera without a refinement (not selected, or failed before it): the pose x, no measures
__device__ __forceinline__ void rs_write_unrefined(double* __restrict__ o, const double (&x)[6], const int status) {
  if (threadIdx.x != 0) return;
  for (int q = 0; q < 6; ++q) o[q] = x[q];
  o[6] = (double)status; o[7] = 0.0; o[8] = HY_NAN; o[9] = HY_NAN;
}

// step 3 from the pose x, which ends as the last accepted one; status becomes DEGENERATE on a failed pivot.  CONS: as rs_pass
template <class CM, bool CONS>
__device__ __forceinline__ void rs_refine(const ResectArgs& a, double (&cam)[CM::CAM], double (&M)[9], const int beg, const int end,
                                          double (&x)[6], int& status, double* __restrict__ lds,
                                          const unsigned char* __restrict__ cons = nullptr) {
  double acc[RS_NSUM], cur[RS_NSUM], xt[6];
#pragma unroll
  for (int q = 0; q < 6; ++q) xt[q] = x[q];
#pragma unroll
  for (int q = 0; q < RS_NSUM; ++q) cur[q] = 0.0;
  double lam = 1e-4;
  bool first = true, small = false;
  int it = 0;
  for (;;) {
    rs_pose<CM>(xt, cam, M);
    rs_pass<CM, CONS>(a, cam, M, beg, end, acc, lds, cons);
    if (first || acc[27] <= cur[27] * (1.0 + TRK_COST_SLACK)) {
#pragma unroll
      for (int q = 0; q < RS_NSUM; ++q) cur[q] = acc[q];
#pragma unroll
      for (int q = 0; q < 6; ++q) x[q] = xt[q];
      if (!first) lam = fmax(0.1 * lam, 1e-12);
    } else {
      lam *= 10.0;
    }
    first = false;
    if (small || it >= a.t.iters) break;
    ++it;
    double dx[6];
    if (!lm_step(cur, lam, false, dx)) { status = RS_DEGENERATE; break; }
    double d2 = 0.0, x2 = 0.0;
#pragma unroll
    for (int q = 0; q < 6; ++q) { xt[q] = x[q] + dx[q]; d2 += dx[q] * dx[q]; x2 += x[q] * x[q]; }
    small = sqrt(d2) <= 1e-14 * sqrt(x2);
  }
}

// steps 4 and 5 at the final pose x of a camera with n usable observations, and its output row.  inl (ba_resect_ransac's
// obs_inlier, else null): the inliers' bytes, through c_orig in the caller's order
template <class CM>
__device__ __forceinline__ void rs_finish(const ResectArgs& a, double (&cam)[CM::CAM], double (&M)[9], const int beg, const int end,
                                          const double (&x)[6], const double n, int status, double* __restrict__ lds,
                                          double* __restrict__ o, unsigned char* __restrict__ inl, const int* __restrict__ c_orig) {
  rs_pose<CM>(x, cam, M);
  double m5[5] = {0, 0, 0, 0, 0};     // in front | behind | inliers | sse of the inliers | sse of those in front
  double mx_in = 0.0, mx_fr = 0.0;
  for (int j = beg + (int)threadIdx.x; j < end; j += RS_THREADS) {
    double X[3], ru, rv;
    double2 uv;
    typename CM::template Obs<double> g;
    const int front = rs_residual<CM>(a, cam, j, ru, rv, uv, X, g);
    if (front < 0) m5[1] += 1.0;
    if (front <= 0) continue;
    const double e2 = ru * ru + rv * rv;
    m5[0] += 1.0; m5[4] += e2;
    mx_fr = fmax(mx_fr, e2);
    if (!(a.t.max_px > 0.0) || sqrt(e2) <= a.t.max_px) {
      m5[2] += 1.0; m5[3] += e2; mx_in = fmax(mx_in, e2);
      if (inl) inl[c_orig[j]] = 1;
    }
  }
  rs_block_sums<5>(m5, lds);
  mx_in = rs_block_max(mx_in, lds);
  mx_fr = rs_block_max(mx_fr, lds);
  if (threadIdx.x == 0) {
    const bool any_in = m5[2] > 0.0;
    const double cnt = any_in ? m5[2] : m5[0];
    const double rms = cnt > 0.0 ? sqrt((any_in ? m5[3] : m5[4]) / cnt) : HY_NAN;
    const double emax = cnt > 0.0 ? sqrt(any_in ? mx_in : mx_fr) : HY_NAN;
    if (status == RS_OK) {
      if (2.0 * m5[1] > n) status = RS_BEHIND;
      else if (m5[2] < (double)a.min_inliers) status = RS_FEW_INLIERS;
      else if (a.max_rms > 0.0 && !(rms <= a.max_rms)) status = RS_HIGH_ERROR;
    }
    for (int q = 0; q < 6; ++q) o[q] = x[q];
    o[6] = (double)status; o[7] = m5[2]; o[8] = rms; o[9] = emax;
  }
}

template <class CM>
__global__ void __launch_bounds__(RS_THREADS) k_resect(const ResectArgs a) {
  __shared__ double lds[RS_WAVES * RS_NSUM];
  const int c = blockIdx.x, tid = threadIdx.x;
  double* o = a.out + RS_OUT * (size_t)c;
  double x[6];
#pragma unroll
  for (int q = 0; q < 6; ++q) x[q] = a.cams[6 * (size_t)c + q];
  if (a.sel && !a.sel[c]) { rs_write_unrefined(o, x, RS_OK); return; }   // (workgroup-uniform, like every branch below)
  const int beg = a.offk[c * (NPART + 1)], end = a.offk[c * (NPART + 1) + NPART];
  double cam[CM::CAM], M[9];
  CM::load_cam_vec(a.t.cs, a.t.intr, c, cam);
  // n and the mean of the points
  double s4[4] = {0, 0, 0, 0};
  for (int j = beg + tid; j < end; j += RS_THREADS) {
    double X[3], bx, by;
    double2 uv;
    if (!rs_obs<CM>(a, cam, j, X, uv, bx, by)) continue;
    s4[0] += 1.0; s4[1] += X[0]; s4[2] += X[1]; s4[3] += X[2];
  }
  rs_block_sums<4>(s4, lds);
  const double n = s4[0];
  int status = RS_OK;
  if (n < (a.init == RS_INIT_DLT ? 6.0 : 3.0)) status = RS_FEW_POINTS;
  else if (a.init == RS_INIT_DLT) {
    const double mean[3] = {s4[1] / n, s4[2] / n, s4[3] / n};
    double v1[1] = {0.0};
    for (int j = beg + tid; j < end; j += RS_THREADS) {
      double X[3], bx, by;
      double2 uv;
      if (!rs_obs<CM>(a, cam, j, X, uv, bx, by)) continue;
      const double e0 = X[0] - mean[0], e1 = X[1] - mean[1], e2 = X[2] - mean[2];
      v1[0] += e0 * e0 + e1 * e1 + e2 * e2;
    }
    rs_block_sums<1>(v1, lds);
    const double sigma = sqrt(v1[0] / (3.0 * n)), isg = 1.0 / sigma;
    double sa[20], sb[20];
#pragma unroll
    for (int q = 0; q < 20; ++q) { sa[q] = 0.0; sb[q] = 0.0; }
    for (int j = beg + tid; j < end; j += RS_THREADS) {      // S | Sx
      double X[3], bx, by;
      double2 uv;
      if (!rs_obs<CM>(a, cam, j, X, uv, bx, by)) continue;
      const double Xt[4] = {(X[0] - mean[0]) * isg, (X[1] - mean[1]) * isg, (X[2] - mean[2]) * isg, 1.0};
#pragma unroll
      for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = p; q < 4; ++q) {
          const double xx = Xt[p] * Xt[q];
          sa[UT(4, p, q)] += xx;
          sa[10 + UT(4, p, q)] += bx * xx;
        }
    }
    rs_block_sums<20>(sa, lds);
    for (int j = beg + tid; j < end; j += RS_THREADS) {      // Sy | Sq
      double X[3], bx, by;
      double2 uv;
      if (!rs_obs<CM>(a, cam, j, X, uv, bx, by)) continue;
      const double Xt[4] = {(X[0] - mean[0]) * isg, (X[1] - mean[1]) * isg, (X[2] - mean[2]) * isg, 1.0};
      const double qq = bx * bx + by * by;
#pragma unroll
      for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = p; q < 4; ++q) {
          const double xx = Xt[p] * Xt[q];
          sb[UT(4, p, q)] += by * xx;
          sb[10 + UT(4, p, q)] += qq * xx;
        }
    }
    rs_block_sums<20>(sb, lds);
    double xs[6];
    if (rs_dlt_pose(sa, sb, n, mean, sigma, xs)) {
#pragma unroll
      for (int q = 0; q < 6; ++q) x[q] = xs[q];
    } else {
      status = RS_DEGENERATE;
    }
  }
  if (status != RS_OK) { rs_write_unrefined(o, x, status); return; }   // the current pose
  rs_refine<CM, false>(a, cam, M, beg, end, x, status, lds);
  rs_finish<CM>(a, cam, M, beg, end, x, n, status, lds, o, nullptr, nullptr);
}

// write_cams: the cameras and the point table ba_set_params would build from the merged cameras and the current points
// (a camera takes its resected pose when it is selected, OK, not fixed_cam and has none of its six pose parameters held;
// the table's other words start at 0 as they do there).  cams_cur / cams0 and ptab_cur / ptab0 may be the same arrays.
__global__ void k_resect_merge(const double* __restrict__ out, const unsigned char* __restrict__ sel, const unsigned short* __restrict__ held,
                               int fixed_cam, const double* cams_cur, int n_cams, double* cams0, const double* ptab_cur, int n_pts,
                               double* ptab0) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_cams) {
    const double* r = out + RS_OUT * (size_t)i;
    const bool take = (!sel || sel[i]) && (int)r[6] == RS_OK && i != fixed_cam && !(held && (held[i] & 0x3f));
    const double* src = take ? r : cams_cur + 6 * (size_t)i;
    double v[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) v[q] = src[q];
#pragma unroll
    for (int q = 0; q < 6; ++q) cams0[6 * (size_t)i + q] = v[q];
  }
  if (i < n_pts) {
    const double* s = ptab_cur + PT * (size_t)i;
    const double X0 = s[0], X1 = s[1], X2 = s[2];
    double* d = ptab0 + PT * (size_t)i;
    d[0] = X0; d[1] = X1; d[2] = X2;
    d[3] = 0; d[4] = 0; d[5] = 0; d[6] = 0; d[7] = 0;
  }
}

}  // namespace ba
