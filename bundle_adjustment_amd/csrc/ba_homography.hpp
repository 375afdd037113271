// Two-view homography (ba_homography): the plane-induced H of raw pixel matches, a share of which may be wrong, and the two
// poses R | t | n it decomposes into -- the planar model next to ba_relative_pose's essential one (ORB-SLAM's initialiser and
// COLMAP's two-view geometry estimate both).  Stand-alone kernels: they read the call's own staging buffers and nothing of a
// resident problem.  Conventions of ba_relpose.hpp: x2~ ~ H~ x1~, H~ / d2 = R + (t / d) n^T, x2 ~ K (R x1 + t), |t| = |n| = 1.
//
// Two launches per call, for all pairs at once:
//   k_homog_score  grid (pairs, ceil(n_hyp / 256)): lane = hypothesis.  Sample -> closed form (3 x 3 cofactors indexed by
//                  constants: H~ and adj H~ in 18 registers) -> the pair's normalised matches stream through LDS
//                  in tiles of HY_TILE (x1 | x2); MSAC cost of the symmetric transfer error; the block's lowest (cost, h) by hy_block_best.
//   k_homog_lo     one workgroup per pair: the lowest (cost, h) over the score blocks, lo_rounds of {consensus bytes;
//                  Marquardt-damped Gauss-Newton in the eight entries of the traceless D of H (I + D)}, the measures, the pixel
//                  H, H~ = U diag V^T (hy_canon_svd), the two poses with their votes and Sampson costs, the status.  The last
//                  accepted H~ and its 45 sums live in LDS.  Sums by rs_block_sums: fixed order, no atomics.
#pragma once
#include "ba_relpose.hpp"

namespace ba {

enum : int { HG_OK = 0, HG_FEW_MATCHES = 1, HG_DEGENERATE = 2, HG_FEW_INLIERS = 3, HG_ROTATION = 4, HG_AMBIGUOUS = 5 };
constexpr int HG_THREADS = HY_THREADS;
constexpr int HG_BEST = 12;                    // doubles per (pair, score block): cost | h | H~[9] | one of padding (a block's record stays 16-byte aligned, as RP_BEST)
constexpr int HG_OUT = 50;                     // doubles per pair: H[9] | status n_inliers rms best_hyp n_pose | R[18] | t[6] | n[6] | t/d[2] | votes[2] | cost[2]
constexpr int HG_NSUM = 45;                    // a refinement pass: H (36) g (8) cost
constexpr double HG_DET_TOL = 1e-12;
static_assert(HG_THREADS == RS_THREADS, "rs_block_sums folds RS_WAVES waves");

struct HomogArgs : PairArgs {   // thr = max_px / fbar; best: HG_BEST doubles per (pair, score block); out: HG_OUT per pair
  double ambiguity, min_translation;
};

// ---------------------------------------------------------------------------------------------- 3 x 3, row-major, in registers
__device__ __forceinline__ void hg_adj(const double (&A)[9], double (&C)[9]) {
  C[0] = A[4] * A[8] - A[5] * A[7]; C[1] = A[2] * A[7] - A[1] * A[8]; C[2] = A[1] * A[5] - A[2] * A[4];
  C[3] = A[5] * A[6] - A[3] * A[8]; C[4] = A[0] * A[8] - A[2] * A[6]; C[5] = A[2] * A[3] - A[0] * A[5];
  C[6] = A[3] * A[7] - A[4] * A[6]; C[7] = A[1] * A[6] - A[0] * A[7]; C[8] = A[0] * A[4] - A[1] * A[3];
}
__device__ __forceinline__ void hg_mul(const double (&A)[9], const double (&B)[9], double (&C)[9]) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}
// unit Frobenius norm and det > 0; det comes back as |det| at unit norm.  false: not finite
__device__ __forceinline__ bool hg_unit(double (&H)[9], double& det) {
  double n2 = 0.0;
#pragma unroll
  for (int q = 0; q < 9; ++q) n2 += H[q] * H[q];
  const double in = 1.0 / sqrt(n2);
#pragma unroll
  for (int q = 0; q < 9; ++q) H[q] *= in;
  det = H[0] * (H[4] * H[8] - H[5] * H[7]) + H[1] * (H[5] * H[6] - H[3] * H[8]) + H[2] * (H[3] * H[7] - H[4] * H[6]);
  if (det < 0.0) {
    det = -det;
#pragma unroll
    for (int q = 0; q < 9; ++q) H[q] = -H[q];
  }
  return sim_finite(in) && sim_finite(det) && n2 > 0.0;
}
__device__ __forceinline__ void hg_identity(double (&H)[9]) {
#pragma unroll
  for (int q = 0; q < 9; ++q) H[q] = (q % 4 == 0) ? 1.0 : 0.0;
}
// a triple with |d12 x d13| <= HY_AREA_TOL max |d_ij|^2 (collinear or coincident)
__device__ __forceinline__ bool hg_flat(const double2 p, const double2 q, const double2 r) {
  const double ax = q.x - p.x, ay = q.y - p.y, bx = r.x - p.x, by = r.y - p.y, cx = r.x - q.x, cy = r.y - q.y;
  const double ext = fmax(fmax(ax * ax + ay * ay, bx * bx + by * by), cx * cx + cy * cy);
  return !(fabs(ax * by - ay * bx) > HY_AREA_TOL * ext) || !sim_finite(ext);
}
__device__ __forceinline__ bool hg_flat4(const double2 (&s)[4]) {
  return hg_flat(s[0], s[1], s[2]) || hg_flat(s[0], s[1], s[3]) || hg_flat(s[0], s[2], s[3]) || hg_flat(s[1], s[2], s[3]);
}
// B = M diag(adj(M) d), M = [a b c] in homogeneous columns: B maps e_k to a multiple of the k-th point and (1, 1, 1) to det(M) d
__device__ __forceinline__ void hg_basis(const double2 (&s)[4], double (&B)[9]) {
  const double M[9] = {s[0].x, s[1].x, s[2].x, s[0].y, s[1].y, s[2].y, 1.0, 1.0, 1.0};
  double C[9];
  hg_adj(M, C);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double lam = C[3 * k] * s[3].x + C[3 * k + 1] * s[3].y + C[3 * k + 2];
    B[k] = M[k] * lam; B[3 + k] = M[3 + k] * lam; B[6 + k] = lam;
  }
}
// step 3: H~ = B2 adj(B1) at unit norm and det > 0; false: a void sample
__device__ __forceinline__ bool hg_solve(const double2 (&s1)[4], const double2 (&s2)[4], double (&H)[9]) {
  if (hg_flat4(s1) || hg_flat4(s2)) return false;
  double B1[9], B2[9], C[9], det;
  hg_basis(s1, B1);
  hg_basis(s2, B2);
  hg_adj(B1, C);
  hg_mul(B2, C, H);
  if (!hg_unit(H, det) || !(det > HG_DET_TOL)) return false;
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 4; ++k) ok = ok && (H[6] * s1[k].x + H[7] * s1[k].y + H[8] > 0.0);
  return ok;
}
// squared forward and backward transfer errors of (x1, x2) at H~ and A = adj H~ (a positive multiple of the inverse: det > 0);
// pf / pb: the third component is positive
__device__ __forceinline__ void hg_transfer(const double (&H)[9], const double (&A)[9], const double2 x1, const double2 x2, double& f, double& b,
                                            bool& pf, bool& pb) {
  const double yw = H[6] * x1.x + H[7] * x1.y + H[8], zw = A[6] * x2.x + A[7] * x2.y + A[8];
  const double iy = 1.0 / yw, iz = 1.0 / zw;
  const double f0 = (H[0] * x1.x + H[1] * x1.y + H[2]) * iy - x2.x, f1 = (H[3] * x1.x + H[4] * x1.y + H[5]) * iy - x2.y;
  const double b0 = (A[0] * x2.x + A[1] * x2.y + A[2]) * iz - x1.x, b1 = (A[3] * x2.x + A[4] * x2.y + A[5]) * iz - x1.y;
  f = f0 * f0 + f1 * f1; b = b0 * b0 + b1 * b1;
  pf = yw > 0.0; pb = zw > 0.0;
}
__device__ __forceinline__ bool hg_inlier(const double (&H)[9], const double (&A)[9], const double2 x1, const double2 x2, const double thr2, double& f, double& b) {
  bool pf, pb;
  hg_transfer(H, A, x1, x2, f, b, pf, pb);
  return pf && pb && f <= thr2 && b <= thr2;
}

// ------------------------------------------------------------------------------------------------ hypotheses and scores
__global__ void __launch_bounds__(HG_THREADS) k_homog_score(const HomogArgs a) {
  __shared__ double tile[HY_TILE * 4];
  __shared__ double red[2 * HY_WAVES];
  const int pair = blockIdx.x, blk = blockIdx.y, tid = threadIdx.x;
  const long long beg = a.off[pair];
  const int n = (int)(a.off[pair + 1] - beg);
  double* out = a.best + HG_BEST * ((size_t)pair * a.n_blk + blk);
  if (n < 5) {                                    // (workgroup-uniform) FEW_MATCHES
    hy_void_block(out);
    return;
  }
  const int h = blk * HG_THREADS + tid;
  bool valid = h < a.n_hyp;
  double H[9], A[9];
  {
    int idx[4];
    hy_sample(a.seed, pair, valid ? h : 0, n, idx);   // (indices below n for every lane)
    double2 s1[4], s2[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) { s1[k] = pv_norm(a, a.p1[beg + idx[k]]); s2[k] = pv_norm(a, a.p2[beg + idx[k]]); }
    valid = hg_solve(s1, s2, H) && valid;
  }
  if (!valid) hg_identity(H);                     // a void hypothesis runs along on finite numbers
  hg_adj(H, A);
  const double thr2 = a.thr * a.thr;
  double cost = 0.0;
  for (int i0 = 0; i0 < n; i0 += HY_TILE) {
    const int m = min(HY_TILE, n - i0);
    __syncthreads();                              // (the readers of the previous tile are done)
    if (tid < m) {
      double2* d = (double2*)(tile + 4 * tid);
      d[0] = pv_norm(a, a.p1[beg + i0 + tid]); d[1] = pv_norm(a, a.p2[beg + i0 + tid]);
    }
    __syncthreads();
    for (int i = 0; i < m; ++i) {                 // every lane reads the same address: an LDS broadcast
      const double2* s = (const double2*)(tile + 4 * i);
      double f, b;
      bool pf, pb;
      hg_transfer(H, A, s[0], s[1], f, b, pf, pb);
      cost += (pf ? fmin(f, thr2) : thr2) + (pb ? fmin(b, thr2) : thr2);
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
    for (int q = 0; q < 9; ++q) out[2 + q] = H[q];
  }
}

// ------------------------------------------------------------------------------------------------ LO, measures, decomposition
// The sums of a refinement pass over the consensus set at H~: the 8 x 8 normal matrix, the gradient and 0.5 sum (|r_f|^2 + |r_b|^2)
// in the entries p0 .. p7 of D = [p0 p1 p2; p3 p4 p5; p6 p7 -(p0 + p4)].  Forward: d pi(H (I + D) x1~) = J_pi(y) H (D x1~), y = H x1~;
// backward, to first order: d pi((I - D) z) = -J_pi(z) (D z), z = adj(H) x2~ (any positive multiple of H^-1 x2~ projects alike).
// A consensus match whose third component is not positive at this H~ makes the cost infinite: leaving it out would lower the
// cost, and the acceptance test would then favour a step that pushes matches behind the camera.  It cannot happen at a round's
// starting H~ (the consensus test asks for both components positive), so it only ever rejects a trial.
__device__ __forceinline__ void hg_pass(const HomogArgs& a, const double (&H)[9], const long long beg, const int n, double (&acc)[HG_NSUM],
                                        double* __restrict__ lds) {
  double A[9];
  hg_adj(H, A);
#pragma unroll
  for (int q = 0; q < HG_NSUM; ++q) acc[q] = 0.0;
  for (int j = (int)threadIdx.x; j < n; j += HG_THREADS) {
    if (!a.cons[beg + j]) continue;
    const double2 x1 = pv_norm(a, a.p1[beg + j]), x2 = pv_norm(a, a.p2[beg + j]);
    const double yw = H[6] * x1.x + H[7] * x1.y + H[8], zw = A[6] * x2.x + A[7] * x2.y + A[8];
    if (!(yw > 0.0 && zw > 0.0)) { acc[44] = HY_INF; continue; }   // (HY_INF + anything finite stays above every accepted cost)
    const double iy = 1.0 / yw, iz = 1.0 / zw;
    const double px = (H[0] * x1.x + H[1] * x1.y + H[2]) * iy, py = (H[3] * x1.x + H[4] * x1.y + H[5]) * iy;
    const double qx = (A[0] * x2.x + A[1] * x2.y + A[2]) * iz, qy = (A[3] * x2.x + A[4] * x2.y + A[5]) * iz;
    const double r[4] = {px - x2.x, py - x2.y, qx - x1.x, qy - x1.y};
    double J[4][8];
    {
      const double g00 = (H[0] - px * H[6]) * iy, g01 = (H[1] - px * H[7]) * iy, g02 = (H[2] - px * H[8]) * iy;
      const double g10 = (H[3] - py * H[6]) * iy, g11 = (H[4] - py * H[7]) * iy, g12 = (H[5] - py * H[8]) * iy;
      J[0][0] = g00 * x1.x - g02; J[0][1] = g00 * x1.y; J[0][2] = g00; J[0][3] = g01 * x1.x; J[0][4] = g01 * x1.y - g02; J[0][5] = g01;
      J[0][6] = g02 * x1.x; J[0][7] = g02 * x1.y;
      J[1][0] = g10 * x1.x - g12; J[1][1] = g10 * x1.y; J[1][2] = g10; J[1][3] = g11 * x1.x; J[1][4] = g11 * x1.y - g12; J[1][5] = g11;
      J[1][6] = g12 * x1.x; J[1][7] = g12 * x1.y;
      J[2][0] = -2.0 * qx; J[2][1] = -qy; J[2][2] = -1.0; J[2][3] = 0.0; J[2][4] = -qx; J[2][5] = 0.0; J[2][6] = qx * qx; J[2][7] = qx * qy;
      J[3][0] = -qy; J[3][1] = 0.0; J[3][2] = 0.0; J[3][3] = -qx; J[3][4] = -2.0 * qy; J[3][5] = -1.0; J[3][6] = qx * qy; J[3][7] = qy * qy;
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
#pragma unroll
      for (int s2 = q; s2 < 8; ++s2) acc[UT(8, q, s2)] += (J[0][q] * J[0][s2] + J[1][q] * J[1][s2]) + (J[2][q] * J[2][s2] + J[3][q] * J[3][s2]);
      acc[36 + q] += (J[0][q] * r[0] + J[1][q] * r[1]) + (J[2][q] * r[2] + J[3][q] * r[3]);
    }
    acc[44] += 0.5 * ((r[0] * r[0] + r[1] * r[1]) + (r[2] * r[2] + r[3] * r[3]));
  }
  rs_block_sums<HG_NSUM>(acc, lds);
}

// H (I + D) exactly, renormalised.  hg_unit's verdict is not needed: a Y that is not finite fails every yw > 0 in hg_pass, the
// trial's cost is infinite and the step is rejected
__device__ __forceinline__ void hg_move(const double (&H)[9], const double (&p)[8], double (&Y)[9]) {
  const double D[9] = {p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], -(p[0] + p[4])};
  hg_mul(H, D, Y);
#pragma unroll
  for (int q = 0; q < 9; ++q) Y[q] += H[q];
  double det;
  hg_unit(Y, det);
}

// a pair without a homography: H = I, no pose
__device__ __forceinline__ void hg_void(double* __restrict__ o, const int status) {
  if (threadIdx.x != 0) return;
  for (int q = 0; q < HG_OUT; ++q) o[q] = 0.0;
  for (int q = 0; q < 9; ++q) o[q] = o[14 + q] = o[23 + q] = (q % 4 == 0) ? 1.0 : 0.0;
  o[9] = (double)status; o[11] = HY_NAN; o[12] = -1.0; o[48] = HY_NAN; o[49] = HY_NAN;
}

__global__ void __launch_bounds__(HG_THREADS) k_homog_lo(const HomogArgs a) {
  __shared__ double lds[RS_WAVES * HG_NSUM];
  __shared__ double s_cur[HG_NSUM], s_x[9];       // the refinement's last accepted sums and H~
  const int pair = blockIdx.x, tid = threadIdx.x;
  const long long beg = a.off[pair];
  const int n = (int)(a.off[pair + 1] - beg);
  double* o = a.out + HG_OUT * (size_t)pair;
  if (n < 5) { hg_void(o, HG_FEW_MATCHES); return; }   // (workgroup-uniform, like every branch below)
  // the lowest (cost, h) over the score blocks, in block order: the same in every lane
  const double* b = a.best + HG_BEST * (size_t)pair * a.n_blk;
  double gc, gk;
  const int win = hy_winner<HG_BEST>(b, a.n_blk, gc, gk);
  if (!(gc < HY_INF)) { hg_void(o, HG_DEGENERATE); return; }   // every hypothesis void
  const int best = (int)gk;
  double H[9], A[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) H[q] = b[HG_BEST * win + 2 + q];
  const double thr2 = a.thr * a.thr;
  int status = HG_OK;
  // ---- local optimisation
  for (int round = 0; round < a.lo_rounds && status == HG_OK; ++round) {
    hg_adj(H, A);
    double cn[1] = {0.0};
    for (int j = tid; j < n; j += HG_THREADS) {   // every lane writes the bytes it reads back in the passes (same stride)
      double f, bb;
      const unsigned char in = hg_inlier(H, A, pv_norm(a, a.p1[beg + j]), pv_norm(a, a.p2[beg + j]), thr2, f, bb) ? 1 : 0;
      a.cons[beg + j] = in;
      cn[0] += (double)in;
    }
    rs_block_sums<1>(cn, lds);
    if (!(cn[0] > 0.0)) break;
    // ba_resect's step 3 in the eight local parameters; a pass keeps only the trial H~ and its own sums in registers
    double acc[HG_NSUM], Ht[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) Ht[q] = H[q];
    double lam = 1e-4;
    bool first = true, small = false;
    int it = 0;
    for (;;) {
      hg_pass(a, Ht, beg, n, acc, lds);
      if (first || acc[44] <= s_cur[44] * (1.0 + TRK_COST_SLACK)) {   // (workgroup-uniform)
        hy_keep(s_cur, s_x, acc, Ht);
        if (!first) lam = fmax(0.1 * lam, 1e-12);
      } else {
        lam *= 10.0;
      }
      first = false;
      if (small || it >= a.iters) break;
      ++it;
      double dx[8];
#pragma unroll
      for (int q = 0; q < HG_NSUM; ++q) acc[q] = s_cur[q];
      if (!lm_step(acc, lam, false, dx)) { status = HG_DEGENERATE; break; }
      double d2 = 0.0;
      bool fin = true;
#pragma unroll
      for (int q = 0; q < 8; ++q) { d2 += dx[q] * dx[q]; fin = fin && sim_finite(dx[q]); }
      if (!fin) { status = HG_DEGENERATE; break; }
#pragma unroll
      for (int q = 0; q < 9; ++q) H[q] = s_x[q];
      hg_move(H, dx, Ht);
      small = sqrt(d2) <= 1e-14;
    }
#pragma unroll
    for (int q = 0; q < 9; ++q) H[q] = s_x[q];
  }
  // ---- measures at the final H~
  hg_adj(H, A);
  double m2[2] = {0.0, 0.0};                      // inliers | sum (f + b)
  for (int j = tid; j < n; j += HG_THREADS) {
    double f, bb;
    if (!hg_inlier(H, A, pv_norm(a, a.p1[beg + j]), pv_norm(a, a.p2[beg + j]), thr2, f, bb)) continue;
    m2[0] += 1.0; m2[1] += f + bb;
    a.inl[beg + j] = 1;                           // (read back below by the lane that wrote it: same stride)
  }
  rs_block_sums<2>(m2, lds);
  const double rms = m2[0] > 0.0 ? a.fbar * sqrt(0.5 * m2[1] / m2[0]) : HY_NAN;
  if (status == HG_OK && m2[0] < (double)a.min_inliers) status = HG_FEW_INLIERS;
  // ---- H~ = U diag(d) V^T; the third columns are the cross products of the first two, so det U = det V = +1 and d3 > 0 (det H~ > 0)
  double U[3][3], V[3][3], d[3];
  hy_canon_svd(H, U, V, d);
  const double d1 = d[0], d2 = d[1], d3 = d[2];
  const double ratio = (d1 - d3) / d2;
  RpPose P[2];
  double nv[2][3], vote[2] = {0.0, 0.0}, pcost[2] = {HY_NAN, HY_NAN}, tod[2] = {0.0, 0.0};
#pragma unroll
  for (int k = 0; k < 2; ++k)
#pragma unroll
    for (int q = 0; q < 9; ++q) { P[k].R[q] = (q % 4 == 0) ? 1.0 : 0.0; if (q < 3) { P[k].t[q] = 0.0; nv[k][q] = 0.0; } }
  int n_pose = 0;
  bool rotation = false, ambiguous = false;
  if (!sim_finite(ratio)) {
    status = HG_DEGENERATE;
  } else if (!(ratio > a.min_translation)) {
    rotation = true;
    n_pose = 1;
    tod[0] = ratio;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) P[0].R[3 * i + j] = U[i][0] * V[j][0] + U[i][1] * V[j][1] + U[i][2] * V[j][2];
  } else {
    // Faugeras & Lustman (1988), d' = +d2: x1 = e1 a1, x3 = e3 a3; pose 0 has e1 e3 = +1, pose 1 has e1 e3 = -1, e1 = +1 in both
    const double q12 = fmax(d1 * d1 - d2 * d2, 0.0), q23 = fmax(d2 * d2 - d3 * d3, 0.0), den = d1 * d1 - d3 * d3;
    const double a1 = sqrt(q12 / den), a3 = sqrt(q23 / den);
    const double ct = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2), st0 = sqrt(q12 * q23) / ((d1 + d3) * d2);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const double e3 = k == 0 ? 1.0 : -1.0, st = e3 * st0;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j)
          P[k].R[3 * i + j] = U[i][0] * (ct * V[j][0] - st * V[j][2]) + U[i][1] * V[j][1] + U[i][2] * (st * V[j][0] + ct * V[j][2]);
        P[k].t[i] = a1 * U[i][0] - e3 * a3 * U[i][2];
        nv[k][i] = a1 * V[i][0] + e3 * a3 * V[i][2];
      }
      tod[k] = ratio;
    }
    // n towards the side most inliers lie on
    double side[4] = {0.0, 0.0, 0.0, 0.0};         // pose 0: n . x1~ > 0 | < 0, pose 1 alike
    for (int j = tid; j < n; j += HG_THREADS) {
      if (!a.inl[beg + j]) continue;
      const double2 x1 = pv_norm(a, a.p1[beg + j]);
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const double s = nv[k][0] * x1.x + nv[k][1] * x1.y + nv[k][2];
        if (s > 0.0) side[2 * k] += 1.0;
        if (s < 0.0) side[2 * k + 1] += 1.0;
      }
    }
    rs_block_sums<4>(side, lds);
#pragma unroll
    for (int k = 0; k < 2; ++k)
      if (side[2 * k + 1] > side[2 * k]) {
#pragma unroll
        for (int i = 0; i < 3; ++i) { P[k].t[i] = -P[k].t[i]; nv[k][i] = -nv[k][i]; }
      }
    // votes of the inliers, MSAC Sampson cost of [t]x R on all matches
    double E0[9], E1[9];
    rp_essential(P[0], E0);
    rp_essential(P[1], E1);
    double vc[4] = {0.0, 0.0, 0.0, 0.0};           // votes 0 | votes 1 | cost 0 | cost 1
    for (int j = tid; j < n; j += HG_THREADS) {
      const double2 x1 = pv_norm(a, a.p1[beg + j]), x2 = pv_norm(a, a.p2[beg + j]);
      double r2, ra[3];
      vc[2] += rp_sampson2(E0, x1.x, x1.y, x2.x, x2.y, r2) ? fmin(r2, thr2) : thr2;
      vc[3] += rp_sampson2(E1, x1.x, x1.y, x2.x, x2.y, r2) ? fmin(r2, thr2) : thr2;
      if (!a.inl[beg + j]) continue;
#pragma unroll
      for (int k = 0; k < 2; ++k)
        if (nv[k][0] * x1.x + nv[k][1] * x1.y + nv[k][2] > 0.0 && rp_front(P[k], 1.0, a.max_depth, x1.x, x1.y, x2.x, x2.y, ra)) vc[k] += 1.0;
    }
    rs_block_sums<4>(vc, lds);
    vote[0] = vc[0]; vote[1] = vc[1]; pcost[0] = vc[2]; pcost[1] = vc[3];
    if (vote[1] > vote[0] || (vote[1] == vote[0] && pcost[1] < pcost[0])) {   // votes descending, cost ascending, number
      const RpPose tp = P[0]; P[0] = P[1]; P[1] = tp;
#pragma unroll
      for (int i = 0; i < 3; ++i) { const double tn = nv[0][i]; nv[0][i] = nv[1][i]; nv[1][i] = tn; }
      double tv = vote[0]; vote[0] = vote[1]; vote[1] = tv;
      tv = pcost[0]; pcost[0] = pcost[1]; pcost[1] = tv;
    }
    n_pose = (vote[0] > 0.0 ? 1 : 0) + (vote[1] > 0.0 ? 1 : 0);
    ambiguous = vote[1] >= a.ambiguity * vote[0];
  }
  if (status == HG_OK) status = rotation ? HG_ROTATION : ambiguous ? HG_AMBIGUOUS : HG_OK;
  if (tid != 0) return;
  // ---- the pixel H = K H~ K^-1 at unit norm, det > 0
  {
    double T[9], Hp[9], det;
#pragma unroll
    for (int j = 0; j < 3; ++j) { T[j] = a.fx * H[j] + a.cx * H[6 + j]; T[3 + j] = a.fy * H[3 + j] + a.cy * H[6 + j]; T[6 + j] = H[6 + j]; }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      Hp[3 * i] = T[3 * i] / a.fx; Hp[3 * i + 1] = T[3 * i + 1] / a.fy;
      Hp[3 * i + 2] = T[3 * i + 2] - Hp[3 * i] * a.cx - Hp[3 * i + 1] * a.cy;
    }
    hg_unit(Hp, det);
    for (int q = 0; q < 9; ++q) o[q] = Hp[q];
  }
  o[9] = (double)status; o[10] = m2[0]; o[11] = rms; o[12] = (double)best; o[13] = (double)n_pose;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    for (int q = 0; q < 9; ++q) o[14 + 9 * k + q] = P[k].R[q];
    for (int q = 0; q < 3; ++q) { o[32 + 3 * k + q] = P[k].t[q]; o[38 + 3 * k + q] = nv[k][q]; }
    o[44 + k] = tod[k]; o[46 + k] = vote[k]; o[48 + k] = pcost[k];
  }
}

}  // namespace ba
