// Two-view fundamental matrix (ba_fundamental): the F of raw pixel matches of an UNCALIBRATED pair, a share of which may be
// wrong -- seven-point minimal samples scored on all matches, then rounds of consensus and refinement (cv2.findFundamentalMat's
// and COLMAP's uncalibrated two-view geometry).  The one two-view model that needs no K.  Stand-alone kernels: they read the
// call's own staging buffers and nothing of a resident problem.  Convention of features.fundamental: p2^T F p1 = 0 in pixels.
//
// Coordinates.  q = p - c are CENTRED pixels, x~ = s q normalised ones (Hartley: c the centroid of the pair's matches in that
// image, s = sqrt(2) / mean |q|).  The solver and the refinement work on F~ (x2~^T F~ x1~ = 0, unit Frobenius norm); every
// distance is taken in centred pixels with F_c = S2 F~ S1, S = diag(s, s, 1) -- the Sampson distance does not change under
// translation, so it is the pixel distance, and no quantity of the order of |c| enters before the last step.
//
// Four launches per call, for all pairs at once:
//   k_fund_norm   one workgroup per pair: c1 | s1 | c2 | s2 of step 1, six doubles; s = 0 marks a DEGENERATE pair.
//   k_fund_solve  grid (pairs, ceil(n_hyp / 64)): lane = hypothesis.  Sample -> the 7 x 9 system in 63 registers, Gauss-Jordan with
//                 the columns swapped in place (every index a compile-time constant: the pivot column is found by comparisons
//                 and moved by selects) -> the two null vectors -> the cubic det(a F1 + (1 - a) F2) -> its real roots by
//                 bisection between the critical points -> up to three F~ and a slot mask per hypothesis.
//   k_fund_score  grid (pairs, ceil(3 n_hyp / 256)): lane = candidate 3 h + slot, F_c in nine registers; the pair's centred matches
//                 stream through LDS in tiles of HY_TILE (q1 | q2); MSAC cost of the squared Sampson distance; the block's
//                 lowest (cost, key) by hy_block_best.
//   k_fund_lo     one workgroup per pair: the lowest (cost, key) over the score blocks, lo_rounds of {consensus bytes; F~ = U
//                 diag(1, sigma, 0) V^T (hy_canon_svd); Marquardt-damped Gauss-Newton in the seven parameters of that
//                 orthonormal representation}, the measures, the pixel F, the epipoles, the status.  The last accepted (U, V,
//                 sigma) and its 36 sums live in LDS.  Sums by rs_block_sums: fixed order, no atomics.
#pragma once
#include "ba_homography.hpp"
#include "ba_sim3.hpp"

namespace ba {

enum : int { FD_OK = 0, FD_FEW_MATCHES = 1, FD_DEGENERATE = 2, FD_FEW_INLIERS = 3 };
constexpr int FD_THREADS = HY_THREADS;
constexpr int FD_SOLVE_THREADS = 64;           // hypotheses per workgroup of k_fund_solve: one wave, so a call of 1024 spreads over 16 CUs
constexpr int FD_SLOTS = 3;                    // solutions per hypothesis, numbered by ascending a
constexpr int FD_BEST = 12;                    // doubles per (pair, score block): cost | key | F~[9] | -
constexpr int FD_OUT = 20;                     // doubles per pair: F[9] | status n_inliers rms best_hyp | epipole1[3] | epipole2[3] | -
constexpr int FD_NSUM = S3_NSUM;               // a refinement pass: J^T J (28, packed upper) | g (7) | cost, as ba_sim3's
constexpr int FD_NORM = 6;                     // doubles per pair: c1x c1y s1 c2x c2y s2
constexpr int FD_MODEL = 19;                   // U[9] | V[9] | sigma
constexpr int FD_MIN_SET = 8;                  // a smaller consensus set ends the rounds: seven matches fit any of three F exactly
constexpr int FD_BISECT = 64;
constexpr double FD_PIVOT_TOL = 1e-12;         // a pivot of the 7 x 9 elimination <= this times the first pivot: rank below 7
constexpr double FD_LEAD_TOL = 1e-12;          // |c3| <= this times max |c0 .. c2| of the cubic: F1 - F2 itself is singular
static_assert(FD_THREADS == RS_THREADS, "rs_block_sums folds RS_WAVES waves");
static_assert(FD_NSUM == 36, "28 + 7 + 1 sums of seven parameters");

struct FundArgs : PairArgs {   // fx = fy = 1, cx = cy = 0 (no K): thr = max_epi_px; best: FD_BEST doubles per (pair, score block); out: FD_OUT per pair
  double* nrm;             // [pairs][FD_NORM]
  double* F;               // [pairs][n_hyp][FD_SLOTS][9]: F~
  unsigned* mask;          // [pairs][n_hyp]: bit s = slot s holds an F~
};

struct FdNorm { double c1x, c1y, s1, c2x, c2y, s2; };
__device__ __forceinline__ FdNorm fd_load_norm(const FundArgs& a, const int pair) {
  const double* t = a.nrm + FD_NORM * (size_t)pair;
  return FdNorm{t[0], t[1], t[2], t[3], t[4], t[5]};
}
__device__ __forceinline__ bool fd_norm_ok(const FdNorm& t) { return t.s1 > 0.0 && t.s2 > 0.0; }
// F_c = S2 F~ S1
__device__ __forceinline__ void fd_centred(const double (&Fn)[9], const FdNorm& t, double (&Fc)[9]) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) Fc[3 * i + j] = Fn[3 * i + j] * (i < 2 ? t.s2 : 1.0) * (j < 2 ? t.s1 : 1.0);
}
// unit Frobenius norm; false: not finite
__device__ __forceinline__ bool fd_unit(double (&F)[9]) {
  double n2 = 0.0;
#pragma unroll
  for (int q = 0; q < 9; ++q) n2 += F[q] * F[q];
  const double in = 1.0 / sqrt(n2);
  bool fin = sim_finite(in) && n2 > 0.0;
#pragma unroll
  for (int q = 0; q < 9; ++q) { F[q] *= in; fin = fin && sim_finite(F[q]); }
  return fin;
}

// ------------------------------------------------------------------------------------------------ step 1: Hartley normalisation
__global__ void __launch_bounds__(FD_THREADS) k_fund_norm(const FundArgs a) {
  __shared__ double lds[RS_WAVES * 4];
  const int pair = blockIdx.x, tid = threadIdx.x;
  const long long beg = a.off[pair];
  const int n = (int)(a.off[pair + 1] - beg);
  double* o = a.nrm + FD_NORM * (size_t)pair;
  if (n < 8) {                                    // (workgroup-uniform) FEW_MATCHES: nothing reads the row
    if (tid < FD_NORM) o[tid] = 0.0;
    return;
  }
  double s4[4] = {0.0, 0.0, 0.0, 0.0};
  for (int j = tid; j < n; j += FD_THREADS) {
    const double2 p1 = a.p1[beg + j], p2 = a.p2[beg + j];
    s4[0] += p1.x; s4[1] += p1.y; s4[2] += p2.x; s4[3] += p2.y;
  }
  rs_block_sums<4>(s4, lds);
  const double inv = 1.0 / (double)n;
  const double c1x = s4[0] * inv, c1y = s4[1] * inv, c2x = s4[2] * inv, c2y = s4[3] * inv;
  double d2[2] = {0.0, 0.0};
  for (int j = tid; j < n; j += FD_THREADS) {
    const double2 p1 = a.p1[beg + j], p2 = a.p2[beg + j];
    const double ax = p1.x - c1x, ay = p1.y - c1y, bx = p2.x - c2x, by = p2.y - c2y;
    d2[0] += sqrt(ax * ax + ay * ay); d2[1] += sqrt(bx * bx + by * by);
  }
  rs_block_sums<2>(d2, lds);
  const double m1 = d2[0] * inv, m2 = d2[1] * inv;
  const bool ok = m1 > 0.0 && m2 > 0.0 && sim_finite(m1) && sim_finite(m2);   // a zero mean distance, or a pixel that is not finite
  if (tid == 0) {
    o[0] = c1x; o[1] = c1y; o[2] = ok ? 1.4142135623730951 / m1 : 0.0;
    o[3] = c2x; o[4] = c2y; o[5] = ok ? 1.4142135623730951 / m2 : 0.0;
  }
}

// ------------------------------------------------------------------------------------------------ step 2: seven-point hypotheses
__device__ __forceinline__ double fd_cubic(const double (&P)[4], const double z) { return ((P[3] * z + P[2]) * z + P[1]) * z + P[0]; }
__device__ __forceinline__ double fd_dcubic(const double (&P)[4], const double z) { return (3.0 * P[3] * z + 2.0 * P[2]) * z + P[1]; }
// the root of the cubic in [lo, hi], on which it is monotone; false: no sign change
__device__ __forceinline__ bool fd_bisect(const double (&P)[4], double lo, double hi, double& root) {
  const double lo0 = lo, hi0 = hi;
  const bool neg = fd_cubic(P, lo) < 0.0;
  if (neg == (fd_cubic(P, hi) < 0.0)) return false;
#pragma unroll 1
  for (int it = 0; it < FD_BISECT; ++it) {
    const double mid = 0.5 * (lo + hi);
    if ((fd_cubic(P, mid) < 0.0) == neg) lo = mid; else hi = mid;
  }
  root = 0.5 * (lo + hi);
#pragma unroll 1
  for (int it = 0; it < 2; ++it) {
    const double zn = root - fd_cubic(P, root) / fd_dcubic(P, root);
    if (zn >= lo0 && zn <= hi0) root = zn;        // (false for NaN)
  }
  return true;
}

__global__ void __launch_bounds__(FD_SOLVE_THREADS) k_fund_solve(const FundArgs a) {
  const int pair = blockIdx.x, h = blockIdx.y * FD_SOLVE_THREADS + threadIdx.x;
  const long long beg = a.off[pair];
  const int n = (int)(a.off[pair + 1] - beg);
  const FdNorm t = fd_load_norm(a, pair);
  if (n < 8 || !fd_norm_ok(t) || h >= a.n_hyp) return;   // FEW_MATCHES and step 1's DEGENERATE: k_fund_score reads no slot
  const size_t hyp = (size_t)pair * a.n_hyp + h;
  a.mask[hyp] = 0u;                               // (no barrier in this kernel: a void hypothesis leaves here)
  // ---- sample, and the 7 x 9 system: row r = kron(x2~_r, x1~_r)
  int idx[7];
  hy_sample(a.seed, pair, h, n, idx);
  double A[7][9];
#pragma unroll
  for (int r = 0; r < 7; ++r) {
    const double2 p1 = a.p1[beg + idx[r]], p2 = a.p2[beg + idx[r]];
    const double f1[3] = {t.s1 * (p1.x - t.c1x), t.s1 * (p1.y - t.c1y), 1.0}, f2[3] = {t.s2 * (p2.x - t.c2x), t.s2 * (p2.y - t.c2y), 1.0};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) A[r][3 * i + j] = f2[i] * f1[j];
  }
  // ---- Gauss-Jordan by rows; the pivot of row r is its largest entry among the columns r .. 8 (the first of equal ones), and
  // that column changes places with column r, so the pivots end in columns 0 .. 6 and the free columns in 7 and 8
  int perm[9];                                    // perm[c]: the column of the system that now stands at c
#pragma unroll
  for (int c = 0; c < 9; ++c) perm[c] = c;
  double piv0 = 0.0;
#pragma unroll
  for (int r = 0; r < 7; ++r) {
    int p = r;
    double pm = fabs(A[r][r]);
#pragma unroll
    for (int c = r + 1; c < 9; ++c) { const double m = fabs(A[r][c]); if (m > pm) { pm = m; p = c; } }
    if (r == 0) piv0 = pm;
    if (!(pm > FD_PIVOT_TOL * piv0) || !sim_finite(pm)) return;   // rank below 7 (pm = piv0 = 0 in row 0 as well)
#pragma unroll
    for (int c = r + 1; c < 9; ++c) {
      const bool sw = c == p;
#pragma unroll
      for (int i = 0; i < 7; ++i) { const double u = A[i][r], v = A[i][c]; A[i][r] = sw ? v : u; A[i][c] = sw ? u : v; }
      const int u = perm[r], v = perm[c];
      perm[r] = sw ? v : u; perm[c] = sw ? u : v;
    }
    const double inv = 1.0 / A[r][r];
#pragma unroll
    for (int c = r; c < 9; ++c) A[r][c] = c == r ? 1.0 : A[r][c] * inv;
#pragma unroll
    for (int i = 0; i < 7; ++i) {
      if (i == r) continue;
      const double f = A[i][r];
#pragma unroll
      for (int c = r; c < 9; ++c) A[i][c] = c == r ? 0.0 : A[i][c] - f * A[r][c];
    }
  }
  // ---- the null vectors: free column 7 (F1) or 8 (F2) is 1, the pivot columns are minus the reduced rows' entries there
  double F1[9], F2[9];
  {
    double n1[9], n2[9];                          // by place; entry c belongs to column perm[c] of the system
#pragma unroll
    for (int c = 0; c < 7; ++c) { n1[c] = -A[c][7]; n2[c] = -A[c][8]; }
    n1[7] = 1.0; n1[8] = 0.0; n2[7] = 0.0; n2[8] = 1.0;
#pragma unroll
    for (int j = 0; j < 9; ++j) {
      F1[j] = 0.0; F2[j] = 0.0;
#pragma unroll
      for (int c = 0; c < 9; ++c) if (perm[c] == j) { F1[j] = n1[c]; F2[j] = n2[c]; }
    }
  }
  // ---- det(a F1 + (1 - a) F2) = det(F2 + a D), D = F1 - F2: c0 = det F2, c1 = tr(adj(F2) D), c2 = tr(adj(D) F2), c3 = det D
  double D[9], AB[9], AD[9], P[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int q = 0; q < 9; ++q) D[q] = F1[q] - F2[q];
  hg_adj(F2, AB);
  hg_adj(D, AD);
  P[0] = F2[0] * AB[0] + F2[1] * AB[3] + F2[2] * AB[6];
  P[3] = D[0] * AD[0] + D[1] * AD[3] + D[2] * AD[6];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) { P[1] += AB[3 * i + j] * D[3 * j + i]; P[2] += AD[3 * i + j] * F2[3 * j + i]; }
  const double cmax = fmax(fmax(fabs(P[0]), fabs(P[1])), fabs(P[2]));
  if (!(fabs(P[3]) > FD_LEAD_TOL * cmax) || !sim_finite(cmax)) return;   // a root at infinity: void (the header's step 2)
  const double B = 1.0 + cmax / fabs(P[3]);       // Cauchy: every root lies inside
  if (!sim_finite(B)) return;
  // the critical points split [-B, B] into at most three intervals on which the cubic is monotone
  double node[4] = {-B, B, B, B};
  int n_int = 1;
  const double disc = P[2] * P[2] - 3.0 * P[3] * P[1];
  if (disc > 0.0) {
    const double q = -(P[2] + (P[2] >= 0.0 ? 1.0 : -1.0) * sqrt(disc));   // (not 0: disc > 0)
    const double r1 = q / (3.0 * P[3]), r2 = P[1] / q;
    const double lo = fmin(fmax(fmin(r1, r2), -B), B), hi = fmin(fmax(fmax(r1, r2), -B), B);
    node[1] = lo; node[2] = hi;
    n_int = 3;
  }
  unsigned bits = 0u;
  int ns = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    double z;
    if (k >= n_int || !fd_bisect(P, node[k], node[k + 1], z)) continue;
    double F[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) F[q] = F2[q] + z * D[q];
    if (!fd_unit(F)) continue;
    double* o = a.F + 9 * (FD_SLOTS * hyp + ns);   // ns < FD_SLOTS: at most three intervals
#pragma unroll
    for (int q = 0; q < 9; ++q) o[q] = F[q];
    bits |= 1u << ns;
    ++ns;
  }
  a.mask[hyp] = bits;
}

// ------------------------------------------------------------------------------------------------ step 3: scores
__global__ void __launch_bounds__(FD_THREADS) k_fund_score(const FundArgs a) {
  __shared__ double tile[HY_TILE * 4];
  __shared__ double red[2 * HY_WAVES];
  const int pair = blockIdx.x, blk = blockIdx.y, tid = threadIdx.x;
  const long long beg = a.off[pair];
  const int n = (int)(a.off[pair + 1] - beg);
  double* out = a.best + FD_BEST * ((size_t)pair * a.n_blk + blk);
  const FdNorm t = fd_load_norm(a, pair);
  if (n < 8 || !fd_norm_ok(t)) {                  // (workgroup-uniform) FEW_MATCHES, or step 1's DEGENERATE
    hy_void_block(out);
    return;
  }
  const int cand = blk * FD_THREADS + tid, h = cand / FD_SLOTS, slot = cand % FD_SLOTS;
  bool valid = false;
  double Fn[9], Fc[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) Fn[q] = 0.0;        // a void candidate: denominator 0, thr^2 each
  if (h < a.n_hyp) {
    const size_t hyp = (size_t)pair * a.n_hyp + h;
    valid = (a.mask[hyp] >> slot) & 1u;
    if (valid) {
      const double* s = a.F + 9 * (FD_SLOTS * hyp + slot);
#pragma unroll
      for (int q = 0; q < 9; ++q) Fn[q] = s[q];
    }
  }
  fd_centred(Fn, t, Fc);
  const double thr2 = a.thr * a.thr;
  double cost = 0.0;
  for (int i0 = 0; i0 < n; i0 += HY_TILE) {
    const int m = min(HY_TILE, n - i0);
    __syncthreads();                              // (the readers of the previous tile are done)
    if (tid < m) {
      const double2 p1 = a.p1[beg + i0 + tid], p2 = a.p2[beg + i0 + tid];
      double2* d = (double2*)(tile + 4 * tid);
      d[0] = make_double2(p1.x - t.c1x, p1.y - t.c1y); d[1] = make_double2(p2.x - t.c2x, p2.y - t.c2y);
    }
    __syncthreads();
    for (int i = 0; i < m; ++i) {                 // every lane reads the same address: an LDS broadcast
      const double2* s = (const double2*)(tile + 4 * i);
      const double2 q1 = s[0], q2 = s[1];
      double r2;
      const bool has = rp_sampson2(Fc, q1.x, q1.y, q2.x, q2.y, r2);
      cost += has ? fmin(r2, thr2) : thr2;
    }
  }
  double gc, gk;
  const bool mine = hy_block_best(valid ? cost : HY_INF, valid ? (double)cand : HY_INF, red, gc, gk);
  if (!(gc < HY_INF)) {
    hy_void_block(out);
    return;
  }
  if (mine) {
    out[0] = gc; out[1] = gk;
#pragma unroll
    for (int q = 0; q < 9; ++q) out[2 + q] = Fn[q];
  }
}

// ------------------------------------------------------------------------------------------------ steps 4 and 5: LO, measures
// F~ = U diag(1, sigma, 0) V^T at unit Frobenius norm, x = U[9] | V[9] | sigma
__device__ __forceinline__ bool fd_compose(const double (&x)[FD_MODEL], double (&Fn)[9]) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) Fn[3 * i + j] = x[3 * i] * x[9 + 3 * j] + x[18] * (x[3 * i + 1] * x[9 + 3 * j + 1]);
  return fd_unit(Fn);
}
// The sums of a refinement pass over the consensus set at x: J^T J, g and 0.5 sum r^2 of the Sampson distance r in centred
// pixels, in the seven local parameters U <- U exp([a]x), V <- V exp([b]x), sigma <- sigma + ds.  With alpha = U^T x2~, beta = V^T
// x1~, w = Sigma beta and z = Sigma alpha: num = alpha . w, F~ x1~ = U w, F~^T x2~ = V z, so the derivatives are cross products per match
// (a_k: w -> e_k x w, z -> -Sigma (e_k x alpha); b_k: z -> e_k x z, w -> -Sigma (e_k x beta); ds: the second columns) and no
// 3 x 3 derivative is held.
__device__ __forceinline__ void fd_pass(const FundArgs& a, const FdNorm& t, const double (&x)[FD_MODEL], const long long beg, const int n,
                                        double (&acc)[FD_NSUM], double* __restrict__ lds) {
  const double sg = x[18];
#pragma unroll
  for (int q = 0; q < FD_NSUM; ++q) acc[q] = 0.0;
  for (int j = (int)threadIdx.x; j < n; j += FD_THREADS) {
    if (!a.cons[beg + j]) continue;
    const double2 p1 = a.p1[beg + j], p2 = a.p2[beg + j];
    const double x1[3] = {t.s1 * (p1.x - t.c1x), t.s1 * (p1.y - t.c1y), 1.0}, x2[3] = {t.s2 * (p2.x - t.c2x), t.s2 * (p2.y - t.c2y), 1.0};
    double al[3], be[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      al[k] = x[k] * x2[0] + x[3 + k] * x2[1] + x[6 + k] * x2[2];
      be[k] = x[9 + k] * x1[0] + x[12 + k] * x1[1] + x[15 + k] * x1[2];
    }
    const double w[3] = {be[0], sg * be[1], 0.0}, z[3] = {al[0], sg * al[1], 0.0};
    const double num = al[0] * w[0] + al[1] * w[1];
    // l = (F_c q1)_xy = s2 (U w)_xy, m = (F_c^T q2)_xy = s1 (V z)_xy
    const double l0 = t.s2 * (x[0] * w[0] + x[1] * w[1]), l1 = t.s2 * (x[3] * w[0] + x[4] * w[1]);
    const double m0 = t.s1 * (x[9] * z[0] + x[10] * z[1]), m1 = t.s1 * (x[12] * z[0] + x[13] * z[1]);
    const double den = l0 * l0 + l1 * l1 + m0 * m0 + m1 * m1;
    if (!(den > 0.0)) continue;
    const double is = 1.0 / sqrt(den), r = num * is, hk = r / den;
    double J[7];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double e[3] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
      double cw[3], ca[3], cb[3], cz[3];
      rp_cross(e, w, cw);
      rp_cross(e, al, ca);
      rp_cross(e, be, cb);
      rp_cross(e, z, cz);
      {                                           // a_k: dw = e_k x w, dz = -Sigma (e_k x alpha)
        const double dz0 = -ca[0], dz1 = -sg * ca[1];
        const double dl0 = t.s2 * (x[0] * cw[0] + x[1] * cw[1] + x[2] * cw[2]), dl1 = t.s2 * (x[3] * cw[0] + x[4] * cw[1] + x[5] * cw[2]);
        const double dm0 = t.s1 * (x[9] * dz0 + x[10] * dz1), dm1 = t.s1 * (x[12] * dz0 + x[13] * dz1);
        const double dnum = al[0] * cw[0] + al[1] * cw[1] + al[2] * cw[2];
        J[k] = dnum * is - hk * ((l0 * dl0 + l1 * dl1) + (m0 * dm0 + m1 * dm1));
      }
      {                                           // b_k: dz = e_k x z, dw = -Sigma (e_k x beta)
        const double dw0 = -cb[0], dw1 = -sg * cb[1];
        const double dl0 = t.s2 * (x[0] * dw0 + x[1] * dw1), dl1 = t.s2 * (x[3] * dw0 + x[4] * dw1);
        const double dm0 = t.s1 * (x[9] * cz[0] + x[10] * cz[1] + x[11] * cz[2]), dm1 = t.s1 * (x[12] * cz[0] + x[13] * cz[1] + x[14] * cz[2]);
        const double dnum = -(z[0] * cb[0] + z[1] * cb[1]);
        J[3 + k] = dnum * is - hk * ((l0 * dl0 + l1 * dl1) + (m0 * dm0 + m1 * dm1));
      }
    }
    {                                             // ds: dF~ = u2 v2^T
      const double dl0 = t.s2 * x[1] * be[1], dl1 = t.s2 * x[4] * be[1], dm0 = t.s1 * x[10] * al[1], dm1 = t.s1 * x[13] * al[1];
      J[6] = al[1] * be[1] * is - hk * ((l0 * dl0 + l1 * dl1) + (m0 * dm0 + m1 * dm1));
    }
#pragma unroll
    for (int q = 0; q < 7; ++q) {
#pragma unroll
      for (int s2 = q; s2 < 7; ++s2) acc[UT(7, q, s2)] += J[q] * J[s2];
      acc[28 + q] += J[q] * r;
    }
    acc[35] += 0.5 * r * r;
  }
  rs_block_sums<FD_NSUM>(acc, lds);
}
// x moved by the local step dx
__device__ __forceinline__ void fd_move(const double (&x)[FD_MODEL], const double (&dx)[7], double (&y)[FD_MODEL]) {
  const double wa[3] = {dx[0], dx[1], dx[2]}, wb[3] = {dx[3], dx[4], dx[5]};
  double Xa[9], Xb[9];
  rp_exp(wa, Xa);
  rp_exp(wb, Xb);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      y[3 * i + j] = x[3 * i] * Xa[j] + x[3 * i + 1] * Xa[3 + j] + x[3 * i + 2] * Xa[6 + j];
      y[9 + 3 * i + j] = x[9 + 3 * i] * Xb[j] + x[9 + 3 * i + 1] * Xb[3 + j] + x[9 + 3 * i + 2] * Xb[6 + j];
    }
  y[18] = x[18] + dx[6];
}
// unit length, the largest-magnitude entry positive (the first of equal ones)
template <int N>
__device__ __forceinline__ void fd_unit_signed(double (&v)[N]) {
  double n2 = 0.0, big = 0.0, sign = 1.0;
#pragma unroll
  for (int q = 0; q < N; ++q) {
    n2 += v[q] * v[q];
    if (fabs(v[q]) > big) { big = fabs(v[q]); sign = v[q] < 0.0 ? -1.0 : 1.0; }
  }
  const double in = sign / sqrt(n2);
#pragma unroll
  for (int q = 0; q < N; ++q) v[q] *= in;
}

// a pair without a fundamental matrix: F = 0 (not a fundamental matrix, so it cannot pass for one), no epipoles
__device__ __forceinline__ void fd_void(double* __restrict__ o, const int status) {
  if (threadIdx.x != 0) return;
  for (int q = 0; q < FD_OUT; ++q) o[q] = 0.0;
  o[9] = (double)status; o[11] = HY_NAN; o[12] = -1.0;
}

__global__ void __launch_bounds__(FD_THREADS) k_fund_lo(const FundArgs a) {
  __shared__ double lds[RS_WAVES * FD_NSUM];
  __shared__ double s_cur[FD_NSUM], s_x[FD_MODEL];   // the refinement's last accepted sums and (U, V, sigma)
  const int pair = blockIdx.x, tid = threadIdx.x;
  const long long beg = a.off[pair];
  const int n = (int)(a.off[pair + 1] - beg);
  double* o = a.out + FD_OUT * (size_t)pair;
  if (n < 8) { fd_void(o, FD_FEW_MATCHES); return; }   // (workgroup-uniform, like every branch below)
  const FdNorm t = fd_load_norm(a, pair);
  if (!fd_norm_ok(t)) { fd_void(o, FD_DEGENERATE); return; }   // step 1
  // the lowest (cost, 3 h + slot) over the score blocks, in block order: the same in every lane
  const double* b = a.best + FD_BEST * (size_t)pair * a.n_blk;
  double gc, gk;
  const int win = hy_winner<FD_BEST>(b, a.n_blk, gc, gk);
  if (!(gc < HY_INF)) { fd_void(o, FD_DEGENERATE); return; }   // every slot void
  const int best = (int)gk / FD_SLOTS;
  double Fn[9], Fc[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) Fn[q] = b[FD_BEST * win + 2 + q];
  const double thr2 = a.thr * a.thr;
  int status = FD_OK;
  // ---- local optimisation
  for (int round = 0; round < a.lo_rounds && status == FD_OK; ++round) {
    fd_centred(Fn, t, Fc);
    double cn[1] = {0.0};
    for (int j = tid; j < n; j += FD_THREADS) {   // every lane writes the bytes it reads back in the passes (same stride)
      const double2 p1 = a.p1[beg + j], p2 = a.p2[beg + j];
      double r2;
      const unsigned char in = rp_sampson2(Fc, p1.x - t.c1x, p1.y - t.c1y, p2.x - t.c2x, p2.y - t.c2y, r2) && r2 <= thr2 ? 1 : 0;
      a.cons[beg + j] = in;
      cn[0] += (double)in;
    }
    rs_block_sums<1>(cn, lds);
    if (cn[0] < (double)FD_MIN_SET) break;
    // the orthonormal representation of the round's starting F~
    double x[FD_MODEL], xt[FD_MODEL];
    {
      double U[3][3], V[3][3], d[3];
      hy_canon_svd(Fn, U, V, d);
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) { x[3 * i + j] = U[i][j]; x[9 + 3 * i + j] = V[i][j]; }
      x[18] = d[1] / d[0];
      bool fin = true;
#pragma unroll
      for (int q = 0; q < FD_MODEL; ++q) { fin = fin && sim_finite(x[q]); xt[q] = x[q]; }
      if (!fin) { status = FD_DEGENERATE; break; }
    }
    // ba_resect's step 3 in the seven local parameters; a pass keeps only the trial model and its own sums in registers
    double acc[FD_NSUM];
    double lam = 1e-4;
    bool first = true, small = false;
    int it = 0;
    for (;;) {
      fd_pass(a, t, xt, beg, n, acc, lds);
      if (first || acc[35] <= s_cur[35] * (1.0 + TRK_COST_SLACK)) {   // (workgroup-uniform)
        hy_keep(s_cur, s_x, acc, xt);
        if (!first) lam = fmax(0.1 * lam, 1e-12);
      } else {
        lam *= 10.0;
      }
      first = false;
      if (small || it >= a.iters) break;
      ++it;
      double dx[7];
#pragma unroll
      for (int q = 0; q < FD_NSUM; ++q) acc[q] = s_cur[q];
      if (!lm_step(acc, lam, false, dx)) { status = FD_DEGENERATE; break; }
      double d2 = 0.0;
      bool fin = true;
#pragma unroll
      for (int q = 0; q < 7; ++q) { d2 += dx[q] * dx[q]; fin = fin && sim_finite(dx[q]); }
      if (!fin) { status = FD_DEGENERATE; break; }
#pragma unroll
      for (int q = 0; q < FD_MODEL; ++q) x[q] = s_x[q];
      fd_move(x, dx, xt);
      small = sqrt(d2) <= 1e-14;
    }
#pragma unroll
    for (int q = 0; q < FD_MODEL; ++q) x[q] = s_x[q];
    fd_compose(x, Fn);
  }
  // ---- measures at the final F~
  fd_centred(Fn, t, Fc);
  double m2[2] = {0.0, 0.0};                      // inliers | sum d^2
  for (int j = tid; j < n; j += FD_THREADS) {
    const double2 p1 = a.p1[beg + j], p2 = a.p2[beg + j];
    double r2;
    if (!(rp_sampson2(Fc, p1.x - t.c1x, p1.y - t.c1y, p2.x - t.c2x, p2.y - t.c2y, r2) && r2 <= thr2)) continue;
    m2[0] += 1.0; m2[1] += r2;
    a.inl[beg + j] = 1;
  }
  rs_block_sums<2>(m2, lds);
  const double rms = m2[0] > 0.0 ? sqrt(m2[1] / m2[0]) : HY_NAN;
  if (status == FD_OK && m2[0] < (double)a.min_inliers) status = FD_FEW_INLIERS;
  if (tid != 0) return;
  // ---- the pixel F = T2^T F_c T1, T = [1 0 -cx; 0 1 -cy; 0 0 1], at unit norm, its largest entry positive
  {
    double M[9], Fp[9];
#pragma unroll
    for (int i = 0; i < 3; ++i) { M[3 * i] = Fc[3 * i]; M[3 * i + 1] = Fc[3 * i + 1]; M[3 * i + 2] = Fc[3 * i + 2] - Fc[3 * i] * t.c1x - Fc[3 * i + 1] * t.c1y; }
#pragma unroll
    for (int j = 0; j < 3; ++j) { Fp[j] = M[j]; Fp[3 + j] = M[3 + j]; Fp[6 + j] = M[6 + j] - t.c2x * M[j] - t.c2y * M[3 + j]; }
    fd_unit_signed<9>(Fp);
    for (int q = 0; q < 9; ++q) o[q] = Fp[q];
  }
  o[9] = (double)status; o[10] = m2[0]; o[11] = rms; o[12] = (double)best;
  // ---- the epipoles: F~ v3 = 0 and F~^T u3 = 0, so e1 = T1^-1 S1^-1 v3 and e2 = T2^-1 S2^-1 u3, unit 3-vectors in pixels
  {
    double U[3][3], V[3][3], d[3];
    hy_canon_svd(Fn, U, V, d);
    const double w1 = V[2][2], w2 = U[2][2];
    double e1[3] = {V[0][2] / t.s1 + t.c1x * w1, V[1][2] / t.s1 + t.c1y * w1, w1};
    double e2[3] = {U[0][2] / t.s2 + t.c2x * w2, U[1][2] / t.s2 + t.c2y * w2, w2};
    fd_unit_signed<3>(e1);
    fd_unit_signed<3>(e2);
    for (int q = 0; q < 3; ++q) { o[13 + q] = e1[q]; o[16 + q] = e2[q]; }
  }
  o[19] = 0.0;
}

}  // namespace ba
