// Two-view relative pose (ba_relative_pose): R | t of the second view against the first from raw pixel matches, a share of
// which may be wrong -- five-point minimal samples scored on all matches, then rounds of consensus and refinement (the
// reference's estimate_pose: cv2.findEssentialMat(RANSAC) + cv2.recoverPose).  Stand-alone kernels: they read the call's own
// staging buffers and nothing of a resident problem.  Convention x2 ~ K (R x1 + t), |t| = 1; x~ = ((u - cx) / fx, (v - cy) / fy, 1).
//
// Three launches per call, for all pairs at once:
//   k_relpose_solve  grid (pairs, ceil(n_hyp / 16)), 256 threads: a hypothesis belongs to a TEAM of 16 lanes (one DPP row; the
//                    teams of a workgroup talk through LDS, the loops are workgroup-uniform so every barrier is __syncthreads).
//                    Sample -> null space (lane = column of the 5 x 9 system, five entries in registers) -> ten cubic
//                    constraints (lane = constraint, its 20 coefficients in registers, indexed by compile-time constants) ->
//                    Gauss-Jordan on the first ten columns (pivot search and pivot row through LDS) -> det B(z), degree 10 ->
//                    real roots (lane = interval between two roots of the next derivative, bisection) -> lane = root: back
//                    substitution, two Gauss-Newton steps, E.  Ten slots of 9 doubles and a validity mask per hypothesis.
//   k_relpose_score  grid (pairs, ceil(10 n_hyp / 256)): lane = candidate 10 h + slot, E in nine registers; the pair's normalised
//                    matches stream through LDS in tiles of HY_TILE (x1 | x2); MSAC cost of the squared Sampson distance; the block's
//                    lowest (cost, key) by hy_block_best.
//   k_relpose_lo     one workgroup per pair: the lowest (cost, key) over the score blocks, E = U diag V^T (hy_canon_svd), the
//                    four (R, t) and their votes, lo_rounds of {consensus bytes; Marquardt-damped Gauss-Newton in five local
//                    parameters}, the measures, the status, match_inlier.  Sums by rs_block_sums: fixed order, no atomics.
//
// Real roots (step 3.5): the real roots of p' split the Cauchy interval [-B, B], B = 1 + max |c_i / c_10|, into intervals on
// which p is monotone, so one bisection per interval with a sign change finds every simple real root, in ascending order; the
// same holds for p', p'', ... down to the linear p^(9).  Ten levels of at most 11 intervals, one lane each, RP_BISECT halvings,
// then two Newton steps on p itself kept inside the bracket.  No Sturm chain: its eleven remainders would be indexed
// dynamically; this needs only the coefficients (registers) and twelve nodes per team (LDS).
//
// Polish (step 3.7) runs on the ten ELIMINATED rows (monomial_i + sum_j C_ij trailing_j = 0, i = 0 .. 9): the same variety as the
// ten raw constraints, 100 coefficients per hypothesis in LDS instead of 200.
#pragma once
#include "ba_hypothesis.hpp"
#include "ba_resect.hpp"

namespace ba {

enum : int { RP_OK = 0, RP_FEW_MATCHES = 1, RP_DEGENERATE = 2, RP_BEHIND = 3, RP_FEW_INLIERS = 4, RP_LOW_PARALLAX = 5 };
constexpr int RP_THREADS = HY_THREADS;
constexpr int RP_TEAM = 16;                    // lanes per hypothesis in k_relpose_solve
constexpr int RP_TEAMS = RP_THREADS / RP_TEAM; // hypotheses per workgroup
constexpr int RP_SLOTS = 10;                   // solutions per hypothesis, numbered by ascending z
constexpr int RP_BEST = 12;                    // doubles per (pair, score block): cost | key | E[9] | -
constexpr int RP_OUT = 18;                     // doubles per pair: R[9] | t[3] | status | n_inliers | rms | parallax | best_hyp | -
constexpr int RP_NSUM = 21;                    // a refinement pass: H (15) g (5) cost
constexpr int RP_BISECT = 64;
constexpr double RP_PIVOT_TOL = 1e-12;
constexpr double RP_RAY_TOL = 1e-24;

struct RelposeArgs : PairArgs {   // thr = max_epi_px / fbar; best: RP_BEST doubles per (pair, score block); out: RP_OUT per pair
  double min_parallax;
  double* E;               // [pairs][n_hyp][RP_SLOTS][9]
  unsigned* mask;          // [pairs][n_hyp]: bit s = slot s holds an E
};

// ---------------------------------------------------------------------------------- polynomials in (x, y, z), fixed orders
// linear: x y z 1;  quadratic: x2 y2 z2 xy xz yz x y z 1;  cubic: the column order of the 10 x 20 constraint matrix,
// x3 y3 x2y xy2 x2z x2 y2z y2 xyz xy | xz2 xz x yz2 yz y z3 z2 z 1.  Every index below folds to a constant once the loops unroll.
__host__ __device__ constexpr int rp_le(const int i, const int v) { return i == v ? 1 : 0; }
__host__ __device__ constexpr int rp_qe(const int i, const int v) {
  return v == 0 ? (i == 0 ? 2 : (i == 3 || i == 4 || i == 6) ? 1 : 0)
       : v == 1 ? (i == 1 ? 2 : (i == 3 || i == 5 || i == 7) ? 1 : 0)
                : (i == 2 ? 2 : (i == 4 || i == 5 || i == 8) ? 1 : 0);
}
__host__ __device__ constexpr int rp_qi(const int ex, const int ey, const int ez) {
  switch (ex * 9 + ey * 3 + ez) {
    case 18: return 0; case 6: return 1; case 2: return 2; case 12: return 3; case 10: return 4;
    case 4: return 5;  case 9: return 6; case 3: return 7; case 1: return 8;  default: return 9;
  }
}
__host__ __device__ constexpr int rp_ci(const int ex, const int ey, const int ez) {
  switch (ex * 16 + ey * 4 + ez) {
    case 48: return 0;  case 12: return 1;  case 36: return 2;  case 24: return 3;  case 33: return 4;
    case 32: return 5;  case 9: return 6;   case 8: return 7;   case 21: return 8;  case 20: return 9;
    case 18: return 10; case 17: return 11; case 16: return 12; case 6: return 13;  case 5: return 14;
    case 4: return 15;  case 3: return 16;  case 2: return 17;  case 1: return 18;  default: return 19;
  }
}
// q += a b
__device__ __forceinline__ void rp_mul_ll(const double (&a)[4], const double (&b)[4], double (&q)[10]) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      q[rp_qi(rp_le(i, 0) + rp_le(j, 0), rp_le(i, 1) + rp_le(j, 1), rp_le(i, 2) + rp_le(j, 2))] += a[i] * b[j];
}
// c += s q l
__device__ __forceinline__ void rp_mul_ql(const double (&q)[10], const double (&l)[4], const double s, double (&c)[20]) {
#pragma unroll
  for (int i = 0; i < 10; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      c[rp_ci(rp_qe(i, 0) + rp_le(j, 0), rp_qe(i, 1) + rp_le(j, 1), rp_qe(i, 2) + rp_le(j, 2))] += s * q[i] * l[j];
}
// entry ab of E = x N0 + y N1 + z N2 + N3 as a linear polynomial (N: 4 x 9 in LDS)
__device__ __forceinline__ void rp_lin(const double* __restrict__ N, const int ab, double (&l)[4]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) l[k] = N[9 * k + ab];
}

__host__ __device__ constexpr double rp_binom(const int n, const int k) {
  double r = 1.0;
  for (int i = 1; i <= k; ++i) r = r * (double)(n - k + i) / (double)i;
  return r;
}
// p^(K)(z) / K! for p = sum P[i] z^i of degree 10
template <int K>
__device__ __forceinline__ double rp_dpoly(const double (&P)[11], const double z) {
  double acc = rp_binom(10, K) * P[10];
#pragma unroll
  for (int i = 9; i >= K; --i) acc = acc * z + rp_binom(i, K) * P[i];
  return acc;
}

// Levels K, K - 1, .. 0 of the root isolation: `nr` real roots of p^(K + 1) lie, ascending and between -B and B, in
// nodes[12 * (K & 1)]; the roots of p^(K) go to the other buffer.  Ends with the roots of p in nodes[12 + 1 ..], nr of them.
template <int K>
__device__ __forceinline__ void rp_levels(const double (&P)[11], const double B, double* __restrict__ nodes, const int tl, const int tw, int& nr) {
  const double* in = nodes + 12 * (K & 1);
  double* out = nodes + 12 * ((K & 1) ^ 1);
  bool has = false;
  double root = 0.0;
  if (tl <= nr) {                                 // interval tl of nr + 1
    double lo = in[tl], hi = in[tl + 1];
    const double lo0 = lo, hi0 = hi;
    const bool neg = rp_dpoly<K>(P, lo) < 0.0;
    has = neg != (rp_dpoly<K>(P, hi) < 0.0);
    if (has) {
#pragma unroll 1
      for (int it = 0; it < RP_BISECT; ++it) {
        const double mid = 0.5 * (lo + hi);
        if ((rp_dpoly<K>(P, mid) < 0.0) == neg) lo = mid; else hi = mid;
      }
      root = 0.5 * (lo + hi);
      if constexpr (K == 0) {
#pragma unroll 1
        for (int it = 0; it < 2; ++it) {
          const double f = rp_dpoly<0>(P, root), df = rp_dpoly<1>(P, root);
          const double zn = root - f / df;
          if (zn >= lo0 && zn <= hi0) root = zn;  // (false for NaN)
        }
      }
    }
  }
  const unsigned bits = (unsigned)(__ballot(has) >> (RP_TEAM * tw)) & 0xffffu;
  const int pos = __popc(bits & ((1u << tl) - 1u));
  nr = __popc(bits);                              // <= the number of intervals <= 10 - K
  if (has) out[1 + pos] = root;
  if (tl == 0) { out[0] = -B; out[nr + 1] = B; }
  __syncthreads();
  if constexpr (K > 0) rp_levels<K - 1>(P, B, nodes, tl, tw, nr);
}

// Squared Sampson distance of (x1, x2) at E; false: a zero (or non-finite) denominator
__device__ __forceinline__ bool rp_sampson2(const double (&E)[9], const double x1x, const double x1y, const double x2x, const double x2y, double& r2) {
  const double l0 = E[0] * x1x + E[1] * x1y + E[2], l1 = E[3] * x1x + E[4] * x1y + E[5], l2 = E[6] * x1x + E[7] * x1y + E[8];
  const double m0 = E[0] * x2x + E[3] * x2y + E[6], m1 = E[1] * x2x + E[4] * x2y + E[7];
  const double num = x2x * l0 + x2y * l1 + l2;
  const double den = l0 * l0 + l1 * l1 + m0 * m0 + m1 * m1;
  r2 = num * num / den;
  return den > 0.0 && sim_finite(r2);
}

// ------------------------------------------------------------------------------------------------ five-point hypotheses
__global__ void __launch_bounds__(RP_THREADS) k_relpose_solve(const RelposeArgs a) {
  __shared__ double sN[RP_TEAMS][36];             // the null-space basis N0 .. N3
  __shared__ double sMag[RP_TEAMS][2][RP_TEAM];   // pivot search: candidates | whole column
  __shared__ double sRow[RP_TEAMS][20];           // the pivot row (the pivot column's five entries in the null-space step)
  __shared__ double sC[RP_TEAMS][10][10];         // the eliminated rows' trailing coefficients, by leading monomial
  __shared__ double sNode[RP_TEAMS][24];          // root isolation: two buffers of 12 nodes
  const int pair = blockIdx.x, tid = threadIdx.x, team = tid / RP_TEAM, tl = tid % RP_TEAM, tw = (tid & 63) / RP_TEAM;
  const long long beg = a.off[pair];
  const int n = (int)(a.off[pair + 1] - beg);
  if (n < 6) return;                              // (workgroup-uniform) FEW_MATCHES: k_relpose_score reads no slot
  const int h = blockIdx.y * RP_TEAMS + team;
  const bool live = h < a.n_hyp;                  // a team past n_hyp computes along (the barriers are the workgroup's) and writes nothing
  bool ok = true;                                 // team-uniform

  // ---- sample, and the 5 x 9 system by columns: lane c < 9 holds column c = 3 i + j of the rows x2_i x1_j
  int idx[5];
  hy_sample(a.seed, pair, h, n, idx);
  double col[5];
  {
    const int ci = tl / 3, cj = tl % 3;
#pragma unroll
    for (int r = 0; r < 5; ++r) {
      const double2 x1 = pv_norm(a, a.p1[beg + idx[r]]), x2 = pv_norm(a, a.p2[beg + idx[r]]);
      const double f2 = ci == 0 ? x2.x : ci == 1 ? x2.y : 1.0, f1 = cj == 0 ? x1.x : cj == 1 ? x1.y : 1.0;
      col[r] = tl < 9 ? f2 * f1 : 0.0;
    }
  }
  double amax = 0.0;
  {
    double m = 0.0;
#pragma unroll
    for (int r = 0; r < 5; ++r) m = fmax(m, fabs(col[r]));
    sMag[team][0][tl] = m;
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 9; ++c) amax = fmax(amax, sMag[team][0][c]);
  }
  ok = ok && sim_finite(amax);
  // Gauss-Jordan by rows, the pivot of row r the largest entry among the columns not used yet
  int prow = -1;                                  // the row this lane's column is the pivot of
  int pcol[5];
#pragma unroll
  for (int r = 0; r < 5; ++r) {
    __syncthreads();                              // (the readers of sMag[.][0] are done)
    sMag[team][0][tl] = (tl < 9 && prow < 0) ? fabs(col[r]) : -1.0;
    __syncthreads();
    int p = 0;
    double pm = sMag[team][0][0];
#pragma unroll
    for (int c = 1; c < 9; ++c) { const double m = sMag[team][0][c]; if (m > pm) { pm = m; p = c; } }
    ok = ok && pm > RP_PIVOT_TOL * amax;
    pcol[r] = p;
    if (tl == p) {
      prow = r;
#pragma unroll
      for (int i = 0; i < 5; ++i) sRow[team][i] = col[i];
    }
    __syncthreads();
    const double ar = col[r] / sRow[team][r];
#pragma unroll
    for (int i = 0; i < 5; ++i) col[i] = i == r ? ar : col[i] - sRow[team][i] * ar;
  }
  // the four null vectors: free column f of rank k gives N_k[f] = 1, N_k[pcol[r]] = -A[r][f]
  {
    const unsigned freebits = (unsigned)(__ballot(tl < 9 && prow < 0) >> (RP_TEAM * tw)) & 0xffffu;
    const int rank = __popc(freebits & ((1u << tl) - 1u));
    if (tl < 9) {
#pragma unroll
      for (int k = 0; k < 4; ++k) sN[team][9 * k + tl] = 0.0;
    }
    __syncthreads();
    if (tl < 9 && prow < 0 && rank < 4) {
#pragma unroll
      for (int r = 0; r < 5; ++r) sN[team][9 * rank + pcol[r]] = -col[r];
      sN[team][9 * rank + tl] = 1.0;
    }
    __syncthreads();
  }

  // ---- the ten cubic constraints: lane l < 9 the entry (i, j) of E E^T E - tr(E E^T) E / 2, lane 9 det E
  double M[20];
#pragma unroll
  for (int q = 0; q < 20; ++q) M[q] = 0.0;
  {
    const double* N = sN[team];
    if (tl < 9) {
      const int i = tl / 3, j = tl % 3;
      double Q[10], la[4], lb[4];
#pragma unroll 1
      for (int l = 0; l < 3; ++l) {               // sum_l (E E^T)_il E_lj
#pragma unroll
        for (int q = 0; q < 10; ++q) Q[q] = 0.0;
#pragma unroll 1
        for (int k = 0; k < 3; ++k) { rp_lin(N, 3 * i + k, la); rp_lin(N, 3 * l + k, lb); rp_mul_ll(la, lb, Q); }
        rp_lin(N, 3 * l + j, la);
        rp_mul_ql(Q, la, 1.0, M);
      }
#pragma unroll
      for (int q = 0; q < 10; ++q) Q[q] = 0.0;
#pragma unroll 1
      for (int k = 0; k < 9; ++k) { rp_lin(N, k, la); rp_mul_ll(la, la, Q); }
      rp_lin(N, tl, la);
      rp_mul_ql(Q, la, -0.5, M);
    } else if (tl == 9) {
      double Q[10], la[4], lb[4];
#pragma unroll 1
      for (int c = 0; c < 3; ++c) {               // E_0c (E_1p E_2q - E_1q E_2p), (c, p, q) cyclic
        const int p = (c + 1) % 3, q2 = (c + 2) % 3;
#pragma unroll
        for (int q = 0; q < 10; ++q) Q[q] = 0.0;
        rp_lin(N, 3 + p, la); rp_lin(N, 6 + q2, lb); rp_mul_ll(la, lb, Q);
        rp_lin(N, 3 + q2, la); rp_lin(N, 6 + p, lb);
#pragma unroll
        for (int k = 0; k < 4; ++k) la[k] = -la[k];
        rp_mul_ll(la, lb, Q);
        rp_lin(N, c, la);
        rp_mul_ql(Q, la, 1.0, M);
      }
    }
  }

  // ---- Gauss-Jordan on the first ten columns, rows pivoted: the lane whose row is the pivot of column c keeps it
  int mycol = -1;
#pragma unroll
  for (int c = 0; c < 10; ++c) {
    const double m = fabs(M[c]);
    sMag[team][0][tl] = (tl < 10 && mycol < 0) ? m : -1.0;
    sMag[team][1][tl] = tl < 10 ? m : 0.0;
    __syncthreads();
    int p = 0;
    double pm = sMag[team][0][0], cm = sMag[team][1][0];
#pragma unroll
    for (int l = 1; l < 10; ++l) {
      const double x = sMag[team][0][l];
      if (x > pm) { pm = x; p = l; }
      cm = fmax(cm, sMag[team][1][l]);
    }
    ok = ok && pm > RP_PIVOT_TOL * cm && sim_finite(cm);
    if (tl == p) {
      mycol = c;
      const double inv = 1.0 / M[c];
#pragma unroll
      for (int q = 0; q < 20; ++q) { M[q] = q == c ? 1.0 : M[q] * inv; sRow[team][q] = M[q]; }
    }
    __syncthreads();
    if (tl != p && tl < 10) {
      const double f = M[c];
#pragma unroll
      for (int q = 0; q < 20; ++q) M[q] = q == c ? 0.0 : M[q] - f * sRow[team][q];
    }
  }
  if (tl < 10 && mycol >= 0) {
#pragma unroll
    for (int q = 0; q < 10; ++q) sC[team][mycol][q] = M[10 + q];
  }
  __syncthreads();

  // ---- B(z): rows (4 - z 5), (6 - z 7), (8 - z 9) acting on (x, y, 1); ascending powers of z; every lane holds all of it
  double Bx[3][4], By[3][4], Bc[3][5];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double* ra = sC[team][4 + 2 * r];
    const double* rb = sC[team][5 + 2 * r];
    Bx[r][0] = ra[2]; Bx[r][1] = ra[1] - rb[2]; Bx[r][2] = ra[0] - rb[1]; Bx[r][3] = -rb[0];
    By[r][0] = ra[5]; By[r][1] = ra[4] - rb[5]; By[r][2] = ra[3] - rb[4]; By[r][3] = -rb[3];
    Bc[r][0] = ra[9]; Bc[r][1] = ra[8] - rb[9]; Bc[r][2] = ra[7] - rb[8]; Bc[r][3] = ra[6] - rb[7]; Bc[r][4] = -rb[6];
  }
  double P[11];
#pragma unroll
  for (int q = 0; q < 11; ++q) P[q] = 0.0;
#pragma unroll
  for (int r = 0; r < 3; ++r) {                   // det = sum_r (-1)^r Bc[r] (Bx[r1] By[r2] - Bx[r2] By[r1]), r1 < r2 the other rows
    constexpr int R1[3] = {1, 0, 0}, R2[3] = {2, 2, 1};
    const int r1 = R1[r], r2 = R2[r];
    double cof[7] = {0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) cof[i + j] += Bx[r1][i] * By[r2][j] - Bx[r2][i] * By[r1][j];
    const double sg = r == 1 ? -1.0 : 1.0;
#pragma unroll
    for (int i = 0; i < 7; ++i)
#pragma unroll
      for (int j = 0; j < 5; ++j) P[i + j] += sg * cof[i] * Bc[r][j];
  }
  // ---- real roots inside the Cauchy bound, ascending
  double B = 0.0;
#pragma unroll
  for (int q = 0; q < 10; ++q) B = fmax(B, fabs(P[q] / P[10]));
  B += 1.0;
  ok = ok && sim_finite(B);
  if (!ok) B = 1.0;                               // (a void hypothesis runs along on finite numbers)
  if (tl == 0) { sNode[team][12] = -B; sNode[team][13] = B; }
  __syncthreads();
  int nr = 0;
  rp_levels<9>(P, B, sNode[team], tl, tw, nr);

  // ---- lane = root: back substitution, polish, E
  bool valid = ok && live && tl < nr;
  double E[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) E[q] = 0.0;
  if (valid) {
    double z = sNode[team][12 + 1 + tl];
    double v[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      v[r][0] = ((Bx[r][3] * z + Bx[r][2]) * z + Bx[r][1]) * z + Bx[r][0];
      v[r][1] = ((By[r][3] * z + By[r][2]) * z + By[r][1]) * z + By[r][0];
      v[r][2] = (((Bc[r][4] * z + Bc[r][3]) * z + Bc[r][2]) * z + Bc[r][1]) * z + Bc[r][0];
    }
    double w[3] = {0.0, 0.0, 0.0}, wl = -1.0;
#pragma unroll
    for (int r = 0; r < 3; ++r) {                 // the row pairs (0, 1), (0, 2), (1, 2): the longest cross product
      constexpr int A1[3] = {0, 0, 1}, A2[3] = {1, 2, 2};
      const int p = A1[r], q = A2[r];
      const double c0 = v[p][1] * v[q][2] - v[p][2] * v[q][1], c1 = v[p][2] * v[q][0] - v[p][0] * v[q][2], c2 = v[p][0] * v[q][1] - v[p][1] * v[q][0];
      const double l2 = c0 * c0 + c1 * c1 + c2 * c2;
      if (l2 > wl) { wl = l2; w[0] = c0; w[1] = c1; w[2] = c2; }
    }
    valid = w[2] != 0.0 && sim_finite(wl);
    double x = w[0] / w[2], y = w[1] / w[2];
    // two Gauss-Newton steps of (x, y, z) on the ten eliminated rows
#pragma unroll 1
    for (int it = 0; it < 2 && valid; ++it) {
      const double x2 = x * x, y2 = y * y, z2 = z * z, xy = x * y, xz = x * z, yz = y * z;
      const double lead[10] = {x2 * x, y2 * y, x2 * y, x * y2, x2 * z, x2, y2 * z, y2, xy * z, xy};
      const double ldx[10] = {3.0 * x2, 0.0, 2.0 * xy, y2, 2.0 * xz, 2.0 * x, 0.0, 0.0, yz, y};
      const double ldy[10] = {0.0, 3.0 * y2, x2, 2.0 * xy, 0.0, 0.0, 2.0 * yz, 2.0 * y, xz, x};
      const double ldz[10] = {0.0, 0.0, 0.0, 0.0, x2, 0.0, y2, 0.0, xy, 0.0};
      const double tr[10] = {x * z2, xz, x, y * z2, yz, y, z2 * z, z2, z, 1.0};
      const double tdx[10] = {z2, z, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      const double tdy[10] = {0.0, 0.0, 0.0, z2, z, 1.0, 0.0, 0.0, 0.0, 0.0};
      const double tdz[10] = {2.0 * xz, x, 0.0, 2.0 * yz, y, 0.0, 3.0 * z2, 2.0 * z, 1.0, 0.0};
      double H[6] = {0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0};
#pragma unroll
      for (int i = 0; i < 10; ++i) {
        double f = lead[i], jx = ldx[i], jy = ldy[i], jz = ldz[i];
#pragma unroll
        for (int q = 0; q < 10; ++q) {
          const double c = sC[team][i][q];
          f += c * tr[q]; jx += c * tdx[q]; jy += c * tdy[q]; jz += c * tdz[q];
        }
        H[0] += jx * jx; H[1] += jx * jy; H[2] += jx * jz; H[3] += jy * jy; H[4] += jy * jz; H[5] += jz * jz;
        g[0] += jx * f; g[1] += jy * f; g[2] += jz * f;
      }
      double C[6];
      sym3_cof(H, C);
      const double det = H[0] * C[0] + H[1] * C[1] + H[2] * C[2];
      if (!(det > 0.0) || !sim_finite(det)) break;
      const double id = 1.0 / det;
      const double dx = (C[0] * g[0] + C[1] * g[1] + C[2] * g[2]) * id, dy = (C[1] * g[0] + C[3] * g[1] + C[4] * g[2]) * id,
                   dz = (C[2] * g[0] + C[4] * g[1] + C[5] * g[2]) * id;
      if (!(sim_finite(dx) && sim_finite(dy) && sim_finite(dz))) break;
      x -= dx; y -= dy; z -= dz;
    }
    double n2 = 0.0;
#pragma unroll
    for (int q = 0; q < 9; ++q) {
      E[q] = x * sN[team][q] + y * sN[team][9 + q] + z * sN[team][18 + q] + sN[team][27 + q];
      n2 += E[q] * E[q];
    }
    const double in = 1.0 / sqrt(n2);
#pragma unroll
    for (int q = 0; q < 9; ++q) { E[q] *= in; valid = valid && sim_finite(E[q]); }
  }
  const unsigned vbits = (unsigned)(__ballot(valid) >> (RP_TEAM * tw)) & 0xffffu;
  if (live) {                                     // h < n_hyp: inside the buffers
    const size_t hyp = (size_t)pair * a.n_hyp + h;
    if (valid) {                                  // tl < nr <= RP_SLOTS
      double* o = a.E + 9 * (RP_SLOTS * hyp + tl);
#pragma unroll
      for (int q = 0; q < 9; ++q) o[q] = E[q];
    }
    if (tl == 0) a.mask[hyp] = vbits;
  }
}

// ------------------------------------------------------------------------------------------------ scores
__global__ void __launch_bounds__(RP_THREADS) k_relpose_score(const RelposeArgs a) {
  __shared__ double tile[HY_TILE * 4];
  __shared__ double red[2 * HY_WAVES];
  const int pair = blockIdx.x, blk = blockIdx.y, tid = threadIdx.x;
  const long long beg = a.off[pair];
  const int n = (int)(a.off[pair + 1] - beg);
  double* out = a.best + RP_BEST * ((size_t)pair * a.n_blk + blk);
  if (n < 6) {                                    // (workgroup-uniform) FEW_MATCHES
    hy_void_block(out);
    return;
  }
  const int cand = blk * RP_THREADS + tid, h = cand / RP_SLOTS, slot = cand % RP_SLOTS;
  bool valid = false;
  double E[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) E[q] = 0.0;         // a void candidate: denominator 0, thr^2 each
  if (h < a.n_hyp) {
    const size_t hyp = (size_t)pair * a.n_hyp + h;
    valid = (a.mask[hyp] >> slot) & 1u;
    if (valid) {
      const double* s = a.E + 9 * (RP_SLOTS * hyp + slot);
#pragma unroll
      for (int q = 0; q < 9; ++q) E[q] = s[q];
    }
  }
  const double thr2 = a.thr * a.thr;
  double cost = 0.0;
  for (int i0 = 0; i0 < n; i0 += HY_TILE) {
    const int m = min(HY_TILE, n - i0);
    __syncthreads();                              // (the readers of the previous tile are done)
    if (tid < m) {
      const double2 x1 = pv_norm(a, a.p1[beg + i0 + tid]), x2 = pv_norm(a, a.p2[beg + i0 + tid]);
      double2* d = (double2*)(tile + 4 * tid);
      d[0] = x1; d[1] = x2;
    }
    __syncthreads();
    for (int i = 0; i < m; ++i) {                 // every lane reads the same address: an LDS broadcast
      const double2* s = (const double2*)(tile + 4 * i);
      const double2 x1 = s[0], x2 = s[1];
      double r2;
      const bool has = rp_sampson2(E, x1.x, x1.y, x2.x, x2.y, r2);
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
    for (int q = 0; q < 9; ++q) out[2 + q] = E[q];
  }
}

// ------------------------------------------------------------------------------------------------ decomposition, LO, measures
struct RpPose { double R[9], t[3]; };

__device__ __forceinline__ void rp_essential(const RpPose& p, double (&E)[9]) {   // [t]x R
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    E[j] = p.t[1] * p.R[6 + j] - p.t[2] * p.R[3 + j];
    E[3 + j] = p.t[2] * p.R[j] - p.t[0] * p.R[6 + j];
    E[6 + j] = p.t[0] * p.R[3 + j] - p.t[1] * p.R[j];
  }
}
// Depths of lambda2 x2~ = lambda1 R x1~ + ts t (ts = +-1) in least squares, both in (0, max_depth]; a = R x1~ comes back for the parallax
__device__ __forceinline__ bool rp_front(const RpPose& p, const double ts, const double max_depth, const double x1x, const double x1y, const double x2x, const double x2y,
                                         double (&ra)[3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i) ra[i] = p.R[3 * i] * x1x + p.R[3 * i + 1] * x1y + p.R[3 * i + 2];
  const double aa = ra[0] * ra[0] + ra[1] * ra[1] + ra[2] * ra[2], bb = x2x * x2x + x2y * x2y + 1.0;
  const double ab = ra[0] * x2x + ra[1] * x2y + ra[2];
  const double at = ts * (ra[0] * p.t[0] + ra[1] * p.t[1] + ra[2] * p.t[2]), bt = ts * (x2x * p.t[0] + x2y * p.t[1] + p.t[2]);
  const double det = aa * bb - ab * ab;
  if (!(det > RP_RAY_TOL * aa * bb)) return false;
  const double l1 = (ab * bt - at * bb) / det, l2 = (aa * bt - ab * at) / det;
  if (!(l1 > 0.0 && l2 > 0.0)) return false;
  return !(max_depth > 0.0) || (l1 <= max_depth && l2 <= max_depth);
}
// exp([w]x)
__device__ __forceinline__ void rp_exp(const double (&w)[3], double (&X)[9]) {
  const double t2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], th = sqrt(t2);
  const double A = th < 1e-8 ? 1.0 - t2 / 6.0 : sin(th) / th, Bq = th < 1e-8 ? 0.5 - t2 / 24.0 : (1.0 - cos(th)) / t2;
  X[0] = 1.0 - Bq * (w[1] * w[1] + w[2] * w[2]); X[1] = -A * w[2] + Bq * w[0] * w[1]; X[2] = A * w[1] + Bq * w[0] * w[2];
  X[3] = A * w[2] + Bq * w[0] * w[1]; X[4] = 1.0 - Bq * (w[0] * w[0] + w[2] * w[2]); X[5] = -A * w[0] + Bq * w[1] * w[2];
  X[6] = -A * w[1] + Bq * w[0] * w[2]; X[7] = A * w[0] + Bq * w[1] * w[2]; X[8] = 1.0 - Bq * (w[0] * w[0] + w[1] * w[1]);
}
// the tangent basis of the unit t: b1 = normalise(e_k x t), k the index of the smallest |t_k|; b2 = t x b1
__device__ __forceinline__ void rp_tangent(const double (&t)[3], double (&b1)[3], double (&b2)[3]) {
  const double a0 = fabs(t[0]), a1 = fabs(t[1]), a2 = fabs(t[2]);
  if (a0 <= a1 && a0 <= a2) { b1[0] = 0.0; b1[1] = -t[2]; b1[2] = t[1]; }
  else if (a1 <= a2) { b1[0] = t[2]; b1[1] = 0.0; b1[2] = -t[0]; }
  else { b1[0] = -t[1]; b1[1] = t[0]; b1[2] = 0.0; }
  const double in = 1.0 / sqrt(b1[0] * b1[0] + b1[1] * b1[1] + b1[2] * b1[2]);
  b1[0] *= in; b1[1] *= in; b1[2] *= in;
  b2[0] = t[1] * b1[2] - t[2] * b1[1]; b2[1] = t[2] * b1[0] - t[0] * b1[2]; b2[2] = t[0] * b1[1] - t[1] * b1[0];
}

// the sums of a refinement pass over the consensus set at the pose p: H, g in the five local parameters (w | tau), and 0.5 sum r^2.
// With a = R x1~ and c = x2~ x t: num = a.c, E x1~ = t x a, E^T x2~ = R^T c, so the derivatives are cross products per match
// (w_k: a -> e_k x a, c fixed in the second view: R^T c -> R^T (c x e_k); tau_i: t -> b_i) and no 3 x 3 derivative is held.
__device__ __forceinline__ void rp_cross(const double (&u)[3], const double (&v)[3], double (&w)[3]) {
  w[0] = u[1] * v[2] - u[2] * v[1]; w[1] = u[2] * v[0] - u[0] * v[2]; w[2] = u[0] * v[1] - u[1] * v[0];
}
__device__ __forceinline__ void rp_pass(const RelposeArgs& a, const RpPose& p, const long long beg, const int n, double (&acc)[RP_NSUM],
                                        double* __restrict__ lds) {
  double bt[2][3];
  rp_tangent(p.t, bt[0], bt[1]);
#pragma unroll
  for (int q = 0; q < RP_NSUM; ++q) acc[q] = 0.0;
  for (int j = (int)threadIdx.x; j < n; j += RP_THREADS) {
    if (!a.cons[beg + j]) continue;
    const double2 x1 = pv_norm(a, a.p1[beg + j]), x2 = pv_norm(a, a.p2[beg + j]);
    const double b[3] = {x2.x, x2.y, 1.0};
    double ra[3], c[3], l[3], ac[3], ab[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) ra[i] = p.R[3 * i] * x1.x + p.R[3 * i + 1] * x1.y + p.R[3 * i + 2];
    rp_cross(b, p.t, c);
    rp_cross(p.t, ra, l);
    rp_cross(ra, c, ac);
    rp_cross(ra, b, ab);
    const double m0 = p.R[0] * c[0] + p.R[3] * c[1] + p.R[6] * c[2], m1 = p.R[1] * c[0] + p.R[4] * c[1] + p.R[7] * c[2];
    const double num = ra[0] * c[0] + ra[1] * c[1] + ra[2] * c[2];
    const double den = l[0] * l[0] + l[1] * l[1] + m0 * m0 + m1 * m1;
    if (!(den > 0.0)) continue;
    const double is = 1.0 / sqrt(den), r = num * is, hk = r / den;
    double J[5];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double e[3] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
      double wa[3], dl[3], cw[3];
      rp_cross(e, ra, wa);
      rp_cross(p.t, wa, dl);
      rp_cross(c, e, cw);
      const double d0 = p.R[0] * cw[0] + p.R[3] * cw[1] + p.R[6] * cw[2], d1 = p.R[1] * cw[0] + p.R[4] * cw[1] + p.R[7] * cw[2];
      J[k] = ac[k] * is - hk * (l[0] * dl[0] + l[1] * dl[1] + m0 * d0 + m1 * d1);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      double dl[3], xb[3];
      rp_cross(bt[i], ra, dl);
      rp_cross(b, bt[i], xb);
      const double d0 = p.R[0] * xb[0] + p.R[3] * xb[1] + p.R[6] * xb[2], d1 = p.R[1] * xb[0] + p.R[4] * xb[1] + p.R[7] * xb[2];
      const double dnum = bt[i][0] * ab[0] + bt[i][1] * ab[1] + bt[i][2] * ab[2];
      J[3 + i] = dnum * is - hk * (l[0] * dl[0] + l[1] * dl[1] + m0 * d0 + m1 * d1);
    }
#pragma unroll
    for (int q = 0; q < 5; ++q) {
#pragma unroll
      for (int s2 = q; s2 < 5; ++s2) acc[UT(5, q, s2)] += J[q] * J[s2];
      acc[15 + q] += J[q] * r;
    }
    acc[20] += 0.5 * r * r;
  }
  rs_block_sums<RP_NSUM>(acc, lds);
}

// the pose x moved by the local step dx
__device__ __forceinline__ void rp_move(const RpPose& x, const double (&dx)[5], RpPose& y) {
  const double w[3] = {dx[0], dx[1], dx[2]};
  double X[9], b1[3], b2[3];
  rp_exp(w, X);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) y.R[3 * i + j] = X[3 * i] * x.R[j] + X[3 * i + 1] * x.R[3 + j] + X[3 * i + 2] * x.R[6 + j];
  rp_tangent(x.t, b1, b2);
  double n2 = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) { y.t[i] = x.t[i] + dx[3] * b1[i] + dx[4] * b2[i]; n2 += y.t[i] * y.t[i]; }
  const double in = 1.0 / sqrt(n2);
#pragma unroll
  for (int i = 0; i < 3; ++i) y.t[i] *= in;
}

__device__ __forceinline__ void rp_write(double* __restrict__ o, const RpPose& x, const int status, const double n_in, const double rms,
                                         const double par, const int best) {
  if (threadIdx.x != 0) return;
  for (int q = 0; q < 9; ++q) o[q] = x.R[q];
  for (int q = 0; q < 3; ++q) o[9 + q] = x.t[q];
  o[12] = (double)status; o[13] = n_in; o[14] = rms; o[15] = par; o[16] = (double)best; o[17] = 0.0;
}

__global__ void __launch_bounds__(RP_THREADS) k_relpose_lo(const RelposeArgs a) {
  __shared__ double lds[RS_WAVES * RP_NSUM];
  __shared__ double s_cur[RP_NSUM], s_x[12];      // the refinement's last accepted sums and pose
  const int pair = blockIdx.x, tid = threadIdx.x;
  const long long beg = a.off[pair];
  const int n = (int)(a.off[pair + 1] - beg);
  double* o = a.out + RP_OUT * (size_t)pair;
  RpPose x;
#pragma unroll
  for (int q = 0; q < 9; ++q) x.R[q] = (q % 4 == 0) ? 1.0 : 0.0;
#pragma unroll
  for (int q = 0; q < 3; ++q) x.t[q] = 0.0;
  if (n < 6) { rp_write(o, x, RP_FEW_MATCHES, 0.0, HY_NAN, HY_NAN, -1); return; }   // (workgroup-uniform, like every branch below)
  // the lowest (cost, 10 h + slot) over the score blocks, in block order: the same in every lane
  const double* b = a.best + RP_BEST * (size_t)pair * a.n_blk;
  double gc, gk;
  const int win = hy_winner<RP_BEST>(b, a.n_blk, gc, gk);
  if (!(gc < HY_INF)) { rp_write(o, x, RP_DEGENERATE, 0.0, HY_NAN, HY_NAN, -1); return; }   // every slot void
  const int best = (int)gk / RP_SLOTS;
  double E[9];
#pragma unroll
  for (int q = 0; q < 9; ++q) E[q] = b[RP_BEST * win + 2 + q];
  const double thr2 = a.thr * a.thr;
  int status = RP_OK;
  // ---- E = U diag V^T; the third columns are the cross products of the first two, so det U = det V = +1
  RpPose cand[2];                                 // R_a, R_b; t = +-u3 in .t of both
  {
    double U[3][3], V[3][3], d[3];
    hy_canon_svd(E, U, V, d);
    // U W = [u2, -u1, u3], U W^T = [-u2, u1, u3]
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const double pl = U[i][1] * V[j][0] - U[i][0] * V[j][1], ax = U[i][2] * V[j][2];
        cand[0].R[3 * i + j] = pl + ax;
        cand[1].R[3 * i + j] = -pl + ax;
        if (!sim_finite(pl + ax)) status = RP_DEGENERATE;
      }
      cand[0].t[i] = U[i][2]; cand[1].t[i] = U[i][2];
    }
  }
  if (status != RP_OK) { rp_write(o, x, RP_DEGENERATE, 0.0, HY_NAN, HY_NAN, best); return; }
  // ---- votes of the matches within thr of the winning E
  {
    double vote[4] = {0.0, 0.0, 0.0, 0.0};
    for (int j = tid; j < n; j += RP_THREADS) {
      const double2 x1 = pv_norm(a, a.p1[beg + j]), x2 = pv_norm(a, a.p2[beg + j]);
      double r2, ra[3];
      if (!rp_sampson2(E, x1.x, x1.y, x2.x, x2.y, r2) || !(r2 <= thr2)) continue;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (rp_front(cand[k >> 1], (k & 1) ? -1.0 : 1.0, a.max_depth, x1.x, x1.y, x2.x, x2.y, ra)) vote[k] += 1.0;
    }
    rs_block_sums<4>(vote, lds);
    int w = 0;
    double wv = vote[0];
    if (vote[1] > wv) { wv = vote[1]; w = 1; }
    if (vote[2] > wv) { wv = vote[2]; w = 2; }
    if (vote[3] > wv) { wv = vote[3]; w = 3; }
    if (!(wv > 0.0)) status = RP_BEHIND;          // candidate 0
    x = (w < 2) ? cand[0] : cand[1];
    if (w & 1) {
#pragma unroll
      for (int i = 0; i < 3; ++i) x.t[i] = -x.t[i];
    }
  }
  // ---- local optimisation
  for (int round = 0; round < a.lo_rounds && status == RP_OK; ++round) {
    double Ex[9];
    rp_essential(x, Ex);
    double cn[1] = {0.0};
    for (int j = tid; j < n; j += RP_THREADS) {   // every lane writes the bytes it reads back in the passes (same stride)
      const double2 x1 = pv_norm(a, a.p1[beg + j]), x2 = pv_norm(a, a.p2[beg + j]);
      double r2, ra[3];
      const unsigned char in = rp_sampson2(Ex, x1.x, x1.y, x2.x, x2.y, r2) && r2 <= thr2 && rp_front(x, 1.0, a.max_depth, x1.x, x1.y, x2.x, x2.y, ra) ? 1 : 0;
      a.cons[beg + j] = in;
      cn[0] += (double)in;
    }
    rs_block_sums<1>(cn, lds);
    if (!(cn[0] > 0.0)) break;
    // ba_resect's step 3 in the five local parameters.  The last accepted pose and its sums live in LDS (every lane holds the
    // same values): a pass keeps only the trial pose and its own sums in registers
    double acc[RP_NSUM];
    RpPose xt = x;
    double lam = 1e-4;
    bool first = true, small = false;
    int it = 0;
    for (;;) {
      rp_pass(a, xt, beg, n, acc, lds);
      if (first || acc[20] <= s_cur[20] * (1.0 + TRK_COST_SLACK)) {   // (workgroup-uniform)
        __syncthreads();                          // (hy_keep, spelled out: a flat view of RpPose moves this kernel's code)
        if (tid == 0) {
#pragma unroll
          for (int q = 0; q < RP_NSUM; ++q) s_cur[q] = acc[q];
#pragma unroll
          for (int q = 0; q < 9; ++q) s_x[q] = xt.R[q];
#pragma unroll
          for (int q = 0; q < 3; ++q) s_x[9 + q] = xt.t[q];
        }
        __syncthreads();
        if (!first) lam = fmax(0.1 * lam, 1e-12);
      } else {
        lam *= 10.0;
      }
      first = false;
      if (small || it >= a.iters) break;
      ++it;
      double dx[5];
#pragma unroll
      for (int q = 0; q < RP_NSUM; ++q) acc[q] = s_cur[q];
      if (!lm_step(acc, lam, false, dx)) { status = RP_DEGENERATE; break; }
      double d2 = 0.0;
#pragma unroll
      for (int q = 0; q < 5; ++q) d2 += dx[q] * dx[q];
#pragma unroll
      for (int q = 0; q < 9; ++q) x.R[q] = s_x[q];
#pragma unroll
      for (int q = 0; q < 3; ++q) x.t[q] = s_x[9 + q];
      rp_move(x, dx, xt);
      small = sqrt(d2) <= 1e-14;
    }
#pragma unroll
    for (int q = 0; q < 9; ++q) x.R[q] = s_x[q];
#pragma unroll
    for (int q = 0; q < 3; ++q) x.t[q] = s_x[9 + q];
  }
  // ---- measures at the final pose
  double m3[3] = {0.0, 0.0, 0.0};                 // inliers | sum r^2 | sum of the angles
  {
    double Ex[9];
    rp_essential(x, Ex);
    for (int j = tid; j < n; j += RP_THREADS) {
      const double2 x1 = pv_norm(a, a.p1[beg + j]), x2 = pv_norm(a, a.p2[beg + j]);
      double r2, ra[3];
      if (!(rp_sampson2(Ex, x1.x, x1.y, x2.x, x2.y, r2) && r2 <= thr2 && rp_front(x, 1.0, a.max_depth, x1.x, x1.y, x2.x, x2.y, ra))) continue;
      const double c0 = ra[1] - ra[2] * x2.y, c1 = ra[2] * x2.x - ra[0], c2 = ra[0] * x2.y - ra[1] * x2.x;
      m3[0] += 1.0; m3[1] += r2;
      m3[2] += atan2(sqrt(c0 * c0 + c1 * c1 + c2 * c2), ra[0] * x2.x + ra[1] * x2.y + ra[2]);
      a.inl[beg + j] = 1;
    }
    rs_block_sums<3>(m3, lds);
  }
  const bool any = m3[0] > 0.0;
  const double rms = any ? a.fbar * sqrt(m3[1] / m3[0]) : HY_NAN;
  const double par = any ? (m3[2] / m3[0]) * 57.29577951308232 : HY_NAN;
  if (status == RP_OK) {
    if (m3[0] < (double)a.min_inliers) status = RP_FEW_INLIERS;
    else if (a.min_parallax > 0.0 && !(par >= a.min_parallax)) status = RP_LOW_PARALLAX;
  }
  rp_write(o, x, status, m3[0], rms, par, best);
}

}  // namespace ba
