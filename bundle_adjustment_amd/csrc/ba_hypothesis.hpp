// The hypothesis stage ba_resect_ransac, ba_relative_pose, ba_homography, ba_sim3 and ba_fundamental share:
// which sample a hypothesis draws, which (cost, key) a score block and a call keep, how a refinement keeps its accepted trial,
// and the pair-shaped calls' common arguments and canonical SVD.  Device code on ba_dpp.hpp and ba_linalg.hpp (the damped step
// lm_step is there); the minimal solvers and the score of a model stay in the calls' own headers.
//
// Generator: mix(z) = the splitmix64 finaliser (z ^= z >> 30, z *= 0xBF58476D1CE4E5B9, z ^= z >> 27, z *= 0x94D049BB133111EB,
// z ^= z >> 31); draw(d) = mix(mix(mix(mix(seed + G) + item) + h) + (d + 1) G), G the golden-ratio increment of hy_sample, all
// modulo 2^64; index_d = high 64 bits of draw(d) * (n - d), raised by one past each earlier index in ascending order: K
// distinct indices below n (n >= K), a pure function of (seed, item, h, n), no retries.  item: the camera or the pair.
//
// Arg-min: a lane offers (cost, key), keys distinct over the call and HY_INF | HY_INF when it holds no model.  The lowest cost
// wins and ties go to the lower key: two DPP min-reductions per wave, the waves folded through LDS in wave order
// (hy_block_best), the score blocks in block order (hy_winner).  A block without a model writes HY_INF | 0 (hy_void_block).
#pragma once
#include "ba_dpp.hpp"
#include "ba_linalg.hpp"

namespace ba {

constexpr int HY_THREADS = 256;       // lanes of a score workgroup
constexpr int HY_WAVES = HY_THREADS / 64;
constexpr int HY_TILE = 256;          // matches per LDS tile of a two-view scoring loop
constexpr int HY_MAX_HYP = 4096;      // n_hyp of every call is 1 .. HY_MAX_HYP
constexpr double HY_INF = 1.7976931348623157e308;
constexpr double HY_AREA_TOL = 1e-6;  // |d12 x d13| <= HY_AREA_TOL max |d_ij|^2: a void triple of a sample

__device__ __forceinline__ unsigned long long hy_mix(unsigned long long z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
template <int K>
__device__ __forceinline__ void hy_sample(const unsigned long long seed, const int item, const int h, const int n, int (&idx)[K]) {
  constexpr unsigned long long G = 0x9E3779B97F4A7C15ull;
  const unsigned long long k = hy_mix(hy_mix(hy_mix(seed + G) + (unsigned long long)item) + (unsigned long long)h);
  int s[K];                                       // the earlier indices, ascending
#pragma unroll
  for (int d = 0; d < K; ++d) {
    int i = (int)__umul64hi(hy_mix(k + (unsigned long long)(d + 1) * G), (unsigned long long)(n - d));
#pragma unroll
    for (int j = 0; j < d; ++j) if (i >= s[j]) ++i;
    idx[d] = i;
    s[d] = i;
#pragma unroll
    for (int j = d; j > 0; --j) if (s[j - 1] > s[j]) { const int t = s[j - 1]; s[j - 1] = s[j]; s[j] = t; }
  }
}

// The block's lowest (cost, key) into gc | gk of every lane (red: 2 HY_WAVES doubles of LDS); true in the one lane that offered it
__device__ __forceinline__ bool hy_block_best(const double bc, const double bk, double* red, double& gc, double& gk) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const double wc = wave_min_dpp(bc);
  const double wk = wave_min_dpp(bc == wc ? bk : HY_INF);
  if (lane == 0) { red[2 * wv] = wc; red[2 * wv + 1] = wk; }
  __syncthreads();
  gc = red[0]; gk = red[1];
#pragma unroll
  for (int w = 1; w < HY_WAVES; ++w) {
    const double xc = red[2 * w], xk = red[2 * w + 1];
    if (xc < gc || (xc == gc && xk < gk)) { gc = xc; gk = xk; }
  }
  return bc == gc && bk == gk;                    // one lane: keys are distinct
}
__device__ __forceinline__ void hy_void_block(double* __restrict__ out) {
  if (threadIdx.x == 0) { out[0] = HY_INF; out[1] = 0.0; }
}
// The score block (records of STRIDE doubles, cost | key first) with the lowest (cost, key), in block order: the same in every lane
template <int STRIDE>
__device__ __forceinline__ int hy_winner(const double* __restrict__ b, const int n_blk, double& gc, double& gk) {
  int win = 0;
  gc = b[0]; gk = b[1];
  for (int k = 1; k < n_blk; ++k) {
    const double xc = b[STRIDE * k], xk = b[STRIDE * k + 1];
    if (xc < gc || (xc == gc && xk < gk)) { gc = xc; gk = xk; win = k; }
  }
  return win;
}

// The refinement's accepted trial into LDS, where every lane reads it back: the sums of its pass and its model
template <int NSUM, int NX>
__device__ __forceinline__ void hy_keep(double (&s_cur)[NSUM], double (&s_x)[NX], const double (&acc)[NSUM], const double (&x)[NX]) {
  __syncthreads();                                // (the readers of s_cur are done)
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < NSUM; ++q) s_cur[q] = acc[q];
#pragma unroll
    for (int q = 0; q < NX; ++q) s_x[q] = x[q];
  }
  __syncthreads();
}

// ---------------------------------------------------------------------------------------------- the pair-shaped calls
struct HypArgs {           // what ba_relative_pose, ba_homography, ba_sim3 and ba_fundamental pass alike: the head of their arguments
  double thr, fbar;        // the call's pixel threshold / fbar, fbar = (fx + fy) / 2
  int n_hyp, lo_rounds, iters, min_inliers;
  int n_blk;               // score blocks per pair
  unsigned long long seed;
  const long long* off;    // [pairs + 1]
  double* best;            // the call's record per (pair, score block): cost | key | model
  unsigned char* cons;     // per match: in the consensus set of the round
  unsigned char* inl;      // match_inlier (zeroed before the launch)
  double* out;             // the call's row per pair
};
struct PairArgs : HypArgs {   // the two-view calls on pixels: RelposeArgs, HomogArgs and FundArgs begin with it
  double fx, fy, cx, cy;   // K
  double max_depth;
  const double2* p1;       // pixels, first / second view
  const double2* p2;
};

__device__ __forceinline__ double2 pv_norm(const PairArgs& a, const double2 p) {
  return make_double2((p.x - a.cx) / a.fx, (p.y - a.cy) / a.fy);
}

// M = U diag(d) V^T, d descending; the first two columns of U at unit length, the third columns of U and V the cross products
// of the first two, so det U = det V = +1
__device__ __forceinline__ void hy_canon_svd(const double (&M)[9], double (&U)[3][3], double (&V)[3][3], double (&d)[3]) {
  double n2[3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) U[i][j] = M[3 * i + j];
  jacobi_svd<3, 24>(U, V);
#pragma unroll
  for (int k = 0; k < 3; ++k) n2[k] = U[0][k] * U[0][k] + U[1][k] * U[1][k] + U[2][k] * U[2][k];
  sim_order<0, 1>(U, V, n2); sim_order<1, 2>(U, V, n2); sim_order<0, 1>(U, V, n2);
#pragma unroll
  for (int k = 0; k < 3; ++k) d[k] = sqrt(n2[k]);
  const double i0 = 1.0 / d[0], i1 = 1.0 / d[1];
#pragma unroll
  for (int k = 0; k < 3; ++k) { U[k][0] *= i0; U[k][1] *= i1; }
  U[0][2] = U[1][0] * U[2][1] - U[2][0] * U[1][1]; U[1][2] = U[2][0] * U[0][1] - U[0][0] * U[2][1]; U[2][2] = U[0][0] * U[1][1] - U[1][0] * U[0][1];
  V[0][2] = V[1][0] * V[2][1] - V[2][0] * V[1][1]; V[1][2] = V[2][0] * V[0][1] - V[0][0] * V[2][1]; V[2][2] = V[0][0] * V[1][1] - V[1][0] * V[0][1];
}

}  // namespace ba
