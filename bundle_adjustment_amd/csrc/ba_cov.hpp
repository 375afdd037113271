// Marginal covariances after a solve (ba_covariance, include/ba_hip.h): kernels of the device path.
//
// Sigma = (J^T w J)^-1 over the free parameters, through the Schur complement the solver is built on:
//   S       = U - W V^-1 W^T          U = Hcc (camera blocks), V_p = Hpp (3x3), W = camera-point blocks
//   Sigma_c = S^-1                    dense fp64, N = NB Nc <= COV_MAX_N
//   Sigma_p = V_p^-1 + V_p^-1 (sum_{i,j in obs(p)} W_i^T Sigma[c_i, c_j] W_j) V_p^-1
// The dense matrix lives in ONE row-major buffer of Npad x Npad doubles (Npad = N rounded up to the tile T = 64; the
// padding is the identity, so every tile of the blocked algorithms is a full tile and the padding never couples to the
// problem's rows).  Only its lower triangle (row >= column) is assembled and read; the blocked Cholesky
// (potrf), triangular inverse (trtri) and L^-T L^-1 product (lauum) overwrite it in place, tile row by tile row, with
// every O(N^3) tile product on v_mfma_f64_16x16x4f64 (cov_tile_mma).  Kernels are templates over the camera model
// (ba_models.hpp) where they touch observations; the dense stages are model-free.
#pragma once
#include "ba_kernels.hpp"

namespace ba {

constexpr int COV_T = 64;            // tile edge of the blocked dense algorithms
constexpr int COV_MAX_N = 16384;     // largest camera system (2 GiB of fp64)
constexpr int COV_LDS = COV_T + 4;   // row stride of the LDS operand slabs (doubles)
constexpr double COV_RCOND_DEFAULT = 1e-10;   // rank test of ba_covariance when the caller passes rcond <= 0
constexpr int COV_FAIL_NONE = 0x7f7f7f7f;   // failure words are memset to 0x7f bytes: "nothing failed"
// point status (k_cov_points): free and determined / held / seen from one camera only (depth unobservable) / rank test failed
enum { COV_PT_OK = 0, COV_PT_HELD = 1, COV_PT_ONECAM = 2, COV_PT_FAIL = 3 };

typedef double cov_d4 __attribute__((ext_vector_type(4)));

__device__ inline bool cov_param_held(const unsigned short* __restrict__ cam_held, int fixed_cam, int nb, int r) {
  const int c = r / nb;
  return c == fixed_cam || ((cam_held_bits(cam_held, c) >> (r - c * nb)) & 1u);
}
// lower-triangle read of the symmetric dense matrix
__device__ inline double cov_sym(const double* __restrict__ A, size_t ld, int r, int c) {
  return r >= c ? A[(size_t)r * ld + c] : A[(size_t)c * ld + r];
}

// ------------------------------------------------------------------------------------------------ per point
// Thread per point (caller order pc, slot s = slot[pc]): status, V^-1 (packed 00 01 02 11 12 22) and the rank test of V
// for a free point seen from two or more cameras (or from one, with a prior: pt_info, nullable): a Cholesky pivot d_k <= rcond V_kk fails, the smallest such caller
// index goes to fail[1].
__global__ void __launch_bounds__(256)
k_cov_points(const int* __restrict__ slot, const int* __restrict__ pt_off, const int* __restrict__ p_cam,
             const double* __restrict__ Hpp, const unsigned char* __restrict__ pt_held, int n_pts, double rcond,
             unsigned char* __restrict__ status, double* __restrict__ Vinv, int* __restrict__ fail,
             const double* __restrict__ pt_info) {
  const int pc = blockIdx.x * 256 + threadIdx.x;
  if (pc >= n_pts) return;
  const int s = slot[pc];
  const int beg = pt_off[s], end = pt_off[s + 1];
  unsigned char st = COV_PT_OK;
  if (pt_held && pt_held[s]) {
    st = COV_PT_HELD;
  } else {
    bool one = true;
    for (int j = beg + 1; j < end; ++j) one = one && p_cam[j] == p_cam[beg];
    if (one && pt_info) {                // a non-zero prior block (ba_set_priors, slot order) fixes the depth: an ordinary point
      bool prior = false;
      for (int q = 0; q < 6; ++q) prior = prior || pt_info[6 * (size_t)s + q] != 0.0;
      one = !prior;
    }
    if (one) st = COV_PT_ONECAM;
  }
  double inv[6] = {0, 0, 0, 0, 0, 0};
  if (st == COV_PT_OK) {
    const double* h = Hpp + 6 * (size_t)s;
    // 3x3 Cholesky pivots, each against its own original diagonal entry
    const double d0 = h[0];
    const double l10 = h[1] / sqrt(d0), l20 = h[2] / sqrt(d0);
    const double d1 = h[3] - l10 * l10;
    const double l21 = (h[4] - l20 * l10) / sqrt(d1);
    const double d2 = h[5] - l20 * l20 - l21 * l21;
    if (!(d0 > rcond * h[0]) || !(d1 > rcond * h[3]) || !(d2 > rcond * h[5]) || !(h[0] > 0.0)) {
      st = COV_PT_FAIL;
      atomicMin(fail + 1, pc);
    } else {
      sym3_inverse(h, inv);
    }
  }
  status[s] = st;
#pragma unroll
  for (int q = 0; q < 6; ++q) Vinv[6 * (size_t)s + q] = inv[q];
}

// ------------------------------------------------------------------------------------------------ assembly
// Diagonal blocks of S from Hcc (packed upper triangles; the fixed camera's block and held rows are zero there), the
// identity on the padding.  Thread per (camera, packed entry); padding rows by the threads past the cameras.
template <int NB>
__global__ void __launch_bounds__(256)
k_cov_diag(const double* __restrict__ Hcc, int n_cams, int n_pad, double* __restrict__ A) {
  constexpr int NH = NB * (NB + 1) / 2;
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int n = NB * n_cams;
  if (t < NH * n_cams) {
    const int c = t / NH, q = t - c * NH;
    int i = 0;
    while (q >= UT(NB, i, NB - 1) + 1) ++i;                 // packed row i holds entries UT(i, i) .. UT(i, NB - 1)
    const int j = i + (q - UT(NB, i, i));
    A[(size_t)(NB * c + j) * n_pad + NB * c + i] = Hcc[(size_t)NH * c + q];   // lower: row j >= column i
  } else {
    const int r = n + (t - NH * n_cams);
    if (r < n_pad) A[(size_t)r * n_pad + r] = 1.0;
  }
}

// W = Jc^T diag(w) Jp of every point-ordered observation (NB x 3, row-major), from the camera model's fp64 Jacobian factors
// and the IRLS weights the linearisation uses.  Observations of a point seen from one camera only take their own share
// Jc^T w Jc back out of U (the exact marginalisation of such a point removes it: W V^+ W^T equals it).
template <class CM>
__global__ void __launch_bounds__(256)
k_cov_w(const double* __restrict__ cs, const double* __restrict__ intr, const double* __restrict__ ptab,
        const int* __restrict__ pt_off, const int* __restrict__ p_cam, const UvArr p_uv, const unsigned char* __restrict__ status,
        int n_pts, double fx, double fy, double cx, double cy, double fscale, int loss, double* __restrict__ Wbuf,
        double* __restrict__ A, int n_pad) {
  constexpr int NB = CM::NB;
  const int s = blockIdx.x * 4 + (threadIdx.x >> 6);       // a wave per point slot, lanes over its observations
  if (s >= n_pts) return;
  const int beg = pt_off[s], end = pt_off[s + 1];
  const unsigned char st = status[s];
  const double4 X = *(const double4*)(ptab + PT * (size_t)s);
  for (int j = beg + (threadIdx.x & 63); j < end; j += 64) {
    const int c = p_cam[j];
    double cam[CM::CAM];
    CM::load_cam(cs, intr, c, cam);
    typename CM::template Obs<double> g;
    CM::template geom<false, double, double>(cam, X.x, X.y, X.z, fx, fy, g);
    const double2 uv = p_uv[j];
    double ru, rv;
    CM::residual(g, uv.x, uv.y, fx, fy, cx, cy, ru, rv);
    double w0 = 1.0, w1 = 1.0;
    if (loss != LOSS_LINEAR) {
      double t;
      robust_loss<false>(loss, ru, fscale, t, w0);
      robust_loss<false>(loss, rv, fscale, t, w1);
    }
    double J0[NB], J1[NB];
    CM::jac_rows(g, X.x, X.y, X.z, J0, J1);
    const double* M = cs + CS * (size_t)c + 12;                // rotation columns: pre-M rows times M
    const double a0[3] = {J0[0], J0[1], J0[2]}, a1[3] = {J1[0], J1[1], J1[2]};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      J0[k] = a0[0] * M[k] + a0[1] * M[3 + k] + a0[2] * M[6 + k];
      J1[k] = a1[0] * M[k] + a1[1] * M[3 + k] + a1[2] * M[6 + k];
    }
    const double* Pm = CM::pm(g);                              // Jp = -Pm
    double* W = Wbuf + (size_t)NB * 3 * j;
#pragma unroll
    for (int a = 0; a < NB; ++a)
#pragma unroll
      for (int k = 0; k < 3; ++k) W[3 * a + k] = -(w0 * J0[a] * Pm[k] + w1 * J1[a] * Pm[3 + k]);
    if (st == COV_PT_ONECAM) {
      double* D = A + (size_t)NB * c * n_pad + NB * c;
      for (int a = 0; a < NB; ++a)
        for (int b = 0; b <= a; ++b) unsafeAtomicAdd(D + (size_t)a * n_pad + b, -(w0 * J0[a] * J0[b] + w1 * J1[a] * J1[b]));
    }
  }
}

// j of the pair index t = j (j + 1) / 2 + i, 0 <= i <= j
__device__ inline void cov_pair_decode(long long t, int& i, int& j) {
  long long jj = (long long)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
  while (jj * (jj + 1) / 2 > t) --jj;
  while ((jj + 1) * (jj + 2) / 2 <= t) ++jj;
  j = (int)jj;
  i = (int)(t - jj * (jj + 1) / 2);
}
// first slot s with poff[s + 1] > q (poff: exclusive scan of the per-slot pair counts, n + 1 entries)
__device__ inline int cov_pair_point(const long long* __restrict__ poff, int n, long long q) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (poff[mid] <= q) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// S -= W_i V^-1 W_j^T for every pair i <= j of observations of a free, determined point: a thread per (point, pair), the
// pairs numbered by the scan poff of L_p (L_p + 1) / 2 over the point-ordered observations (tracks of any length spread
// evenly over the grid).  Lower triangle only: a pair of two cameras goes to the block below the diagonal, a pair of two
// observations of the same camera to its diagonal block as W_i V^-1 W_j^T + its transpose.  fp64 atomics: the sum order
// is not fixed (ba_covariance does not promise bit-reproducible results).
template <int NB>
__global__ void __launch_bounds__(256)
k_cov_pairs(const long long* __restrict__ poff, int n_pts, const int* __restrict__ pt_off, const int* __restrict__ p_cam,
            const unsigned char* __restrict__ status, const double* __restrict__ Vinv, const double* __restrict__ Wbuf,
            double* __restrict__ A, int n_pad) {
  const long long total = poff[n_pts];
  for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < total; q += (long long)gridDim.x * 256) {
    const int s = cov_pair_point(poff, n_pts, q);
    if (status[s] != COV_PT_OK) continue;
    int i, j;
    cov_pair_decode(q - poff[s], i, j);
    const int oi = pt_off[s] + i, oj = pt_off[s] + j;
    const int ci = p_cam[oi], cj = p_cam[oj];
    const double* vi = Vinv + 6 * (size_t)s;
    const double v[6] = {vi[0], vi[1], vi[2], vi[3], vi[4], vi[5]};
    const double* Wi = Wbuf + (size_t)NB * 3 * oi;
    const double* Wj = Wbuf + (size_t)NB * 3 * oj;
    // row a of W_i V^-1 against rows b of W_j: B[a][b] = (W_i V^-1)_a . (W_j)_b
    const bool lower = ci > cj, same = ci == cj;
    double* blk = A + (size_t)NB * (lower || same ? ci : cj) * n_pad + NB * (lower || same ? cj : ci);
    for (int a = 0; a < NB; ++a) {
      double u[3];
      sym3_mul(v, Wi + 3 * a, u);
      for (int b = 0; b < NB; ++b) {
        const double* wb = Wj + 3 * b;
        const double x = u[0] * wb[0] + u[1] * wb[1] + u[2] * wb[2];   // B[a][b]
        if (lower) {
          unsafeAtomicAdd(blk + (size_t)a * n_pad + b, -x);
        } else if (!same) {
          unsafeAtomicAdd(blk + (size_t)b * n_pad + a, -x);          // block (cj, ci) gets B^T
        } else if (i == j) {
          if (b <= a) unsafeAtomicAdd(blk + (size_t)a * n_pad + b, -x);
        } else {                                                       // B + B^T on the lower triangle, diagonal twice
          if (b < a) unsafeAtomicAdd(blk + (size_t)a * n_pad + b, -x);
          else if (b > a) unsafeAtomicAdd(blk + (size_t)b * n_pad + a, -x);
          else unsafeAtomicAdd(blk + (size_t)a * n_pad + a, -2.0 * x);
        }
      }
    }
  }
}

// Held rows / columns (masks and the fixed camera): value on the diagonal, zero elsewhere, lower triangle.  A workgroup
// per parameter row r (blockIdx.y), grid-stride along it.  value 1 before the factorisation (identity rows, as in
// ba_schur_system), 0 on the inverse (Sigma is conditional on the held values).
__global__ void __launch_bounds__(256)
k_cov_held(const unsigned short* __restrict__ cam_held, int fixed_cam, int nb, int n, int n_pad, double value, double* __restrict__ A) {
  const int r = blockIdx.y;
  if (r >= n || !cov_param_held(cam_held, fixed_cam, nb, r)) return;
  for (int t = blockIdx.x * 256 + threadIdx.x; t < n_pad; t += gridDim.x * 256) {
    if (t <= r) A[(size_t)r * n_pad + t] = (t == r) ? value : 0.0;
    if (t > r) A[(size_t)t * n_pad + r] = 0.0;
  }
}
__global__ void k_cov_save_diag(const double* __restrict__ A, int n_pad, double* __restrict__ d) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r < n_pad) d[r] = A[(size_t)r * n_pad + r];
}

// ------------------------------------------------------------------------------------------------ tile product
// acc (one 64x64 tile per workgroup of 4 waves; each wave a 32x32 quadrant as 2x2 MFMA tiles of 16x16) += op(A) op(B)
// over K (a multiple of 16):  op(A)[r][k] = TA ? A[k * lda + r] : A[r * lda + k],  op(B)[k][c] = TB ? B[c * ldb + k] :
// B[k * ldb + c].  Operands go through LDS as k-major slabs of 16 x 64 (the next slab's global loads are issued before
// the current one is multiplied).  v_mfma_f64_16x16x4f64 lane layout (tools/microbench/mfma_f64_probe.hip): A operand
// lane l = A[l % 16][k = l / 16], B operand lane l = B[k = l / 16][l % 16], result register e of lane l = D[4 e + l / 16][l % 16].
template <bool TA, bool TB>
__device__ inline void cov_tile_mma(const double* __restrict__ Ag, size_t lda, const double* __restrict__ Bg, size_t ldb, int K,
                                    cov_d4 (&acc)[2][2]) {
  __shared__ double sA[16][COV_LDS], sB[16][COV_LDS];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int qr = (w >> 1) * 32, qc = (w & 1) * 32;
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n) acc[m][n] = (cov_d4){0.0, 0.0, 0.0, 0.0};
  // per slab a thread loads 4 consecutive doubles of A and of B: "row-major" operand (r, k): row tid / 4, k 4 (tid % 4) ..;
  // "k-major" operand (k, r): k tid / 16, r 4 (tid % 16) ..
  double ra[4], rb[4];
  auto load = [&](int k0) {
    if (TA) { const double* p = Ag + (size_t)(k0 + (tid >> 4)) * lda + 4 * (tid & 15); for (int e = 0; e < 4; ++e) ra[e] = p[e]; }
    else    { const double* p = Ag + (size_t)(tid >> 2) * lda + k0 + 4 * (tid & 3);   for (int e = 0; e < 4; ++e) ra[e] = p[e]; }
    if (TB) { const double* p = Bg + (size_t)(tid >> 2) * ldb + k0 + 4 * (tid & 3);   for (int e = 0; e < 4; ++e) rb[e] = p[e]; }
    else    { const double* p = Bg + (size_t)(k0 + (tid >> 4)) * ldb + 4 * (tid & 15); for (int e = 0; e < 4; ++e) rb[e] = p[e]; }
  };
  load(0);
  for (int k0 = 0; k0 < K; k0 += 16) {
    __syncthreads();                                          // the previous slab has been read
    if (TA) { for (int e = 0; e < 4; ++e) sA[tid >> 4][4 * (tid & 15) + e] = ra[e]; }
    else    { for (int e = 0; e < 4; ++e) sA[4 * (tid & 3) + e][tid >> 2] = ra[e]; }
    if (TB) { for (int e = 0; e < 4; ++e) sB[4 * (tid & 3) + e][tid >> 2] = rb[e]; }
    else    { for (int e = 0; e < 4; ++e) sB[tid >> 4][4 * (tid & 15) + e] = rb[e]; }
    __syncthreads();
    if (k0 + 16 < K) load(k0 + 16);
#pragma unroll
    for (int k4 = 0; k4 < 16; k4 += 4) {
      const int kk = k4 + (lane >> 4);
      double a[2], b[2];
#pragma unroll
      for (int m = 0; m < 2; ++m) a[m] = sA[kk][qr + 16 * m + (lane & 15)];
#pragma unroll
      for (int n = 0; n < 2; ++n) b[n] = sB[kk][qc + 16 * n + (lane & 15)];
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n) acc[m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[m], b[n], acc[m][n], 0, 0, 0);
    }
  }
}
// C (64x64 tile at C, leading dimension ldc) = alpha acc + beta C
__device__ inline void cov_tile_store(double* __restrict__ C, size_t ldc, const cov_d4 (&acc)[2][2], double alpha, double beta) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int qr = (w >> 1) * 32, qc = (w & 1) * 32;
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        double* p = C + (size_t)(qr + 16 * m + 4 * e + (lane >> 4)) * ldc + qc + 16 * n + (lane & 15);
        *p = alpha * acc[m][n][e] + (beta != 0.0 ? beta * *p : 0.0);
      }
}
// (i, j), j <= i, of the t-th tile of a lower triangle of tiles numbered row by row
__device__ inline void cov_tri_decode(int t, int& i, int& j) {
  int ii = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
  while (ii * (ii + 1) / 2 > t) --ii;
  while ((ii + 1) * (ii + 2) / 2 <= t) ++ii;
  i = ii;
  j = t - ii * (ii + 1) / 2;
}

// ------------------------------------------------------------------------------------------------ 64x64 diagonal tiles
// Load the lower triangle of diagonal tile kt into LDS (upper part zero).
__device__ inline void cov_load_diag(const double* __restrict__ A, size_t ld, int kt, double (&a)[COV_T][COV_T + 1]) {
  const double* src = A + (size_t)kt * COV_T * ld + (size_t)kt * COV_T;
  for (int e = threadIdx.x; e < COV_T * COV_T; e += 256) {
    const int r = e / COV_T, c = e % COV_T;
    a[r][c] = c <= r ? src[(size_t)r * ld + c] : 0.0;
  }
  __syncthreads();
}
// inv = L^-1 of the lower-triangular tile in a (thread c < 64: column c by forward substitution)
__device__ inline void cov_trinv_lds(const double (&a)[COV_T][COV_T + 1], double (&inv)[COV_T][COV_T + 1]) {
  const int c = threadIdx.x;
  if (c < COV_T) {
    for (int i = 0; i < COV_T; ++i) {
      if (i < c) { inv[i][c] = 0.0; continue; }
      double s = (i == c) ? 1.0 : 0.0;
      for (int k = c; k < i; ++k) s -= a[i][k] * inv[k][c];
      inv[i][c] = s / a[i][i];
    }
  }
  __syncthreads();
}
__device__ inline void cov_store_tile(const double (&a)[COV_T][COV_T + 1], double* __restrict__ dst, size_t ld) {
  for (int e = threadIdx.x; e < COV_T * COV_T; e += 256) dst[(size_t)(e / COV_T) * ld + e % COV_T] = a[e / COV_T][e % COV_T];
}

// potrf, diagonal tile kt: unblocked Cholesky in LDS with the rank test -- pivot d_k of global column g = 64 kt + k fails
// when d_k <= rcond * dS[g] (dS: S's diagonal before the factorisation; columns g >= n are the padding); the smallest
// failing column goes to fail[0] (the host reads it once, after the last kernel) and the factorisation goes on with
// d_k = 1 where d_k is not positive.  Writes L_kk (upper part zero) and L_kk^-1 (tinv, for the panel).
__global__ void __launch_bounds__(256)
k_cov_potrf_diag(double* __restrict__ A, int n_pad, int kt, const double* __restrict__ dS, int n, double rcond,
                 int* __restrict__ fail, double* __restrict__ tinv) {
  __shared__ double a[COV_T][COV_T + 1], inv[COV_T][COV_T + 1];
  cov_load_diag(A, n_pad, kt, a);
  for (int j = 0; j < COV_T; ++j) {
    if (threadIdx.x == 0) {
      const int g = kt * COV_T + j;
      double d = a[j][j];
      if (g < n && !(d > rcond * dS[g])) atomicMin(fail, g);
      if (!(d > 0.0)) d = 1.0;
      a[j][j] = sqrt(d);
    }
    __syncthreads();
    const double s = a[j][j];
    if ((int)threadIdx.x > j && threadIdx.x < COV_T) a[threadIdx.x][j] /= s;
    __syncthreads();
    for (int e = threadIdx.x; e < COV_T * COV_T; e += 256) {
      const int r = e / COV_T, c = e % COV_T;
      if (c > j && c <= r) a[r][c] -= a[r][j] * a[c][j];
    }
    __syncthreads();
  }
  cov_trinv_lds(a, inv);
  cov_store_tile(a, A + (size_t)kt * COV_T * n_pad + (size_t)kt * COV_T, n_pad);
  cov_store_tile(inv, tinv, COV_T);
}
// potrf panel: L_ik = A_ik L_kk^-T for the tiles below kt (in place: the tile is read whole before it is written)
__global__ void __launch_bounds__(256)
k_cov_potrf_panel(double* __restrict__ A, int n_pad, int kt, const double* __restrict__ tinv) {
  const int i = kt + 1 + blockIdx.x;
  double* Aik = A + (size_t)i * COV_T * n_pad + (size_t)kt * COV_T;
  cov_d4 acc[2][2];
  cov_tile_mma<false, true>(Aik, n_pad, tinv, COV_T, COV_T, acc);
  __syncthreads();
  cov_tile_store(Aik, n_pad, acc, 1.0, 0.0);
}
// potrf trailing update: A_ij -= L_ik L_jk^T for kt < j <= i
__global__ void __launch_bounds__(256)
k_cov_potrf_update(double* __restrict__ A, int n_pad, int kt) {
  int i, j;
  cov_tri_decode(blockIdx.x, i, j);
  i += kt + 1; j += kt + 1;
  cov_d4 acc[2][2];
  cov_tile_mma<false, true>(A + (size_t)i * COV_T * n_pad + (size_t)kt * COV_T, n_pad,
                            A + (size_t)j * COV_T * n_pad + (size_t)kt * COV_T, n_pad, COV_T, acc);
  cov_tile_store(A + (size_t)i * COV_T * n_pad + (size_t)j * COV_T, n_pad, acc, -1.0, 1.0);
}

// trtri (X = L^-1 in place, tile columns from the last to the first), column jt:
//   diag:   X_jj = L_jj^-1 (also into tinv)
//   panel:  P_i = L_ij X_jj for i > jt (into the panel buffer P, 64-wide)
//   update: X_ij = -sum_{l = jt+1 .. i} X_il P_l   (X_il: columns already inverted; X_ii lower triangular)
__global__ void __launch_bounds__(256)
k_cov_trtri_diag(double* __restrict__ A, int n_pad, int jt, double* __restrict__ tinv) {
  __shared__ double a[COV_T][COV_T + 1], inv[COV_T][COV_T + 1];
  cov_load_diag(A, n_pad, jt, a);
  cov_trinv_lds(a, inv);
  cov_store_tile(inv, A + (size_t)jt * COV_T * n_pad + (size_t)jt * COV_T, n_pad);
  cov_store_tile(inv, tinv, COV_T);
}
__global__ void __launch_bounds__(256)
k_cov_trtri_panel(const double* __restrict__ A, int n_pad, int jt, const double* __restrict__ tinv, double* __restrict__ P) {
  const int i = jt + 1 + blockIdx.x;
  cov_d4 acc[2][2];
  cov_tile_mma<false, false>(A + (size_t)i * COV_T * n_pad + (size_t)jt * COV_T, n_pad, tinv, COV_T, COV_T, acc);
  cov_tile_store(P + (size_t)i * COV_T * COV_T, COV_T, acc, 1.0, 0.0);
}
__global__ void __launch_bounds__(256)
k_cov_trtri_update(double* __restrict__ A, int n_pad, int jt, const double* __restrict__ P) {
  const int i = jt + 1 + blockIdx.x;
  cov_d4 acc[2][2];
  cov_tile_mma<false, false>(A + (size_t)i * COV_T * n_pad + (size_t)(jt + 1) * COV_T, n_pad, P + (size_t)(jt + 1) * COV_T * COV_T,
                             COV_T, (i - jt) * COV_T, acc);
  cov_tile_store(A + (size_t)i * COV_T * n_pad + (size_t)jt * COV_T, n_pad, acc, -1.0, 0.0);
}

// lauum (Sigma = X^T X in place, tile rows from the first to the last), row it:
//   Sigma_ij = sum_{k >= it} X_ki^T X_kj for j <= it.  Workgroup j < it writes its tile directly (it alone reads X_ij);
//   workgroup it writes the diagonal tile to D (the others still read X_ii), k_cov_lauum_copy puts it in place.
__global__ void __launch_bounds__(256)
k_cov_lauum(double* __restrict__ A, int n_pad, int it, double* __restrict__ D) {
  const int j = blockIdx.x, nt = n_pad / COV_T;
  cov_d4 acc[2][2];
  cov_tile_mma<true, false>(A + (size_t)it * COV_T * n_pad + (size_t)it * COV_T, n_pad,
                            A + (size_t)it * COV_T * n_pad + (size_t)j * COV_T, n_pad, (nt - it) * COV_T, acc);
  __syncthreads();
  if (j < it) cov_tile_store(A + (size_t)it * COV_T * n_pad + (size_t)j * COV_T, n_pad, acc, 1.0, 0.0);
  else cov_tile_store(D, COV_T, acc, 1.0, 0.0);
}
__global__ void __launch_bounds__(256)
k_cov_lauum_copy(double* __restrict__ A, int n_pad, int it, const double* __restrict__ D) {
  double* dst = A + (size_t)it * COV_T * n_pad + (size_t)it * COV_T;
  for (int e = threadIdx.x; e < COV_T * COV_T; e += 256) dst[(size_t)(e / COV_T) * n_pad + e % COV_T] = D[e];
}

// ------------------------------------------------------------------------------------------------ outputs
// Sigma_p = V^-1 + V^-1 T V^-1,  T = sum_{i, j in obs(p)} W_i^T Sigma[c_i, c_j] W_j: a wave per point slot, lanes over the
// pairs i <= j (i != j counted with its transpose), the lanes' partial sums combined by one fixed butterfly.  Held points
// get 0, points seen from one camera NaN (depth unobservable).  Packed 00 01 02 11 12 22, slot order.
template <int NB>
__global__ void __launch_bounds__(256)
k_cov_point_cov(const double* __restrict__ A, int n_pad, const int* __restrict__ pt_off, const int* __restrict__ p_cam,
                const unsigned char* __restrict__ status, const double* __restrict__ Vinv, const double* __restrict__ Wbuf,
                int n_pts, double* __restrict__ out) {
  const int s = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (s >= n_pts) return;
  const unsigned char st = status[s];
  double* o = out + 6 * (size_t)s;
  if (st != COV_PT_OK) {
    if (lane < 6) o[lane] = (st == COV_PT_HELD) ? 0.0 : __builtin_nan("");
    return;
  }
  const int beg = pt_off[s], L = pt_off[s + 1] - beg;
  const long long npair = (long long)L * (L + 1) / 2;
  double T[6] = {0, 0, 0, 0, 0, 0};
  for (long long q = lane; q < npair; q += 64) {
    int i, j;
    cov_pair_decode(q, i, j);
    const int ci = p_cam[beg + i], cj = p_cam[beg + j];
    const double* Wi = Wbuf + (size_t)NB * 3 * (beg + i);
    const double* Wj = Wbuf + (size_t)NB * 3 * (beg + j);
    // G = Sigma[c_i, c_j] W_j (NB x 3), then M = W_i^T G
    double M[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    for (int a = 0; a < NB; ++a) {
      double g[3] = {0, 0, 0};
      for (int b = 0; b < NB; ++b) {
        const double sg = cov_sym(A, n_pad, NB * ci + a, NB * cj + b);
        g[0] += sg * Wj[3 * b]; g[1] += sg * Wj[3 * b + 1]; g[2] += sg * Wj[3 * b + 2];
      }
      for (int x = 0; x < 3; ++x)
        for (int y = 0; y < 3; ++y) M[x][y] += Wi[3 * a + x] * g[y];
    }
    const double f = (i == j) ? 1.0 : 2.0;                      // (M + M^T) / 2 per ordered pair, both orders
    T[0] += f * M[0][0]; T[3] += f * M[1][1]; T[5] += f * M[2][2];
    T[1] += 0.5 * f * (M[0][1] + M[1][0]); T[2] += 0.5 * f * (M[0][2] + M[2][0]); T[4] += 0.5 * f * (M[1][2] + M[2][1]);
  }
#pragma unroll
  for (int k = 0; k < 6; ++k)
    for (int m = 32; m > 0; m >>= 1) T[k] += __shfl_xor(T[k], m, 64);
  if (lane == 0) {
    const double* v = Vinv + 6 * (size_t)s;
    // Sigma_p = v + v T v (3x3 symmetric, packed)
    double vt[3][3];
    const double Vf[3][3] = {{v[0], v[1], v[2]}, {v[1], v[3], v[4]}, {v[2], v[4], v[5]}};
    const double Tf[3][3] = {{T[0], T[1], T[2]}, {T[1], T[3], T[4]}, {T[2], T[4], T[5]}};
    for (int x = 0; x < 3; ++x)
      for (int y = 0; y < 3; ++y) vt[x][y] = Vf[x][0] * Tf[0][y] + Vf[x][1] * Tf[1][y] + Vf[x][2] * Tf[2][y];
    int q = 0;
    for (int x = 0; x < 3; ++x)
      for (int y = x; y < 3; ++y, ++q) o[q] = Vf[x][y] + vt[x][0] * Vf[0][y] + vt[x][1] * Vf[1][y] + vt[x][2] * Vf[2][y];
  }
}
// packed upper triangles of the diagonal camera blocks, Hcc's order
template <int NB>
__global__ void __launch_bounds__(256)
k_cov_cam_blocks(const double* __restrict__ A, int n_pad, int n_cams, double* __restrict__ out) {
  constexpr int NH = NB * (NB + 1) / 2;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= NH * n_cams) return;
  const int c = t / NH, q = t - c * NH;
  int i = 0;
  while (q >= UT(NB, i, NB - 1) + 1) ++i;
  const int j = i + (q - UT(NB, i, i));
  out[t] = A[(size_t)(NB * c + j) * n_pad + NB * c + i];
}
// upper triangle from the lower one (the whole matrix leaves as a full symmetric one)
__global__ void __launch_bounds__(256)
k_cov_symmetrize(double* __restrict__ A, int n_pad, int n) {
  const int r = blockIdx.y;
  for (int c = r + 1 + blockIdx.x * 256 + threadIdx.x; c < n; c += gridDim.x * 256) A[(size_t)r * n_pad + c] = A[(size_t)c * n_pad + r];
}

}  // namespace ba
