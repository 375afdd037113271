// HIP kernels of the bundle-adjustment solve step (gfx950).
//
// Data in HBM (built once per problem in ba_set_problem, see DESIGN.md "Layout"):
//   points keep the caller's numbering when the whole camera table fits in LDS; otherwise they are
//   renumbered internally (slot[]) by the mean index of the cameras that see them, so that a run of
//   consecutive points is seen from a narrow window of cameras whenever the data has that locality
//   ptab[2][Np][8]   point records {X0 X1 X2 - y0 y1 y2 -}: one 64-byte sector per point, so a
//                    camera-ordered pass fetches everything it needs about a point with one
//                    sector; [cur] = accepted points, [1-cur] = trial points; y = PCG scratch
//   camera order:    observations of camera c are [cam_off[c], cam_off[c+1]), sorted by point;
//                    offk[c][k] cuts them into NPART equal-count chunks ("partitions")
//                    -> c_pt (int32), c_uv, c_w (double2), c_orig (caller's row), c_ptf (c_pt with
//                    the "weights are not (1, 1)" flag, written by the linearisation)
//   point order:     observations of point p are [pt_off[p], pt_off[p+1]) -> p_cam, p_uv, p_w, p_camf
//   cs[2][Nc][24]    per-camera state R t M (camera_state), camA[2][Nc][18] = R t | vtil, the
//                    packed table the point passes stage in LDS (vtil = camera vector of the pass)
//
// Camera passes (k_cam_*: a WAVE, k_camrow_*: a 16-lane row, per (camera, partition) segment).
// Workgroups are dealt round-robin over the 8 XCDs; group_of_block maps a workgroup to its segment
// so that an XCD keeps gathering from one eighth of the point table (partition x of every camera, or
// all partitions of the x-th eighth of the cameras for band-structured data) and holds it in its
// own 4 MB L2.  Speed only: results do not depend on the placement.  Per-(partition, camera)
// partial sums are combined, in fixed order, by the consuming kernel.
//
// Point passes (k_pt_*): LPP lanes per point (a 16-lane row for long tracks) walk its observations
// (software-prefetched index stream), the per-camera table sits in LDS, lanes are combined with
// DPP row shifts; workgroup ranges are grouped per XCD like the camera passes' slices.
//
// Every sum has a fixed order: results are bitwise reproducible run to run.
#pragma once
#include "ba_device.hpp"
#include "ba_dpp.hpp"
#include "ba_models.hpp"

namespace ba {

// Diagnostic build only (-DBA_STAMPS, tools/stamp_timeline.py): thread 0 of every workgroup records
// where its time goes.  Slot 0 / 7: s_memrealtime (100 MHz) at entry / exit, slots 1..6: s_memtime
// (shader clock) at the stages marked in the kernels.  The product build compiles none of it.
#ifdef BA_STAMPS
constexpr int STAMP_BLOCKS = 8192;
__device__ unsigned long long g_stamps[4][STAMP_BLOCKS * 8];
__device__ int g_dbg_mode;      // diagnostic variants of the camera pass's gather (tools/stamp_timeline.py): 0 = product path
#define BA_STAMP(kind, slot)                                                                              \
  do {                                                                                                    \
    if (threadIdx.x == 0 && blockIdx.x < STAMP_BLOCKS)                                                    \
      g_stamps[kind][blockIdx.x * 8 + (slot)] =                                                           \
          ((slot) == 0 || (slot) == 7) ? __builtin_amdgcn_s_memrealtime() : __builtin_amdgcn_s_memtime(); \
  } while (0)
#else
#define BA_STAMP(kind, slot) do { } while (0)
#endif

constexpr int NPART = 8;         // point partitions (= XCDs)
constexpr int WPB = 4;           // waves (= cameras) per workgroup in camera passes
constexpr int PT = 8;            // doubles per point record
constexpr int TA = Pinhole::TA;  // doubles per camera in camA, the reference's pinhole: R[9] t[3] vtil[6]
constexpr int TA_MAX = BalCam::TA; // the widest row of any camera model (ba_models.hpp): what the table buffers are sized for
constexpr int PT_THREADS = 1024; // threads per workgroup in point passes
constexpr int LPP = 2;           // lanes per point in point passes (short tracks)
constexpr int LPP_LONG = 16;     // one DPP row per point for long tracks (threshold chosen per problem)
constexpr int VEC_BLOCK = 64;    // threads per workgroup in camera-vector kernels (one wave)
constexpr int VEC_CAMS = Pinhole::VC;   // cameras per workgroup (CM::VC per camera model): a thread per camera reads hundreds of
                                        // strided words, i.e. one cache line per lane per load; 16 live lanes per wave spread
                                        // that over 4x the CUs

// Flagged index streams.  With a robust loss the linearisation writes, next to the IRLS weights,
// a copy of each index stream whose top bit says "this observation's weights are not (1, 1)".
// The Schur passes read that copy and fetch the 16-byte weight only for flagged observations:
// near the solution most observations are Huber inliers, and the weight streams are otherwise
// the largest share of a pass's traffic.  Bit-identical results: an unflagged weight IS (1, 1).  (Under the smooth losses
// -- soft_l1, cauchy, arctan -- almost no weight is exactly 1: every index is flagged and every weight fetched.)
constexpr int IDX_FLAG = (int)0x80000000;
constexpr int IDX_MASK = 0x7fffffff;
__device__ inline int flagged_index(int idx, double w0, double w1) { return (w0 != 1.0 || w1 != 1.0) ? (idx | IDX_FLAG) : idx; }

template <int VCM = VEC_CAMS>
__device__ inline int vec_camera(int n_cams) {      // camera of this thread in a camera-vector kernel, n_cams = none
  return (threadIdx.x < VCM) ? (int)(blockIdx.x * VCM + threadIdx.x) : n_cams;
}

// max that keeps a NaN (fmax drops it): a non-finite gradient must not read as "converged"
__device__ inline double nanmax(double a, double b) { return (a != a) ? a : ((b != b) ? b : fmax(a, b)); }
__device__ inline double wave_nanmax(double m) {
  for (int o = 32; o > 0; o >>= 1) m = nanmax(m, __shfl_xor(m, o, 64));
  return m;
}

// PCG device state, two copies indexed by iteration parity (see k_pcg_step)
struct PcgState {
  double gamma_prev, alpha_prev, gamma0;
  double q_tot;                    // -q(x_k): decrease of the quadratic model 1/2 x^T S x - g^T x since x = 0 (sum of 1/2 alpha gamma)
  int done, iters, flag;           // done: 1 converged, 2 breakdown
  int stop_model;                  // the model test (ba_options.pcg_model_tol) fired after the last iteration: the next one does not run
};

// scalar slots written by k_scalars (device `scal`)
enum { S_SSE = 0, S_RHO = 1, S_PT_GD = 2, S_PT_DDD = 3, S_PT_DD = 4, S_PT_XX = 5, S_GAIN = 6, S_LAM_NEXT = 7,
       S_CAM_GD = 8, S_CAM_DDD = 9, S_DC_R = 10, S_CAM_DD = 11, S_CAM_XX = 12, S_GMAX_C = 16, S_GMAX_P = 17,
       S_PCG_FIN = 20, S_PCG_ITERS = 21, S_COUNT = 24 };

// -------------------------------------------------------------------------------------
// small per-camera / per-point kernels
// -------------------------------------------------------------------------------------
template <class CM>
__global__ void k_cam_prepare(const double* __restrict__ cams, const double* __restrict__ intr, double* __restrict__ cs,
                              double* __restrict__ camA, int n_cams) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_cams) return;
  camera_state(cams + 6 * c, cs + CS * c);
  CM::table_row(cs + CS * c, intr + 3 * (size_t)c, camA + CM::TA * (size_t)c);      // (the pinhole ignores intr)
}

// In-place fold of nparts per-partition partial-sum arrays of n values each (multi-rank jobs, ahead of
// the all-reduce): partition 0 <- sum over the partitions in partition order.  The other partitions keep their
// (now stale) local sums: every consumer of an all-reduced array reads partition 0 only (nparts = 1).
__global__ void k_fold_parts(double* __restrict__ parts, size_t n, int nparts) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double v[NPART];
#pragma unroll
  for (int k = 0; k < NPART; ++k) v[k] = (k < nparts) ? parts[(size_t)k * n + i] : 0.0;     // all loads in flight at once
  double s = v[0];
#pragma unroll
  for (int k = 1; k < NPART; ++k) s += v[k];
  parts[i] = s;
}

// The damped system's message of a multi-rank job, gathered into ONE buffer for ONE all-reduce:
//   msg = [ u.y word, 0 | sum_k part6[k] (n6 values) | sum_k partE[k] (nE values, 0 without Schur-Jacobi blocks) | world slots ]
// Slot `rank` of the tail holds this rank's max |bp| (the per-workgroup maxima of the point half, partG), the other
// slots 0: after the sum all-reduce every rank holds every rank's maximum, and the first PCG probe takes the largest
// (the reference's gtol test) exactly as it folds partG on a single rank.  nparts: partitions to add up (1 when the
// camera passes already wrote whole lists into partition 0).
__global__ void __launch_bounds__(256)
k_fold_msg(const double* __restrict__ uy_src, const double* __restrict__ part6, size_t n6, const double* __restrict__ partE,
           size_t nE, int nparts, const double* __restrict__ partG, int nG, int rank, int world, double* __restrict__ msg) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n6 + nE) {
    const double* src = (i < n6) ? part6 + i : partE + (i - n6);
    const size_t stride = (i < n6) ? n6 : nE;
    double v[NPART];
#pragma unroll
    for (int k = 0; k < NPART; ++k) v[k] = (k < nparts) ? src[(size_t)k * stride] : 0.0;
    double s = v[0];
#pragma unroll
    for (int k = 1; k < NPART; ++k) s += v[k];
    msg[2 + i] = s;
  }
  if (blockIdx.x == 0 && threadIdx.x < 64) {
    double m = 0.0;
    for (int b = threadIdx.x; b < nG; b += 64) m = nanmax(m, partG[b]);
    m = wave_nanmax(m);
    double* tail = msg + 2 + n6 + nE;
    for (int r = threadIdx.x; r < world; r += 64) tail[r] = (r == rank) ? m : 0.0;
    if (threadIdx.x == 0) { msg[0] = uy_src[0]; msg[1] = 0.0; }
  }
}

// The camera half of a linearisation in a multi-rank job: msg = [ 8 header words | sum_k partL[k] (n values) ], one
// all-reduce.  The header carries the step's six local sums (k_scalars' block, scal6 != null) when the pass was speculated
// at a trial point -- the trial cost comes out of the same pass, so verdict and linearisation share one collective.
__global__ void __launch_bounds__(256)
k_fold_lin(const double* __restrict__ scal6, const double* __restrict__ partL, size_t n, int nparts, double* __restrict__ msg) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    double v[NPART];
#pragma unroll
    for (int k = 0; k < NPART; ++k) v[k] = (k < nparts) ? partL[(size_t)k * n + i] : 0.0;
    double s = v[0];
#pragma unroll
    for (int k = 1; k < NPART; ++k) s += v[k];
    msg[8 + i] = s;
  }
  if (blockIdx.x == 0 && threadIdx.x < 8) msg[threadIdx.x] = (scal6 && threadIdx.x < 6) ? scal6[threadIdx.x] : 0.0;
}

// The pixel streams (c_uv / p_uv) of the multi-kernel path.  The reference's measurements are cv2 keypoints (kp.pt,
// /root/reference/src/bundle_adjuster.py:216): float32 values handed over as doubles.  When EVERY pixel of a problem is such
// a value (ba_set_problem checks all of them) the two streams are stored as float2 -- half the bytes of the linearisation
// passes' largest input -- and widened on load: exactly the doubles the caller gave, so every result stays bit-identical.
// Loads of the observation streams (index, pixel and weight arrays: every element is read once per pass, in order).
template <class T> __device__ __forceinline__ T ld_stream(const T* p) { return *p; }
// "this double is a float32 value" (finite; out-of-range values are clamped first: a double -> float conversion outside
// float's range is undefined in C++; NaN, infinities and anything beyond FLT_MAX keep the problem on double2)
__host__ __device__ inline bool pixel_is_f32(double u) {
  const double c = fmin(fmax(u, -3.4028234663852886e38), 3.4028234663852886e38);
  return (double)(float)c == u;
}
struct UvArr {
  const void* p;
  int f32;
  __device__ __forceinline__ double2 operator[](size_t i) const {
    if (f32) { const float2 v = ld_stream((const float2*)p + i); return make_double2((double)v.x, (double)v.y); }
    return ld_stream((const double2*)p + i);
  }
};
// out[j] = uv[idx[j]]: the caller-order pixels into point order / camera order (ba_set_problem); f32: stored as float2
__global__ void k_gather_uv(const double2* __restrict__ uv, const int* __restrict__ idx, int n, double2* __restrict__ out, int f32) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const double2 v = uv[idx[j]];
  if (f32) ((float2*)out)[j] = make_float2((float)v.x, (float)v.y);
  else out[j] = v;
}

// the flagged copies of the two index streams start as the plain streams (a robust linearisation stores an entry only
// where its flag changes)
__global__ void k_init_flagged(const int* __restrict__ c_pt, const int* __restrict__ p_cam, int n, int* __restrict__ c_ptf0,
                               int* __restrict__ c_ptf1, int* __restrict__ p_camf0, int* __restrict__ p_camf1) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int a = c_pt[j], b = p_cam[j];
  c_ptf0[j] = a; c_ptf1[j] = a; p_camf0[j] = b; p_camf1[j] = b;
}

// pts (Np,3) -> X slots of the point table; table (Np,8) -> pts
// `slot[p]` = internal (locality-sorted) index of the caller's point p
__global__ void k_pack_points(const double* __restrict__ pts, const int* __restrict__ slot, int n_pts,
                              double* __restrict__ ptab) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pts) return;
  double* o = ptab + PT * (size_t)slot[p];
  o[0] = pts[3 * (size_t)p]; o[1] = pts[3 * (size_t)p + 1]; o[2] = pts[3 * (size_t)p + 2];
  o[3] = 0; o[4] = 0; o[5] = 0; o[6] = 0; o[7] = 0;
}
// flags in the caller's point order -> point slots (ba_set_held)
__global__ void k_scatter_flags(const unsigned char* __restrict__ in, const int* __restrict__ slot, int n, unsigned char* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[slot[i]] = in[i];
}
__global__ void k_unpack_points(const double* __restrict__ ptab, const int* __restrict__ slot, int n_pts,
                                double* __restrict__ pts) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pts) return;
  const double* s = ptab + PT * (size_t)slot[p];
  pts[3 * (size_t)p] = s[0]; pts[3 * (size_t)p + 1] = s[1]; pts[3 * (size_t)p + 2] = s[2];
}
// dst[p][0..W) = src[slot[p]][0..W)   (per-point outputs back in the caller's point order)
__global__ void k_unpermute_rows(const double* __restrict__ src, const int* __restrict__ slot, int n_pts, int width,
                                 double* __restrict__ dst) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pts) return;
  for (int q = 0; q < width; ++q) dst[(size_t)p * width + q] = src[(size_t)slot[p] * width + q];
}

// -------------------------------------------------------------------------------------
// camera passes: wave = (camera c, partition k)
// -------------------------------------------------------------------------------------
struct Seg { int c, k, beg, end, lane; };
// Workgroup -> (camera group, partition).  Workgroups are dealt round-robin over the NPART XCDs.
// band = 0: XCD x takes partition x of every camera -- right when a camera's k-th chunk lies in the
// k-th eighth of the point table (observations spread over all points: C3).  band = 1: XCD x takes
// all partitions of the x-th eighth of the cameras -- right when a camera's points sit in a band
// around the camera's own position in the point numbering (sequential captures: C5).  Either way
// an XCD keeps gathering from the same slice of the point table, the one its point-pass ranges
// write; ba_set_problem counts which fits the data.  Speed only.
__device__ inline void group_of_block(int n_groups, int band, int& group, int& k) {
  if (band) {
    const int q = (int)(blockIdx.x % NPART) * n_groups + (int)(blockIdx.x / NPART);
    group = q / NPART; k = q % NPART;
  } else {
    group = blockIdx.x / NPART; k = blockIdx.x % NPART;
  }
}
__device__ inline bool cam_segment(const int* __restrict__ offk, int n_cams, int band, Seg& s) {
  int group;
  group_of_block((n_cams + WPB - 1) / WPB, band, group, s.k);
  s.c = __builtin_amdgcn_readfirstlane(group * WPB + (int)(threadIdx.x >> 6));
  s.lane = threadIdx.x & 63;
  if (s.c >= n_cams) return false;
  s.beg = offk[s.c * (NPART + 1) + s.k];
  s.end = offk[s.c * (NPART + 1) + s.k + 1];
  return true;
}
template <int N>
__device__ inline void wave_store_sums(double (&acc)[N], int lane, double* __restrict__ dst) {
#pragma unroll
  for (int q = 0; q < N; ++q) acc[q] = wave_scan_sum_dpp(acc[q]);
  if (lane == 63) {
#pragma unroll
    for (int q = 0; q < N; ++q) dst[q] = acc[q];
  }
}

// K1: residuals / cost.  partR[(k*Nc + c)*2 + {0,1}] = sum r^2, sum rho-term.
template <bool ROBUST>
__global__ void __launch_bounds__(64 * WPB)
k_cam_residual(const double* __restrict__ cs, const double* __restrict__ ptab, const int* __restrict__ offk,
               const int* __restrict__ c_pt, const UvArr c_uv, const int* __restrict__ c_orig,
               double fx, double fy, double cx, double cy, double hub_c, int loss, int n_cams, int band,
               double* __restrict__ r_out, double* __restrict__ partR) {
  Seg s;
  if (!cam_segment(offk, n_cams, band, s)) return;
  const double* cam = cs + CS * s.c;
  double acc[2] = {0.0, 0.0};
  for (int i = s.beg + s.lane; i < s.end; i += 64) {
    const int p = ld_stream(c_pt + i);
    const double2 uv = c_uv[i];
    const double4 X = *(const double4*)(ptab + PT * (size_t)p);
    double xh, yh;
    obs_project(cam, X.x, X.y, X.z, xh, yh);
    const double ru = uv.x - (xh * fx + cx);
    const double rv = uv.y - (yh * fy + cy);
    acc[0] += ru * ru + rv * rv;
    if (ROBUST) {
      double t0, t1, w;
      robust_loss<true>(loss, ru, hub_c, t0, w);
      robust_loss<true>(loss, rv, hub_c, t1, w);
      acc[1] += t0 + t1;
    }
    if (r_out) {
      const int o = c_orig[i];
      r_out[2 * (size_t)o] = ru;
      r_out[2 * (size_t)o + 1] = rv;
    }
  }
  if (!ROBUST) acc[1] = acc[0];
  wave_store_sums<2>(acc, s.lane, partR + ((size_t)s.k * n_cams + s.c) * 2);
}

// K1 for the BAL 9-parameter camera (row f2; bal.py): intr[c] = (f, k1, k2), the camera looks down -z,
// p = -P[:2] / P.z, projection f (1 + k1 |p|^2 + k2 |p|^4) p, origin at the image centre.  Same mapping, partial sums
// and row order as k_cam_residual.
template <bool ROBUST>
__global__ void __launch_bounds__(64 * WPB)
k_cam_residual_bal(const double* __restrict__ cs, const double* __restrict__ intr, const double* __restrict__ ptab,
                   const int* __restrict__ offk, const int* __restrict__ c_pt, const UvArr c_uv,
                   const int* __restrict__ c_orig, double hub_c, int loss, int n_cams, int band,
                   double* __restrict__ r_out, double* __restrict__ partR) {
  Seg s;
  if (!cam_segment(offk, n_cams, band, s)) return;
  const double* cam = cs + CS * s.c;
  const double f = intr[3 * s.c], k1 = intr[3 * s.c + 1], k2 = intr[3 * s.c + 2];
  double acc[2] = {0.0, 0.0};
  for (int i = s.beg + s.lane; i < s.end; i += 64) {
    const int p = ld_stream(c_pt + i);
    const double2 uv = c_uv[i];
    const double4 X = *(const double4*)(ptab + PT * (size_t)p);
    double xh, yh;
    obs_project(cam, X.x, X.y, X.z, xh, yh);             // P.x / P.z, P.y / P.z  (z == 0 guarded as in cv2)
    const double px = -xh, py = -yh;
    const double n2 = px * px + py * py;
    const double rad = f * (1.0 + n2 * (k1 + k2 * n2));
    const double ru = uv.x - rad * px;
    const double rv = uv.y - rad * py;
    acc[0] += ru * ru + rv * rv;
    if (ROBUST) {
      double t0, t1, w;
      robust_loss<true>(loss, ru, hub_c, t0, w);
      robust_loss<true>(loss, rv, hub_c, t1, w);
      acc[1] += t0 + t1;
    }
    if (r_out) {
      const int o = c_orig[i];
      r_out[2 * (size_t)o] = ru;
      r_out[2 * (size_t)o + 1] = rv;
    }
  }
  if (!ROBUST) acc[1] = acc[0];
  wave_store_sums<2>(acc, s.lane, partR + ((size_t)s.k * n_cams + s.c) * 2);
}

// rows of the pre-M camera Jacobian: J0 = [P0 x X | -d00 0 -d02], J1 = [P1 x X | 0 -d11 -d12]
__device__ inline void cam_jac_rows(const Geom& g, double X0, double X1, double X2, double (&J0)[6], double (&J1)[6]) {
  J0[0] = g.P[1] * X2 - g.P[2] * X1; J0[1] = g.P[2] * X0 - g.P[0] * X2; J0[2] = g.P[0] * X1 - g.P[1] * X0;
  J1[0] = g.P[4] * X2 - g.P[5] * X1; J1[1] = g.P[5] * X0 - g.P[3] * X2; J1[2] = g.P[3] * X1 - g.P[4] * X0;
  J0[3] = -g.d00; J0[4] = 0.0;    J0[5] = -g.d02;
  J1[3] = 0.0;    J1[4] = -g.d11; J1[5] = -g.d12;
}

// symmetric congruence H = T^T A T, T = diag(M, I(NB-3)), A given as full NB x NB
template <int NB>
__device__ inline void m_congruence(const double* __restrict__ M, double (&A)[NB][NB]) {
  double B[NB][NB];
  for (int i = 0; i < NB; ++i) {
    for (int j = 0; j < 3; ++j) B[i][j] = A[i][0] * M[j] + A[i][1] * M[3 + j] + A[i][2] * M[6 + j];
    for (int j = 3; j < NB; ++j) B[i][j] = A[i][j];
  }
  for (int j = 0; j < NB; ++j) {
    const double h0 = M[0] * B[0][j] + M[3] * B[1][j] + M[6] * B[2][j];
    const double h1 = M[1] * B[0][j] + M[4] * B[1][j] + M[7] * B[2][j];
    const double h2 = M[2] * B[0][j] + M[5] * B[1][j] + M[8] * B[2][j];
    A[0][j] = h0; A[1][j] = h1; A[2][j] = h2;
    for (int i = 3; i < NB; ++i) A[i][j] = B[i][j];
  }
}

// Held parameters (ba_set_held): per camera a bit set over its NB block columns (the caller's coordinates, after M), per
// point one flag.  A held camera parameter has zero rows and columns in Hcc | bc, identity ones in every damped block, and
// zero entries in every PCG vector and step; a held point has Hpp = bp = 0 and Hpp^-1 := 0, so that it neither moves nor
// couples into S.  The observation loops are untouched: they only ever see camera vectors whose held entries are 0.
// cam_held == null: nothing held beyond fixed_cam.
__device__ inline unsigned cam_held_bits(const unsigned short* __restrict__ cam_held, int c) { return cam_held ? cam_held[c] : 0u; }
template <int NB>
__device__ inline void held_identity(unsigned held, double* __restrict__ H) {   // held rows / columns of an NB block -> identity
  for (int i = 0; i < NB; ++i)
    for (int j = i; j < NB; ++j)
      if (((held >> i) | (held >> j)) & 1u) H[UT(NB, i, j)] = (i == j) ? 1.0 : 0.0;
}

// Gaussian priors (ba_set_priors): 0.5 (x - mu)^T L (x - mu) per camera block and per point, x the caller's additive
// coordinates.  Camera side: info[c] = packed upper triangle of L_c (nb (nb + 1) / 2 entries, Hcc's order), mean[c] (nb), nb = 6
// (pose only) or 9; cams / intr = the raw parameters of the linearisation point.  info == null: no camera priors.
struct CamPriors { const double* info; const double* mean; const double* cams; const double* intr; int nb; };
// H += L_c, b += L_c (x_c - mu_c) for camera c, in the caller's coordinates (behind the M congruence)
template <int NB>
__device__ inline void cam_prior_add(const CamPriors& pr, int c, double* __restrict__ H, double* __restrict__ b) {
  const int nb = pr.nb < NB ? pr.nb : NB;
  const double* __restrict__ L = pr.info + (size_t)(pr.nb * (pr.nb + 1) / 2) * c;
  const double* __restrict__ mu = pr.mean + (size_t)pr.nb * c;
  double d[NB];
  for (int q = 0; q < nb; ++q) d[q] = (q < 6 ? pr.cams[6 * (size_t)c + q] : pr.intr[3 * (size_t)c + (q - 6)]) - mu[q];
  for (int i = 0; i < nb; ++i)
    for (int j = i; j < nb; ++j) {
      const double l = L[UT(pr.nb, i, j)];
      H[UT(NB, i, j)] += l;
      b[i] += l * d[j];
      if (j > i) b[j] += l * d[i];
    }
}

// Combine the NPART partial sums of k_camrow_linearize (fixed order), apply M:
//   Hcc[c] (NH) = Jc^T w Jc,  bc[c] (NB) = Jc^T w r  (zero for the fixed camera; zero rows / columns for held parameters).
// a[NH + NB] = the camera's pre-M sums (NH of Jc^T w Jc, upper triangle; NB of Jc^T w r), M from its state
template <int NB>
// pr (nullable) / c: the camera's prior is added behind M and ahead of the held zeroing
__device__ inline void lin_finalize_sums(const double* __restrict__ a, const double* __restrict__ M, bool fixed,
                                         double* __restrict__ H, double* __restrict__ b, unsigned held = 0u,
                                         const CamPriors* pr = nullptr, int c = 0) {
  constexpr int NH = NB * (NB + 1) / 2;
  if (fixed) {
    for (int q = 0; q < NH; ++q) H[q] = 0.0;
    for (int q = 0; q < NB; ++q) b[q] = 0.0;
    return;
  }
  double A[NB][NB];
  for (int i = 0; i < NB; ++i) for (int j = 0; j < NB; ++j) A[i][j] = a[ST(NB, i, j)];
  m_congruence<NB>(M, A);
  for (int i = 0; i < NB; ++i) for (int j = i; j < NB; ++j) H[UT(NB, i, j)] = A[i][j];
  b[0] = M[0] * a[NH] + M[3] * a[NH + 1] + M[6] * a[NH + 2];
  b[1] = M[1] * a[NH] + M[4] * a[NH + 1] + M[7] * a[NH + 2];
  b[2] = M[2] * a[NH] + M[5] * a[NH + 1] + M[8] * a[NH + 2];
  for (int q = 3; q < NB; ++q) b[q] = a[NH + q];
  if (pr && pr->info) cam_prior_add<NB>(*pr, c, H, b);
  if (held) {
    for (int i = 0; i < NB; ++i) {
      if ((held >> i) & 1u) b[i] = 0.0;
      for (int j = i; j < NB; ++j)
        if (((held >> i) | (held >> j)) & 1u) H[UT(NB, i, j)] = 0.0;
    }
  }
}
template <int NB>
__device__ inline void lin_finalize_camera(const double* __restrict__ partL, int nparts, const double* __restrict__ cam, int n_cams,
                                           int c, int fixed_cam, double* __restrict__ H, double* __restrict__ b, unsigned held,
                                           const CamPriors& pr) {
  constexpr int NL = NB * (NB + 1) / 2 + NB;
  double a[NL];
  for (int q = 0; q < NL; ++q) a[q] = 0.0;
  if (c != fixed_cam) {
    for (int k = 0; k < nparts; ++k) {
      const double* src = partL + ((size_t)k * n_cams + c) * NL;
      for (int q = 0; q < NL; ++q) a[q] += src[q];
    }
  }
  lin_finalize_sums<NB>(a, cam + 12, c == fixed_cam, H, b, held, &pr, c);
}
// stand-alone form (multi-rank jobs all-reduce Hcc|bc between this and k_pcg_setup; test hook)
template <int NB>
__global__ void __launch_bounds__(VEC_BLOCK)
k_lin_finalize(const double* __restrict__ partL, int nparts, const double* __restrict__ cs, int n_cams, int fixed_cam,
               double* __restrict__ Hcc, double* __restrict__ bc, const unsigned short* __restrict__ cam_held, CamPriors pr) {
  const int c = vec_camera(n_cams);
  if (c >= n_cams) return;
  lin_finalize_camera<NB>(partL, nparts, cs + CS * c, n_cams, c, fixed_cam, Hcc + (NB * (NB + 1) / 2) * (size_t)c, bc + NB * (size_t)c,
                          cam_held_bits(cam_held, c), pr);
}

// K4b: camera pass of the Schur product, pre-M:  part6[(k*Nc + c)*6 + ..] = sum Jc^T w (Jp y_p)
// with y read from the point table.  PCG = true: iteration kit of the solve (early exit once
// converged; an extra workgroup folds the point pass's u.y partials).  The right-hand side
// pass that also builds the Schur-Jacobi blocks is k_camrow_schur_diag.
// Host-visible progress word (host-mapped, coherent memory): payload first, then the
// sequence number with a system-scope release; the host spins on the sequence number.
__device__ inline void publish_flag(long long* __restrict__ host_flag, long long seq, long long payload) {
  if (!host_flag) return;
  __hip_atomic_store(host_flag + 1, payload, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(host_flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Called by whole waves (all 64 lanes live): the nblkV partial pairs are summed lane-strided, then
// across the wave -- a fixed order, the same in every wave of every kernel.
__device__ inline bool pcg_finished(int k, const PcgState* __restrict__ st, const double* __restrict__ partV,
                                    int nblkV, double tol2, int min_iters, double& gamma, double& zeta) {
  const PcgState& s = st[k & 1];
  const double2* pv = (const double2*)(partV + (size_t)(k & 1) * 2 * nblkV);
  double g = 0, z = 0;
  for (int b = threadIdx.x & 63; b < nblkV; b += 64) { const double2 t = pv[b]; g += t.x; z += t.y; }
  g = wave_total_dpp(g);
  z = wave_total_dpp(z);
  gamma = g; zeta = z;
  if (s.done || s.stop_model) return true;
  const double g0 = (k == 0) ? g : s.gamma0;
  if (!(g > 0.0)) return true;
  return (k >= min_iters && g <= tol2 * g0);
}

// PCG verdict word of iteration k (vd = verdict + 4 * (k & 1)): {gamma, zeta, finished}.  Written once per
// iteration by workgroup 0 of the point pass (the probe, first kernel of the iteration, which sums the vector
// kernel's partials); the camera pass and the vector kernel of the same iteration read these three words
// instead of re-reducing the partials in every wave (~9 % of the camera pass's vector instructions).
__device__ inline bool pcg_verdict(const double* __restrict__ verdict, int k, double& gamma, double& zeta) {
  const double* vd = verdict + 4 * (k & 1);
  gamma = vd[0]; zeta = vd[1];
  return vd[2] != 0.0;
}

// SEGL lanes per (camera, partition) segment: 64 (a wave) or 16 (one DPP row).  Fewer lanes per segment =
// fewer waves, so the per-wave prologue and the cross-lane reduction of the six sums are paid for 4
// segments at once (the pass is vector-issue bound: SQ counters, profiles/), at the price of a longer chain
// of dependent gathers per lane.  Workgroup = 256 / SEGL consecutive cameras of one partition.
template <int SEGL>
__device__ inline double seg_sum_dpp(double x) {    // the last lane of every SEGL-lane segment ends with the segment total
  x += dpp_f64<DPP_ROW_SHR1, 0xf>(x);
  x += dpp_f64<DPP_ROW_SHR2, 0xf>(x);
  x += dpp_f64<DPP_ROW_SHR4, 0xf>(x);
  x += dpp_f64<DPP_ROW_SHR8, 0xf>(x);
  if (SEGL == 64) {
    x += dpp_f64<DPP_ROW_BCAST15, 0xa>(x);
    x += dpp_f64<DPP_ROW_BCAST31, 0xc>(x);
  }
  return x;
}
template <class CM, bool ROBUST, bool PCG, typename JT, int SEGL>
__global__ void __launch_bounds__(64 * WPB)
k_cam_schur(const double* __restrict__ cs, const double* __restrict__ intr, const double* __restrict__ ptab,
            const int* __restrict__ offk, const int* __restrict__ c_pt, const double2* __restrict__ c_w,
            double fx, double fy, int n_cams, int band, int fixed_cam, double* __restrict__ part6,
            int kit, const double* __restrict__ verdict, const double* __restrict__ partA, int nblkA,
            double* __restrict__ uy) {
  constexpr int NB = CM::NB;
  static_assert(SEGL == 16 || SEGL == 64, "16 or 64 lanes per segment");
  constexpr int CPB = 64 * WPB / SEGL;         // cameras per workgroup
  // segment bounds and camera state are fetched before the PCG verdict is known: one round trip
  // less on the way to the first gather (an early-exit launch wastes a few loads)
  const bool extra = PCG && blockIdx.x == gridDim.x - 1;   // extra workgroup: folds the point pass's u.y partials
  if (PCG) { BA_STAMP(1, 0); BA_STAMP(1, 1); }
  int group, k;
  group_of_block((n_cams + CPB - 1) / CPB, band, group, k);
  int c = group * CPB + (int)(threadIdx.x / SEGL);
  if (SEGL == 64) c = __builtin_amdgcn_readfirstlane(c);       // wave-uniform: camera state in scalar registers
  const int lane = threadIdx.x % SEGL;
  const bool live = !extra && c < n_cams;
  int beg = 0, end = 0;
  JT cam[CM::CAM];                             // Jacobian blocks in JT (double, or float for config 5)
#pragma unroll
  for (int q = 0; q < CM::CAM; ++q) cam[q] = (JT)0;
  if (live) {
    beg = offk[c * (NPART + 1) + k];
    end = offk[c * (NPART + 1) + k + 1];
    CM::template load_cam<JT>(cs, intr, c, cam);
  }
  if (PCG) {
    double g, z;
    if (pcg_verdict(verdict, kit, g, z)) return;
    if (extra) {
      __shared__ double smu[WPB];
      double a = 0.0;
      for (int b = threadIdx.x; b < nblkA; b += 64 * WPB) a += partA[b];
      a = wave_total_dpp(a);
      if ((threadIdx.x & 63) == 0) smu[threadIdx.x >> 6] = a;
      __syncthreads();
      if (threadIdx.x == 0) { double t = 0; for (int w = 0; w < WPB; ++w) t += smu[w]; uy[0] = t; }
      return;
    }
  }
  if (SEGL == 64 && !live) return;             // (narrower segments: dead lanes idle through the reduction)
  if (PCG) BA_STAMP(1, 2);
  const JT fxj = (JT)fx, fyj = (JT)fy;
  double acc[NB];                              // sums always in fp64
#pragma unroll
  for (int q = 0; q < NB; ++q) acc[q] = 0.0;
  if (live && c != fixed_cam) {
    int i = beg + lane;
    int pf = (i < end) ? ld_stream(c_pt + i) : 0;          // ROBUST: the flagged copy of c_pt
    double2 w = make_double2(1.0, 1.0);
    if (ROBUST && pf < 0) w = ld_stream(c_w + i);
    while (i < end) {
      const int in = i + SEGL;
      const int pn = (in < end) ? ld_stream(c_pt + in) : 0;          // prefetch the next index
      int p = ROBUST ? (pf & IDX_MASK) : pf;
#ifdef BA_STAMPS
      const int dbg = g_dbg_mode;
      if (dbg == 1) p = i % 100000;                          // no gather: consecutive records (coalesced)
      if (dbg == 3) p = (p & ~7) | (lane & 7);               // gather whole 512-byte groups: 8 lanes share 4 lines
#endif
      double4 Xd = *(const double4*)(ptab + PT * (size_t)p);
      double4 Yd = *(const double4*)(ptab + PT * (size_t)p + 4);
#ifdef BA_STAMPS
      if (dbg == 2) Yd = Xd;                                 // one 32-byte half of the record only
#endif
      double2 wn = make_double2(1.0, 1.0);                 // next weight, only where it is not (1, 1)
      if (ROBUST && pn < 0) wn = ld_stream(c_w + in);
      const JT X0 = (JT)Xd.x, X1 = (JT)Xd.y, X2 = (JT)Xd.z, Y0 = (JT)Yd.x, Y1 = (JT)Yd.y, Y2 = (JT)Yd.z;
      typename CM::template Obs<JT> g;
      CM::template geom<true, JT, JT>(cam, X0, X1, X2, fxj, fyj, g);
      const JT* Pm = CM::pm(g);
      const JT s0 = -(Pm[0] * Y0 + Pm[1] * Y1 + Pm[2] * Y2) * (JT)w.x;       // w (Jp y), Jp = -Pm
      const JT s1 = -(Pm[3] * Y0 + Pm[4] * Y1 + Pm[5] * Y2) * (JT)w.y;
      CM::jct_accumulate(g, X0, X1, X2, s0, s1, acc);
      i = in; pf = pn; w = wn;
    }
  }
  if (PCG) BA_STAMP(1, 3);
#pragma unroll
  for (int q = 0; q < NB; ++q) acc[q] = seg_sum_dpp<SEGL>(acc[q]);
  if (live && lane == SEGL - 1) {
    double* dst = part6 + ((size_t)k * n_cams + c) * NB;
#pragma unroll
    for (int q = 0; q < NB; ++q) dst[q] = acc[q];
  }
  if (PCG) { BA_STAMP(1, 6); BA_STAMP(1, 7); }
}

// ---- 27-sum camera passes, one 16-lane DPP row per (camera, partition) segment ------------
// With 27 running sums the 64-lane reduction of the wave-per-segment mapping costs as much as
// the arithmetic of a ~125-observation segment; a row walks the segment in 8 steps and only
// needs the 4 in-row shifts.  Workgroup = 16 consecutive cameras of one partition.
constexpr int ROW_LANES = 16;                   // lanes per (camera, partition) segment: one DPP row
constexpr int ROWS = 256 / ROW_LANES;           // segments (= cameras) per 256-thread workgroup
struct RowSeg { int c, k, beg, end, l16; bool live; };   // l16: lane inside the segment
__device__ inline void row_segment(const int* __restrict__ offk, int n_cams, int band, RowSeg& s) {
  int group;
  group_of_block((n_cams + ROWS - 1) / ROWS, band, group, s.k);
  s.c = group * ROWS + (int)(threadIdx.x / ROW_LANES);
  s.l16 = threadIdx.x % ROW_LANES;
  s.live = s.c < n_cams;
  s.beg = s.live ? offk[s.c * (NPART + 1) + s.k] : 0;
  s.end = s.live ? offk[s.c * (NPART + 1) + s.k + 1] : 0;
}
__device__ inline double row_sum_dpp(double x) {     // the last lane of every segment ends with the segment total
  x += dpp_f64<DPP_ROW_SHR1, 0xf>(x);
  x += dpp_f64<DPP_ROW_SHR2, 0xf>(x);
  x += dpp_f64<DPP_ROW_SHR4, 0xf>(x);
  x += dpp_f64<DPP_ROW_SHR8, 0xf>(x);
  return x;
}

// K2a: camera half of the normal equations, pre-M: partL[(k*Nc + c)*27 ..] = 21 sums of Jc^T w Jc (upper triangle), 6 of Jc^T w r;
// IRLS weights and flagged indices of camera-ordered observations when ROBUST
// COST: also the cost partials of K1 (partR[(k*Nc + c)*2 + {0,1}] = sum r^2, sum rho-term), so that the pass at a
// TRIAL point is the trial-cost evaluation and the camera half of the next linearisation in one (ba_solve).
template <class CM, bool ROBUST, bool COST>
__global__ void __launch_bounds__(ROW_LANES * ROWS)
k_camrow_linearize(const double* __restrict__ cs, const double* __restrict__ intr, const double* __restrict__ ptab,
                   const int* __restrict__ offk, const int* __restrict__ c_pt, const UvArr c_uv,
                   double fx, double fy, double cx, double cy, double hub_c, int loss, int n_cams, int band,
                   double2* __restrict__ c_w, int* __restrict__ c_ptf, double* __restrict__ partL,
                   double* __restrict__ partR) {
  constexpr int NB = CM::NB, NH = CM::NH, NL = CM::NL;
  RowSeg s;
  row_segment(offk, n_cams, band, s);
  constexpr int NACC = COST ? NL + 2 : NL;
  double acc[NACC];
#pragma unroll
  for (int q = 0; q < NACC; ++q) acc[q] = 0.0;
  if (s.live) {
    double cam[CM::CAM];
    CM::load_cam_vec(cs, intr, s.c, cam);
    // ROBUST: the index stream is read from the flagged copy this pass maintains (c_ptf holds c_pt | flag from an earlier
    // linearisation, or plain c_pt): an entry is stored only when its flag CHANGES -- near the solution almost none does,
    // and the 4-byte-per-observation store stream disappears from the pass's traffic
    const int* __restrict__ idx_in = ROBUST ? (const int*)c_ptf : c_pt;
    int i = s.beg + s.l16;
    int pr = (i < s.end) ? ld_stream(idx_in + i) : 0;
    double2 uv = (i < s.end) ? c_uv[i] : make_double2(0, 0);
    while (i < s.end) {
      const int in = i + ROW_LANES;
      const int pn = (in < s.end) ? ld_stream(idx_in + in) : 0;
      const double2 uvn = (in < s.end) ? c_uv[in] : make_double2(0, 0);
      const int p = ROBUST ? (pr & IDX_MASK) : pr;
      const double4 X = *(const double4*)(ptab + PT * (size_t)p);
      typename CM::template Obs<double> g;
      CM::template geom<false, double, double>(cam, X.x, X.y, X.z, fx, fy, g);
      double ru, rv;
      CM::residual(g, uv.x, uv.y, fx, fy, cx, cy, ru, rv);
      double w0 = 1.0, w1 = 1.0;
      if (COST) acc[NL] += ru * ru + rv * rv;
      if (ROBUST) {
        double t0, t1;
        robust_loss<COST>(loss, ru, hub_c, t0, w0);
        robust_loss<COST>(loss, rv, hub_c, t1, w1);
        if (COST) acc[NL + 1] += t0 + t1;
        const int pfl = flagged_index(p, w0, w1);
        if (pfl != pr) c_ptf[i] = pfl;
        if (pfl < 0) c_w[i] = make_double2(w0, w1);        // unflagged weights are never read
      }
      double J0[NB], J1[NB];
      CM::jac_rows(g, X.x, X.y, X.z, J0, J1);
#pragma unroll
      for (int a = 0; a < NB; ++a) {
        const double wa0 = w0 * J0[a], wa1 = w1 * J1[a];
#pragma unroll
        for (int b = a; b < NB; ++b) acc[UT(NB, a, b)] += wa0 * J0[b] + wa1 * J1[b];
        acc[NH + a] += wa0 * ru + wa1 * rv;
      }
      i = in; pr = pn; uv = uvn;
    }
  }
  if (COST && !ROBUST) acc[NL + 1] = acc[NL];
#pragma unroll
  for (int q = 0; q < NACC; ++q) acc[q] = row_sum_dpp(acc[q]);
  if (s.live && s.l16 == ROW_LANES - 1) {
    double* o = partL + ((size_t)s.k * n_cams + s.c) * NL;
#pragma unroll
    for (int q = 0; q < NL; ++q) o[q] = acc[q];
    if (COST) {
      double* r2 = partR + ((size_t)s.k * n_cams + s.c) * 2;
      r2[0] = acc[NL]; r2[1] = acc[NL + 1];
    }
  }
}

// right-hand side + Schur-Jacobi blocks (row form of k_cam_schur<.., DIAG = true, PCG = false>)
template <class CM, bool ROBUST>
__global__ void __launch_bounds__(ROW_LANES * ROWS)
k_camrow_schur_diag(const double* __restrict__ cs, const double* __restrict__ intr, const double* __restrict__ ptab,
                    const int* __restrict__ offk, const int* __restrict__ c_pt, const double2* __restrict__ c_w,
                    const double* __restrict__ Hppinv, double fx, double fy, int n_cams, int band, int fixed_cam,
                    double* __restrict__ part6, double* __restrict__ partE) {
  constexpr int NB = CM::NB, NH = CM::NH, NL = CM::NL;
  RowSeg s;
  row_segment(offk, n_cams, band, s);
  double acc[NL];
#pragma unroll
  for (int q = 0; q < NL; ++q) acc[q] = 0.0;
  if (s.live && s.c != fixed_cam) {
    double cam[CM::CAM];
    CM::load_cam_vec(cs, intr, s.c, cam);
    int i = s.beg + s.l16;
    int pf = (i < s.end) ? ld_stream(c_pt + i) : 0;          // ROBUST: the flagged copy of c_pt
    double2 w = make_double2(1.0, 1.0);
    if (ROBUST && pf < 0) w = ld_stream(c_w + i);
    while (i < s.end) {
      const int in = i + ROW_LANES;
      const int pn = (in < s.end) ? ld_stream(c_pt + in) : 0;
      const int p = ROBUST ? (pf & IDX_MASK) : pf;
      const double4 X = *(const double4*)(ptab + PT * (size_t)p);
      const double4 Y = *(const double4*)(ptab + PT * (size_t)p + 4);
      double2 wn = make_double2(1.0, 1.0);
      if (ROBUST && pn < 0) wn = ld_stream(c_w + in);
      typename CM::template Obs<double> g;
      CM::template geom<false, double, double>(cam, X.x, X.y, X.z, fx, fy, g);
      const double* Pm = CM::pm(g);
      const double s0 = -(Pm[0] * Y.x + Pm[1] * Y.y + Pm[2] * Y.z) * w.x;
      const double s1 = -(Pm[3] * Y.x + Pm[4] * Y.y + Pm[5] * Y.z) * w.y;
      {
        double a9[NB];
#pragma unroll
        for (int q = 0; q < NB; ++q) a9[q] = acc[q];
        CM::jct_accumulate(g, X.x, X.y, X.z, s0, s1, a9);
#pragma unroll
        for (int q = 0; q < NB; ++q) acc[q] = a9[q];
      }
      double hi[6];
      const double2* hp = (const double2*)(Hppinv + 6 * (size_t)p);
      const double2 h01 = hp[0], h23 = hp[1], h45 = hp[2];
      hi[0] = h01.x; hi[1] = h01.y; hi[2] = h23.x; hi[3] = h23.y; hi[4] = h45.x; hi[5] = h45.y;
      double t0[3], t1[3];
      sym3_mul(hi, Pm, t0);
      sym3_mul(hi, Pm + 3, t1);
      const double G00 = w.x * w.x * (Pm[0] * t0[0] + Pm[1] * t0[1] + Pm[2] * t0[2]);
      const double G01 = w.x * w.y * (Pm[0] * t1[0] + Pm[1] * t1[1] + Pm[2] * t1[2]);
      const double G11 = w.y * w.y * (Pm[3] * t1[0] + Pm[4] * t1[1] + Pm[5] * t1[2]);
      double J0[NB], J1[NB];
      CM::jac_rows(g, X.x, X.y, X.z, J0, J1);
#pragma unroll
      for (int a = 0; a < NB; ++a) {
        const double l0 = J0[a] * G00 + J1[a] * G01, l1 = J0[a] * G01 + J1[a] * G11;
#pragma unroll
        for (int b = a; b < NB; ++b) acc[NB + UT(NB, a, b)] += l0 * J0[b] + l1 * J1[b];
      }
      i = in; pf = pn; w = wn;
    }
  }
#pragma unroll
  for (int q = 0; q < NL; ++q) acc[q] = row_sum_dpp(acc[q]);
  if (s.live && s.l16 == ROW_LANES - 1) {
    double* o6 = part6 + ((size_t)s.k * n_cams + s.c) * NB;
#pragma unroll
    for (int q = 0; q < NB; ++q) o6[q] = acc[q];
    double* oe = partE + ((size_t)s.k * n_cams + s.c) * NH;
#pragma unroll
    for (int q = 0; q < NH; ++q) oe[q] = acc[NB + q];
  }
}

// -------------------------------------------------------------------------------------
// point passes: LPP lanes per point, camera table (camA) in LDS when it fits
// -------------------------------------------------------------------------------------
// Camera table of a point-pass workgroup: rows [lo, lo + n) of the packed table camA =
// R[9] t[3] | vtil[6] -- the window of cameras its points are observed from (host-computed per
// workgroup).  The window is staged in LDS when it fits (use_lds, workgroup-uniform), else rows
// are gathered from L2.  ROWLEN 12 reads R|t only.
constexpr int LDS_TAB_BYTES = 150 * 1024;
template <int ROWLEN, int STRIDE>
__device__ inline void load_cam_row(bool use_lds, const double* __restrict__ tab, const double* __restrict__ camA,
                                    int lo, int c, double (&row)[ROWLEN]) {
  const double2* src = use_lds ? (const double2*)(tab + STRIDE * (c - lo)) : (const double2*)(camA + STRIDE * (size_t)c);
#pragma unroll
  for (int q = 0; q < ROWLEN / 2; ++q) { const double2 t = src[q]; row[2 * q] = t.x; row[2 * q + 1] = t.y; }
}
// The copy in two halves: fill_cam_table_issue starts it, fill_cam_table_wait ends it (wait + workgroup barrier); what a
// kernel does in between overlaps the copy's round trips.  SKIP_WAVE0: wave 0 has other work in between (the PCG probe)
// and takes no share of the copy -- its probe loads would otherwise queue behind its share.
template <int BLOCK, int STRIDE, bool SKIP_WAVE0 = false>
__device__ inline void fill_cam_table_issue(double* __restrict__ tab, const double* __restrict__ camA, int lo, int n) {
  static_assert(STRIDE % 2 == 0, "table rows are copied and read 16 bytes at a time");
  const double2* src = (const double2*)(camA + STRIDE * (size_t)lo);
  const int total = n * STRIDE / 2;
  // LDS-DMA (global_load_lds_dwordx4, gfx950): 16 bytes per lane straight into LDS at (wave-uniform base) + lane * 16,
  // no staging registers and no ds_write issue slots; a wave copies whole 1 KB pieces, the lanes past the end of the
  // table sit out (an inactive lane neither loads nor stores).  The copy is invisible to the compiler: the explicit
  // vmcnt(0) of fill_cam_table_wait keeps every later LDS read behind it.
  // Every workgroup copies the same table at the same time: each starts at a different piece, so that the
  // workgroups of an XCD are not all on the same L2 channel at any moment.
  constexpr int NW = BLOCK / 64 - (SKIP_WAVE0 ? 1 : 0);
  const int wave = (int)(threadIdx.x >> 6) - (SKIP_WAVE0 ? 1 : 0), lane = threadIdx.x & 63;
  if (SKIP_WAVE0 && wave < 0) return;
  const int npieces = (total + 63) / 64;
  const int rot = (int)((blockIdx.x * 37u) % (unsigned)npieces);
  for (int q = wave; q < npieces; q += NW) {
    int piece = q + rot;
    if (piece >= npieces) piece -= npieces;
    const int i = piece * 64 + lane;
    if (i < total)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + i),
                                       (__attribute__((address_space(3))) void*)(tab + piece * 128), 16, 0, 0);
  }
}
__device__ inline void fill_cam_table_wait() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}
template <int BLOCK, int STRIDE>
__device__ inline void fill_cam_table(double* __restrict__ tab, const double* __restrict__ camA, int lo, int n) {
  fill_cam_table_issue<BLOCK, STRIDE>(tab, camA, lo, n);
  fill_cam_table_wait();
}
// deterministic workgroup sum of N values held by every wave's lane 0 -> thread 0
template <int N, int BLOCK, int M>
__device__ inline void block_combine(double (&v)[M], double* __restrict__ sm) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < N; ++q) sm[wv * N + q] = v[q];
  }
  // Only the LDS words above cross this barrier.  __syncthreads() would also wait for every global store the wave has
  // in flight (the point records just written: a round trip to L2 nobody in this workgroup needs).
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < N; ++q) {
      double a = 0;
      for (int w = 0; w < BLOCK / 64; ++w) a += sm[w * N + q];
      v[q] = a;
    }
  }
}

// vt = (M v_r, v_t, ..): a camera vector in the form the point passes multiply with (ba_models.hpp)
template <int NB>
__device__ inline void write_vtil(const double* __restrict__ M, const double (&v)[NB], double* __restrict__ dst) {
  dst[0] = M[0] * v[0] + M[1] * v[1] + M[2] * v[2];
  dst[1] = M[3] * v[0] + M[4] * v[1] + M[5] * v[2];
  dst[2] = M[6] * v[0] + M[7] * v[1] + M[8] * v[2];
#pragma unroll
  for (int q = 3; q < NB; ++q) dst[q] = v[q];
}

// ---- riders: small one-workgroup-per-unit kernels that run as EXTRA workgroups of a point-pass launch -------------------
// A point pass occupies one workgroup per compute unit on part of the chip (C3: 196 of 256) and the O(Nc) / O(1) kernels
// between the passes are pure launch latency on a handful of waves.  Two of them have no dependence on the point pass
// they now share a launch with, only a one-way hand-over:
//   * the camera update (K7a) rides along the back substitution: the trial cameras are not needed before the NEXT kernel;
//     the one thing the back substitution needs from it -- the step in the point passes' form, vt = (M dc_r, dc_t, ..) --
//     is computed by every point workgroup for the rows of its own LDS window, right behind the table copy;
//   * the step's scalar fold + LM verdict (k_scalars) rides along the speculated point half of the next linearisation as
//     workgroup 0: the point workgroups need its result (the damping an accepted step continues with) only when they
//     invert their first Hpp, a whole observation loop later, and pick it up through one device-scope word.
// CamUpdateArgs / ScalarsArgs are the riders' arguments (n_blocks / on = 0: no rider in this launch).
struct CamUpdateArgs {
  double* lam_slot;              // cleared by every back-substitution launch: see ScalarsArgs::lam_slot
  const double *cams, *intr, *dc, *rpcg, *Hcc, *bc, *cs;
  const double* vx;              // (M x_r, x_t, ..) of the PCG iterate, NB per camera, kept current by k_pcg_setup / k_pcg_step
  double *cams_trial, *intr_trial, *cs_trial, *vtil, *camA_trial, *partC;
  int n_cams, fixed_cam, n_blocks;
  int groups;                    // camera groups (of CM::VC cameras, one wave each) per riding 1024-thread workgroup (CU_GROUPS; <= 16)
  int fuse;                      // a PCG point pass (MODE 0) that finds PCG finished goes on as the back substitution in the SAME launch
                                 // (n_blocks camera-update workgroups ride in front, as in a MODE 1 launch): see pt_schur_body
  const int* cam_gl;             // shared intrinsics (null = none): dc.r_pcg, |dc|^2 and |cams|^2 count a shared entry at its leader only
};
struct ScalarsArgs {
  const double* partR; int nR;
  const double* partB; int nB;
  const double* partC; int nC;
  int kit;
  const PcgState* st;
  const double* partV; int nblkV;
  double tol2; int min_iters;
  double *scal, *scal_host;
  long long* host_flag; long long seq;
  int decide; double cost_cur, lambda, lam_floor;
  double* lam_slot;              // rider mode: device word the point workgroups of the same launch wait on.  It holds 0 (cleared by
                                 // the back substitution of the same step, two kernels earlier) until the rider stores the next
                                 // damping (> 0) into it: ONE word carries "ready" and the value, one relaxed load reads both
  long long* err_flag;           // host-mapped word a point workgroup sets when that wait runs out (RIDER_WAIT_TICKS)
  int on;
};
constexpr long long RIDER_WAIT_TICKS = 100000000;   // 1 s of the 100 MHz wall clock: only a rider that is never dispatched gets there
constexpr int CU_GROUPS = 4;          // camera groups (of CM::VC cameras, one wave each) per riding 1024-thread workgroup
template <class CM> __device__ void cam_update_body(const CamUpdateArgs& a, int blk, bool active, double* __restrict__ lds);
template <class CM> __device__ __forceinline__ void cam_update_rider(const CamUpdateArgs& a, int rb, double* __restrict__ dyn_lds);
template <class CM> __host__ __device__ constexpr int cam_update_lds_doubles() {
  return CM::VC * (6 + 3 * CM::NB + CM::NH + CS + 6 + CS);
}
__device__ void scalars_body(const ScalarsArgs& a);

// Work list of a point-pass launch.  Range mode (plist == nullptr): slot s is point s, points
// with more than skip_thr observations are left to the long-track launch.  List mode: slot s is
// point plist[s] (the long tracks, LANES = 16: one DPP row per point).
struct PtWork { const int* plist; int n_slots; int skip_thr; int blk_base; int slots_per_block; int xcd_ranges; };

// Range a point-pass workgroup works on.  Workgroups are dealt round-robin over the NPART XCDs
// (measured: XCC_ID = blockIdx % 8); with xcd_ranges the ranges of one XCD are consecutive, so XCD x
// reads and writes the x-th eighth of the point table -- the same slice its camera-pass partition x
// gathers from, which keeps y and X in that XCD's L2 between the two passes.  Speed only: the
// range -> partial-sum slot mapping does not change, so results are bit-identical either way.
__device__ inline int pt_range_of_block(int b, int n, int xcd_ranges) {
  if (!xcd_ranges) return b;
  const int x = b % NPART;
  int start = 0;
  for (int q = 0; q < x; ++q) start += (n - q + NPART - 1) / NPART;   // workgroups with blockIdx % NPART == q
  return start + b / NPART;
}

template <int LANES>
__device__ inline double lanes_sum(double x) {      // last lane of every LANES-group ends with the group sum
  x += dpp_f64<DPP_ROW_SHR1, 0xf>(x);
  if (LANES >= 4) x += dpp_f64<DPP_ROW_SHR2, 0xf>(x);
  if (LANES >= 8) x += dpp_f64<DPP_ROW_SHR4, 0xf>(x);
  if (LANES >= 16) x += dpp_f64<DPP_ROW_SHR8, 0xf>(x);
  return x;
}

// K2b: point half of the normal equations.  Hpp[p] (6) = sum P^T w P, bp[p] (3) = -sum P^T w r,
// IRLS weights of point-ordered observations (p_w) when ROBUST; K3 fused: damped inverse and y0.
// Body for workgroup `bid` of `nblk`: LANES lanes per point (LPP short tracks, LPP_LONG long ones).
template <class CM, bool ROBUST, bool ALL_LDS, int LANES>
__device__ __forceinline__ void
pt_linearize_body(const double* __restrict__ camA, double* __restrict__ ptab, const int* __restrict__ pt_off,
                  const int* __restrict__ p_cam, const UvArr p_uv, const int2* __restrict__ blk_win,
                  const PtWork& wk, int bid, int nblk, double fx, double fy, double cx, double cy, double hub_c, int loss,
                  double lambda_arg, const double* __restrict__ lam_dev, double* __restrict__ Hpp, double* __restrict__ bp,
                  double2* __restrict__ p_w, int* __restrict__ p_camf, double* __restrict__ Hppinv, double* __restrict__ y0,
                  double* __restrict__ partG, const double* __restrict__ lam_slot = nullptr, long long* __restrict__ err_flag = nullptr) {
  extern __shared__ __align__(16) double tab[];   // 16-byte aligned: the table is read and written with b128 LDS operations
  __shared__ double smg[PT_THREADS / 64];
  double gm = 0.0;                                 // max |bp| over this thread's points (the reference's gtol test, scipy trf.py:451-453)
  // lam_dev: the damping of a SPECULATED linearisation is decided on the device (k_scalars) -- by the kernel ahead of this
  // launch (lam_slot == null), or by workgroup 0 of this very launch (the rider, lam_slot = the word it stores the damping
  // in, 0 until then): then the damping is fetched as late as possible, before the first inverse
  double lambda = (lam_dev && !lam_slot) ? lam_dev[0] : lambda_arg;
  bool have_lambda = !(lam_dev && lam_slot);
  const int rb = pt_range_of_block(bid, nblk, wk.xcd_ranges);
  const int2 win = blk_win[wk.blk_base + rb];
  const bool use_lds = ALL_LDS || (size_t)win.y * CM::TA * sizeof(double) <= LDS_TAB_BYTES;   // ALL_LDS: every window fits
  if (use_lds) fill_cam_table<PT_THREADS, CM::TA>(tab, camA, win.x, win.y);
  const int sub = threadIdx.x % LANES;
  const int send = min(wk.n_slots, (rb + 1) * wk.slots_per_block);
  for (int sb = rb * wk.slots_per_block; sb < send; sb += PT_THREADS / LANES) {
    const int sl = sb + threadIdx.x / LANES;
    int p = -1, beg = 0, end = 0;
    if (sl < send) {
      p = wk.plist ? wk.plist[sl] : sl;
      beg = pt_off[p]; end = pt_off[p + 1];
      if (end - beg > wk.skip_thr) p = -1;          // long track: handled by the list-mode launch
    }
    double a[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (p >= 0) {
      const double4 X = *(const double4*)(ptab + PT * (size_t)p);
      // (ROBUST: index stream from the flagged copy, stored back only where the flag changes -- see k_camrow_linearize)
      const int* __restrict__ idx_in = ROBUST ? (const int*)p_camf : p_cam;
      int j = beg + sub;
      int cr = (j < end) ? ld_stream(idx_in + j) : 0;
      double2 uv = (j < end) ? p_uv[j] : make_double2(0, 0);
      while (j < end) {
        const int jn = j + LANES;
        const int cn = (jn < end) ? ld_stream(idx_in + jn) : 0;
        const double2 uvn = (jn < end) ? p_uv[jn] : make_double2(0, 0);
        const int c = ROBUST ? (cr & IDX_MASK) : cr;
        double row[CM::LIN_ROW];
        load_cam_row<CM::LIN_ROW, CM::TA>(use_lds, tab, camA, win.x, c, row);
        typename CM::template Obs<double> g;
        CM::template geom<false, double, double>(row, X.x, X.y, X.z, fx, fy, g);
        double ru, rv;
        CM::residual(g, uv.x, uv.y, fx, fy, cx, cy, ru, rv);
        const double* Pm = CM::pm(g);
        double w0 = 1.0, w1 = 1.0;
        if (ROBUST) {
          double t;
          robust_loss<false>(loss, ru, hub_c, t, w0);
          robust_loss<false>(loss, rv, hub_c, t, w1);
          const int cfl = flagged_index(c, w0, w1);
          if (cfl != cr) p_camf[j] = cfl;
          if (cfl < 0) p_w[j] = make_double2(w0, w1);      // unflagged weights are never read
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const double wa0 = w0 * Pm[q], wa1 = w1 * Pm[3 + q];
#pragma unroll
          for (int r = q; r < 3; ++r) a[U3(q, r)] += wa0 * Pm[r] + wa1 * Pm[3 + r];
          a[6 + q] -= wa0 * ru + wa1 * rv;       // Jp = -Pm
        }
        j = jn; cr = cn; uv = uvn;
      }
    }
#pragma unroll
    for (int q = 0; q < 9; ++q) a[q] = lanes_sum<LANES>(a[q]);
    if (!have_lambda) {
      // workgroup 0 never waits for anybody and is dispatched first, so this wait ends; by now it has usually ended long ago
      // RELAXED device-scope loads (served at the coherence point, nothing invalidated): an ACQUIRE here would make every
      // wave of the launch invalidate its CU's L1 (measured: the pass went from 21 to 99 us).  The word is 0 until the rider
      // stores the damping (always > 0) into it: the load that sees "ready" IS the value, no second word to order behind
      // it.  Bounded by the wall clock: a rider that never comes leaves an error word for the host instead of a hang.
      double lv = __hip_atomic_load(lam_slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (lv == 0.0) {
        const long long t_start = (long long)wall_clock64();
        int spins = 0;
        while ((lv = __hip_atomic_load(lam_slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == 0.0) {
          __builtin_amdgcn_s_sleep(8);
          if ((++spins & 255) == 0 && (long long)wall_clock64() - t_start > RIDER_WAIT_TICKS) {
            if (err_flag) __hip_atomic_store(err_flag, 1ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            lv = 1.0;                                    // (any finite damping: the host discards the solve)
            break;
          }
        }
      }
      lambda = lv;
      have_lambda = true;
    }
    if (p >= 0 && sub == LANES - 1) {
#pragma unroll
      for (int q = 0; q < 6; ++q) Hpp[6 * (size_t)p + q] = a[q];
#pragma unroll
      for (int q = 0; q < 3; ++q) { bp[3 * (size_t)p + q] = a[6 + q]; gm = nanmax(gm, fabs(a[6 + q])); }
      double h[6] = {a[0], a[1], a[2], a[3], a[4], a[5]}, inv[6], y[3];
      h[0] += lambda * fmax(h[0], DIAG_FLOOR);
      h[3] += lambda * fmax(h[3], DIAG_FLOOR);
      h[5] += lambda * fmax(h[5], DIAG_FLOOR);
      sym3_inverse(h, inv);
#pragma unroll
      for (int q = 0; q < 6; ++q) Hppinv[6 * (size_t)p + q] = inv[q];
      sym3_mul(inv, a + 6, y);
      y0[3 * (size_t)p] = y[0]; y0[3 * (size_t)p + 1] = y[1]; y0[3 * (size_t)p + 2] = y[2];
      double* o = ptab + PT * (size_t)p + 4;
      o[0] = y[0]; o[1] = y[1]; o[2] = y[2];
    }
  }
  gm = wave_nanmax(gm);
  if ((threadIdx.x & 63) == 0) smg[threadIdx.x >> 6] = gm;
  __syncthreads();
  if (threadIdx.x == 0) {
    double m = smg[0];
    for (int w = 1; w < PT_THREADS / 64; ++w) m = nanmax(m, smg[w]);
    partG[wk.blk_base + rb] = m;
  }
}

#define BA_LIN_PARAMS const double* __restrict__ camA, double* __restrict__ ptab, const int* __restrict__ pt_off,               \
                      const int* __restrict__ p_cam, const UvArr p_uv, const int2* __restrict__ blk_win
#define BA_LIN_TAIL double fx, double fy, double cx, double cy, double hub_c, int loss, double lambda, const double* __restrict__ lam_dev, \
                    double* __restrict__ Hpp, double* __restrict__ bp, double2* __restrict__ p_w, int* __restrict__ p_camf,      \
                    double* __restrict__ Hppinv, double* __restrict__ y0, double* __restrict__ partG, ScalarsArgs sa
// one kind of track per launch
template <class CM, bool ROBUST, bool ALL_LDS, int LANES>
__global__ void __launch_bounds__(PT_THREADS)
k_pt_linearize(BA_LIN_PARAMS, PtWork wk, BA_LIN_TAIL) {
  // the rider: workgroup 0; workgroups 1 .. NPART-1 leave at once, so that the point workgroups keep their XCD (= index mod NPART)
  if (sa.on && blockIdx.x < NPART) { if (blockIdx.x == 0) scalars_body(sa); return; }
  pt_linearize_body<CM, ROBUST, ALL_LDS, LANES>(camA, ptab, pt_off, p_cam, p_uv, blk_win, wk, (int)blockIdx.x - sa.on * NPART, (int)gridDim.x - sa.on * NPART,
                                            fx, fy, cx, cy, hub_c, loss, lambda, lam_dev, Hpp, bp, p_w, p_camf, Hppinv, y0, partG,
                                            sa.on ? sa.lam_slot : (const double*)nullptr, sa.err_flag);
}
// short and long tracks in one launch: workgroups [0, nblk_short) take the range list with LPP lanes
// per point, the rest the long-track list with a DPP row per point (saves a launch per pass on data
// with long tracks)
template <class CM, bool ROBUST, bool ALL_LDS>
__global__ void __launch_bounds__(PT_THREADS)
k_pt_linearize_both(BA_LIN_PARAMS, PtWork wk, int nblk_short, PtWork wl, BA_LIN_TAIL) {
  if (sa.on && blockIdx.x < NPART) { if (blockIdx.x == 0) scalars_body(sa); return; }      // the rider: workgroup 0 (1 .. NPART-1 idle, see k_pt_linearize)
  const int bid = (int)blockIdx.x - sa.on * NPART, nblk = (int)gridDim.x - sa.on * NPART;
  const double* lf = sa.on ? sa.lam_slot : (const double*)nullptr;
  if (bid < nblk_short)
    pt_linearize_body<CM, ROBUST, ALL_LDS, LPP>(camA, ptab, pt_off, p_cam, p_uv, blk_win, wk, bid, nblk_short, fx, fy, cx, cy,
                                            hub_c, loss, lambda, lam_dev, Hpp, bp, p_w, p_camf, Hppinv, y0, partG, lf, sa.err_flag);
  else
    pt_linearize_body<CM, ROBUST, ALL_LDS, LPP_LONG>(camA, ptab, pt_off, p_cam, p_uv, blk_win, wl, bid - nblk_short,
                                                 nblk - nblk_short, fx, fy, cx, cy, hub_c, loss, lambda, lam_dev, Hpp, bp, p_w,
                                                 p_camf, Hppinv, y0, partG, lf, sa.err_flag);
}
#undef BA_LIN_PARAMS
#undef BA_LIN_TAIL

// K3: damped 3x3 inverse per point and y0 = (Hpp + lam Dp)^-1 bp (also placed in the y
// slot of the point table, where the right-hand-side camera pass reads it).
__global__ void __launch_bounds__(256)
k_point_invert(const double* __restrict__ Hpp, const double* __restrict__ bp, double lambda, int n_pts,
               double* __restrict__ Hppinv, double* __restrict__ y0, double* __restrict__ ptab,
               const unsigned char* __restrict__ pt_held) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n_pts) return;
  double h[6], inv[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) h[k] = Hpp[6 * (size_t)p + k];
  h[0] += lambda * fmax(h[0], DIAG_FLOOR);
  h[3] += lambda * fmax(h[3], DIAG_FLOOR);
  h[5] += lambda * fmax(h[5], DIAG_FLOOR);
  sym3_inverse(h, inv);
  if (pt_held && pt_held[p]) {                     // held point: Hpp^-1 := 0 (its Hpp and bp are 0 already)
#pragma unroll
    for (int k = 0; k < 6; ++k) inv[k] = 0.0;
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) Hppinv[6 * (size_t)p + k] = inv[k];
  const double b[3] = {bp[3 * (size_t)p], bp[3 * (size_t)p + 1], bp[3 * (size_t)p + 2]};
  double y[3];
  sym3_mul(inv, b, y);
  y0[3 * (size_t)p] = y[0]; y0[3 * (size_t)p + 1] = y[1]; y0[3 * (size_t)p + 2] = y[2];
  double* o = ptab + PT * (size_t)p + 4;
  o[0] = y[0]; o[1] = y[1]; o[2] = y[2];
}

// Held points (ba_set_held) after a point half of the linearisation, which knows nothing of them: Hpp = bp = 0,
// Hpp^-1 := 0, y0 = 0 (also in the point table's y slot), and the gtol maxima redone without them -- one workgroup per
// partG word (the linearisation's count of them), grid-stride over every point slot.  Launched only while points are held.
__global__ void __launch_bounds__(256)
k_held_points(const unsigned char* __restrict__ pt_held, int n_pts, double* __restrict__ Hpp, double* __restrict__ bp,
              double* __restrict__ Hppinv, double* __restrict__ y0, double* __restrict__ ptab, double* __restrict__ partG) {
  __shared__ double smg[4];
  double gm = 0.0;
  for (int p = blockIdx.x * 256 + threadIdx.x; p < n_pts; p += gridDim.x * 256) {
    if (pt_held[p]) {
      for (int q = 0; q < 6; ++q) { Hpp[6 * (size_t)p + q] = 0.0; Hppinv[6 * (size_t)p + q] = 0.0; }
      for (int q = 0; q < 3; ++q) { bp[3 * (size_t)p + q] = 0.0; y0[3 * (size_t)p + q] = 0.0; ptab[PT * (size_t)p + 4 + q] = 0.0; }
    } else {
      for (int q = 0; q < 3; ++q) gm = nanmax(gm, fabs(bp[3 * (size_t)p + q]));
    }
  }
  gm = wave_nanmax(gm);
  if ((threadIdx.x & 63) == 0) smg[threadIdx.x >> 6] = gm;
  __syncthreads();
  if (threadIdx.x == 0) partG[blockIdx.x] = nanmax(nanmax(smg[0], smg[1]), nanmax(smg[2], smg[3]));
}

// Point priors (ba_set_priors) after a point half of the linearisation, which knows nothing of them (the shape of
// k_held_points, and ahead of it where both apply): Hpp += L_p, bp += L_p (X_p - mu_p), then the damped inverse, y0 and the
// point table's y slot redone at the damping the point half used (lam_dev != null: the device word a speculated pass read
// it from), and the gtol maxima redone.  info / mean in point-slot order; a zero block leaves its point untouched.
// Launched only while point priors are set.
__global__ void __launch_bounds__(256)
k_prior_points(const double* __restrict__ info, const double* __restrict__ mean, int n_pts, double lambda_arg,
               const double* __restrict__ lam_dev, double* __restrict__ Hpp, double* __restrict__ bp, double* __restrict__ Hppinv,
               double* __restrict__ y0, double* __restrict__ ptab, double* __restrict__ partG) {
  __shared__ double smg[4];
  const double lambda = lam_dev ? lam_dev[0] : lambda_arg;
  double gm = 0.0;
  for (int p = blockIdx.x * 256 + threadIdx.x; p < n_pts; p += gridDim.x * 256) {
    double L[6];
    bool any = false;
    for (int q = 0; q < 6; ++q) { L[q] = info[6 * (size_t)p + q]; any = any || L[q] != 0.0; }
    if (any) {
      double d[3], Ld[3], h[6], b[3], inv[6], y[3];
      for (int q = 0; q < 3; ++q) d[q] = ptab[PT * (size_t)p + q] - mean[3 * (size_t)p + q];
      sym3_mul(L, d, Ld);
      for (int q = 0; q < 6; ++q) { h[q] = Hpp[6 * (size_t)p + q] + L[q]; Hpp[6 * (size_t)p + q] = h[q]; }
      for (int q = 0; q < 3; ++q) { b[q] = bp[3 * (size_t)p + q] + Ld[q]; bp[3 * (size_t)p + q] = b[q]; }
      h[0] += lambda * fmax(h[0], DIAG_FLOOR);
      h[3] += lambda * fmax(h[3], DIAG_FLOOR);
      h[5] += lambda * fmax(h[5], DIAG_FLOOR);
      sym3_inverse(h, inv);
      sym3_mul(inv, b, y);
      for (int q = 0; q < 6; ++q) Hppinv[6 * (size_t)p + q] = inv[q];
      for (int q = 0; q < 3; ++q) { y0[3 * (size_t)p + q] = y[q]; ptab[PT * (size_t)p + 4 + q] = y[q]; }
    }
    for (int q = 0; q < 3; ++q) gm = nanmax(gm, fabs(bp[3 * (size_t)p + q]));
  }
  gm = wave_nanmax(gm);
  if ((threadIdx.x & 63) == 0) smg[threadIdx.x >> 6] = gm;
  __syncthreads();
  if (threadIdx.x == 0) partG[blockIdx.x] = nanmax(nanmax(smg[0], smg[1]), nanmax(smg[2], smg[3]));
}

// The prior terms of the objective at one parameter set, as PRIOR_ROWS extra rows of the residual partials:
// rows[b] = {0, sum (x - mu)^T L (x - mu)} over workgroup b's cameras and points (grid-stride, fixed order), so the scalar
// fold that adds nR + PRIOR_ROWS rows finds the total cost in its rho sum and the reprojection sse unchanged.
// pr.info == null: no camera part (also rank > 0 of a multi-rank job: the camera sum counts once); pt_info == null: no point part.
constexpr int PRIOR_ROWS = 32;
__global__ void __launch_bounds__(256)
k_prior_cost(CamPriors pr, int n_cams, const double* __restrict__ pt_info, const double* __restrict__ pt_mean,
             const double* __restrict__ ptab, int n_pts, double* __restrict__ rows) {
  __shared__ double sm[4];
  double acc = 0.0;
  if (pr.info) {
    const int nb = pr.nb, nh = nb * (nb + 1) / 2;
    for (int c = blockIdx.x * 256 + threadIdx.x; c < n_cams; c += gridDim.x * 256) {
      const double* __restrict__ L = pr.info + (size_t)nh * c;
      double d[9];
      for (int q = 0; q < nb; ++q) d[q] = (q < 6 ? pr.cams[6 * (size_t)c + q] : pr.intr[3 * (size_t)c + (q - 6)]) - pr.mean[(size_t)nb * c + q];
      double s = 0.0;
      for (int i = 0; i < nb; ++i)
        for (int j = i; j < nb; ++j) s += (j > i ? 2.0 : 1.0) * L[UT(nb, i, j)] * d[i] * d[j];
      acc += s;
    }
  }
  if (pt_info) {
    for (int p = blockIdx.x * 256 + threadIdx.x; p < n_pts; p += gridDim.x * 256) {
      double d[3], Ld[3];
      for (int q = 0; q < 3; ++q) d[q] = ptab[PT * (size_t)p + q] - pt_mean[3 * (size_t)p + q];
      sym3_mul(pt_info + 6 * (size_t)p, d, Ld);
      acc += d[0] * Ld[0] + d[1] * Ld[1] + d[2] * Ld[2];
    }
  }
  acc = wave_total_dpp(acc);
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) { rows[2 * blockIdx.x] = 0.0; rows[2 * blockIdx.x + 1] = (sm[0] + sm[1]) + (sm[2] + sm[3]); }
}
// rows in the caller's point order -> point slots (ba_set_priors): out[slot[p]][0..W) = in[p][0..W)
__global__ void k_scatter_rows(const double* __restrict__ in, const int* __restrict__ slot, int n_pts, int width, double* __restrict__ out) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pts) return;
  for (int q = 0; q < width; ++q) out[(size_t)slot[p] * width + q] = in[(size_t)p * width + q];
}

// K4a / K6: point pass of the Schur product.  u = sum_o Jp^T w (Jc v_c) with
//   Jc v = P (X x vt_r) - dpi vt_t,  vt = (M v_r, v_t) = camA[c][12..17].
// MODE 0 (PCG): y[p] = Hppinv u into the point table, partA[block] = sum u.y; early exit when done.
// MODE 1 (back substitution): dp = -(y0 + Hppinv u), trial point = X + dp, partB[block][4] =
//         bp.dp, sum Dp dp^2, |dp|^2, |X|^2.
// Head of a PCG iteration, run by wave 0 of every point-pass workgroup (all 64 lanes): sum the vector kernel's
// partials and decide whether iteration kit runs.  Workgroup 0 also (i) leaves the verdict word for the iteration's
// other kernels, (ii) on the first probe behind a fresh linearisation folds max |gradient| from the partials of the
// point half (partG) and of k_pcg_setup (partGc) into host-mapped memory -- the reference's gtol test costs no kernel
// of its own -- and (iii) tells the host NOW whether this iteration runs (it then queues the next one behind it) or
// PCG is over (it queues the step kernels instead).
__device__ inline bool pcg_probe(int kit, const PcgState* __restrict__ st, const double* __restrict__ partV, int nblkV,
                                 double tol2, int min_iters, long long* __restrict__ host_flag, long long flag_base,
                                 double* __restrict__ verdict, const double* __restrict__ partG, int nG,
                                 const double* __restrict__ partGc, int nGc, double* __restrict__ gmax_out) {
  double g, z;
  const bool fin = pcg_finished(kit, st, partV, nblkV, tol2, min_iters, g, z);
  double gmx = 0.0;
  if (gmax_out && blockIdx.x == 0) {
    for (int b = threadIdx.x; b < nG; b += 64) gmx = nanmax(gmx, partG[b]);
    for (int b = threadIdx.x; b < nGc; b += 64) gmx = nanmax(gmx, partGc[b]);
    gmx = wave_nanmax(gmx);
  }
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    if (gmax_out) gmax_out[0] = gmx;      // ordered ahead of the sequence word by publish_flag's release
    double* vd = verdict + 4 * (kit & 1);
    vd[0] = g; vd[1] = z; vd[2] = fin ? 1.0 : 0.0;
    const PcgState& s = st[kit & 1];
    publish_flag(host_flag, flag_base + kit + 1, fin ? (long long)(s.done ? s.iters : kit) + 1 : 0);
  }
  return fin;
}
// The probe alone: a rank whose landmark shard is empty has no point pass to launch, but its host loop and the
// other kernels of the iteration still need the verdict (multi-rank jobs).  partA has no entries then.
__global__ void __launch_bounds__(64)
k_pcg_probe(int kit, const PcgState* __restrict__ st, const double* __restrict__ partV, int nblkV, double tol2, int min_iters,
            long long* __restrict__ host_flag, long long flag_base, double* __restrict__ verdict,
            const double* __restrict__ partG, int nG, const double* __restrict__ partGc, int nGc, double* __restrict__ gmax_out) {
  (void)pcg_probe(kit, st, partV, nblkV, tol2, min_iters, host_flag, flag_base, verdict, partG, nG, partGc, nGc, gmax_out);
}

template <class CM, bool ROBUST, int MODE, bool ALL_LDS, int LANES, typename JT>
__device__ __forceinline__ void
pt_schur_body(const double* __restrict__ camA, double* __restrict__ ptab, const int* __restrict__ pt_off,
              const int* __restrict__ p_cam, const double2* __restrict__ p_w, const double* __restrict__ Hppinv,
              const int2* __restrict__ blk_win, const PtWork& wk, int bid, int nblk,
              double fx, double fy, int fixed_cam, double* __restrict__ partA,
              int kit, const PcgState* __restrict__ st, const double* __restrict__ partV, int nblkV, double tol2,
              int min_iters,
              const double* __restrict__ y0, const double* __restrict__ Hpp, const double* __restrict__ bp,
              double* __restrict__ ptab_trial, double* __restrict__ partB,
              long long* __restrict__ host_flag, long long flag_base, double* __restrict__ verdict,
              const double* __restrict__ partG, int nG, const double* __restrict__ partGc, int nGc, double* __restrict__ gmax_out,
              const CamUpdateArgs& cu) {
  extern __shared__ __align__(16) double tab[];   // 16-byte aligned: the table is read and written with b128 LDS operations
  __shared__ double sm[4 * (PT_THREADS / 64)];
  if (MODE == 0) { BA_STAMP(0, 0); BA_STAMP(0, 1); }
  // the workgroup's window and the first round's track bounds are fetched before the PCG verdict
  // is known: one round trip less on the way to the first camera row
  const int rb = pt_range_of_block(bid, nblk, wk.xcd_ranges);
  const int2 win = blk_win[wk.blk_base + rb];
  const int send = min(wk.n_slots, (rb + 1) * wk.slots_per_block);
  const int sb0 = rb * wk.slots_per_block;
  int p0 = -1, beg0 = 0, end0 = 0;
  if (sb0 + (int)(threadIdx.x / LANES) < send) {
    p0 = wk.plist ? wk.plist[sb0 + threadIdx.x / LANES] : sb0 + (int)(threadIdx.x / LANES);
    beg0 = pt_off[p0];
    end0 = pt_off[p0 + 1];
  }
  const bool use_lds = ALL_LDS || (size_t)win.y * CM::TA * sizeof(double) <= LDS_TAB_BYTES;   // ALL_LDS: every window fits
  bool table_ready = !use_lds;
  // MODE 0 with cu.fuse: the launch that finds PCG finished (s_fin) does not leave -- it already holds the table (the copy
  // started before the verdict was known), so it drops the ITERATE's vt (vx, kept current by the vector kernels) into the
  // rows' vector slots and walks its observations as the back substitution (MODE 1's epilogue); the host, which reads the
  // same verdict, does not launch one.  One launch and one table copy less per LM iteration.
  bool back = MODE == 1;
  // The table copy starts BEFORE the PCG verdict is known: the copy does not depend on it (the previous kernel of the
  // stream wrote the table), and its round trips hide the probe's.  A launch that turns out to be past the end of PCG
  // pays for a copy it does not use -- one launch per LM iteration against a round trip saved in every working one.
  __shared__ int s_fin;
  if (use_lds) fill_cam_table_issue<PT_THREADS, CM::TA, MODE == 0>(tab, camA, win.x, win.y);
  if (MODE == 0) {
    // wave 0 sums the vector kernel's partials and decides for the workgroup while the other waves copy
    if (threadIdx.x < 64) {
      const bool fin = pcg_probe(kit, st, partV, nblkV, tol2, min_iters, host_flag, flag_base, verdict, partG, nG, partGc, nGc, gmax_out);
      if (threadIdx.x == 0) s_fin = fin ? 1 : 0;
    }
    BA_STAMP(0, 2);
    if (!use_lds) {
      __syncthreads();
      if (s_fin) return;
    }
  }
  const int sub = threadIdx.x % LANES;
  double acc[4] = {0, 0, 0, 0};
  for (int sb = sb0; sb < send; sb += PT_THREADS / LANES) {
    const int sl = sb + threadIdx.x / LANES;
    int p = -1, j = 0, end = 0, c = 0, cn = 0;   // ROBUST: p_cam is the flagged copy
    double u[3] = {0, 0, 0};
    double4 X = make_double4(0, 0, 0, 0);
    double hi[6] = {0, 0, 0, 0, 0, 0};
    double2 w = make_double2(1.0, 1.0);
    if (sl < send) {                     // first loads of the index stream go out before the table fill
      int beg;
      if (sb == sb0) { p = p0; beg = beg0; end = end0; }
      else {
        p = wk.plist ? wk.plist[sl] : sl;
        beg = pt_off[p];
        end = pt_off[p + 1];
      }
      if (end - beg > wk.skip_thr) { p = -1; end = 0; }     // long track: list-mode launch
      else {
        X = *(const double4*)(ptab + PT * (size_t)p);
        j = beg + sub;
        c = (j < end) ? ld_stream(p_cam + j) : 0;
        cn = (j + LANES < end) ? ld_stream(p_cam + (j + LANES)) : 0;
        if (ROBUST && c < 0) w = ld_stream(p_w + j);
        if (sub == LANES - 1) {
          const double2* hp = (const double2*)(Hppinv + 6 * (size_t)p);
          const double2 h01 = hp[0], h23 = hp[1], h45 = hp[2];
          hi[0] = h01.x; hi[1] = h01.y; hi[2] = h23.x; hi[3] = h23.y; hi[4] = h45.x; hi[5] = h45.y;
        }
      }
    }
    if (!table_ready) {
      if (MODE == 0 && cu.fuse) {
        // The verdict is known long before the table has landed (wave 0's probe: ~1 us, the copy: ~4 us after entry).  One
        // barrier that waits for LDS only -- not for the copy, not for the index loads in flight -- hands s_fin to every
        // wave, and the launch that finished fetches the first four words per thread of its window's vx slice while the
        // copy is still under way, as MODE 1 does; they go into the rows once the copy has landed.
        constexpr int NBm = CM::NB;
        const int nw = win.y * NBm;
        const double* __restrict__ src = cu.vx + NBm * (size_t)win.x;
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        const bool fin = s_fin != 0;
        // (the thread's index as a value born here: the addresses below are then computed here, where they are used once,
        // and not ahead of the slot loop, where they were kept live across the first index loads and spilled)
        int tid = (int)threadIdx.x;
        asm volatile("" : "+v"(tid));
        double v0[4] = {0.0, 0.0, 0.0, 0.0};
        if (fin) {
#pragma unroll
          for (int q = 0; q < 4; ++q) { const int e = tid + q * PT_THREADS; if (e < nw) v0[q] = src[e]; }
        }
        fill_cam_table_wait();
        if (fin) {
          back = true;
#pragma unroll
          for (int q = 0; q < 4; ++q) { const int e = tid + q * PT_THREADS; if (e < nw) tab[CM::TA * (e / NBm) + CM::VOFF + e % NBm] = v0[q]; }
          for (int e0 = tid + 4 * PT_THREADS; e0 < nw; e0 += 4 * PT_THREADS) {      // four loads in flight per thread
            double v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) { const int e = e0 + q * PT_THREADS; v[q] = e < nw ? src[e] : 0.0; }
#pragma unroll
            for (int q = 0; q < 4; ++q) { const int e = e0 + q * PT_THREADS; if (e < nw) tab[CM::TA * (e / NBm) + CM::VOFF + e % NBm] = v[q]; }
          }
          __syncthreads();
        }
      } else if (MODE == 1 && cu.n_blocks > 0) {
        // the camera update rides along this launch (extra workgroups), so nobody has put the step's vt = (M dc_r, dc_t, ..)
        // into the table rows: the PCG vector kernels keep that form of their iterate in vx (NB doubles per camera, dense),
        // and the window's slice of it is dropped into the LDS rows here -- fetched while the table copy is in flight
        constexpr int NBm = CM::NB;
        const int nw = win.y * NBm;                      // doubles of vx this window needs, contiguous from NBm * win.x
        const double* __restrict__ src = cu.vx + NBm * (size_t)win.x;
        int e = threadIdx.x;
        double v0 = 0.0, v1 = 0.0;
        const int e1 = e + PT_THREADS;
        if (e < nw) v0 = src[e];
        if (e1 < nw) v1 = src[e1];
        fill_cam_table_wait();
        if (e < nw) tab[CM::TA * (e / NBm) + CM::VOFF + e % NBm] = v0;
        if (e1 < nw) tab[CM::TA * (e1 / NBm) + CM::VOFF + e1 % NBm] = v1;
        for (e += 2 * PT_THREADS; e < nw; e += PT_THREADS) tab[CM::TA * (e / NBm) + CM::VOFF + e % NBm] = src[e];
        __syncthreads();
      } else {
        fill_cam_table_wait();
      }
      table_ready = true;
      if (MODE == 0 && s_fin && !back) return;
    }
    if (MODE == 0 && sb == sb0) BA_STAMP(0, 3);
    if (p >= 0) {
      while (j < end) {
        // index two observations ahead, weight (only where it is not (1, 1)) one ahead
        const int jn = j + LANES, jnn = jn + LANES;
        const int cnn = (jnn < end) ? ld_stream(p_cam + jnn) : 0;
        double2 wn = make_double2(1.0, 1.0);
        if (ROBUST && cn < 0) wn = ld_stream(p_w + jn);
        const int cc = ROBUST ? (c & IDX_MASK) : c;
        if (cc != fixed_cam) {
          double rowd[CM::SCH_ROW];
          load_cam_row<CM::SCH_ROW, CM::TA>(use_lds, tab, camA, win.x, cc, rowd);
          JT row[CM::SCH_ROW];                   // Jacobian blocks in JT (double, or float for config 5)
#pragma unroll
          for (int q = 0; q < CM::SCH_ROW; ++q) row[q] = (JT)rowd[q];
          const JT X0 = (JT)X.x, X1 = (JT)X.y, X2 = (JT)X.z;
          typename CM::template Obs<JT> g;
          CM::template geom<true, JT, JT>(row, X0, X1, X2, (JT)fx, (JT)fy, g);
          JT s0, s1;
          CM::jc_times(g, X0, X1, X2, row + CM::VOFF, s0, s1);      // Jc vt
          s0 *= (JT)w.x; s1 *= (JT)w.y;
          const JT* Pm = CM::pm(g);
          u[0] -= (double)(Pm[0] * s0 + Pm[3] * s1);        // Jp^T (.), Jp = -Pm; sums always in fp64
          u[1] -= (double)(Pm[1] * s0 + Pm[4] * s1);
          u[2] -= (double)(Pm[2] * s0 + Pm[5] * s1);
        }
        j = jn; c = cn; cn = cnn; w = wn;
      }
    }
    if (MODE == 0 && sb == sb0) BA_STAMP(0, 4);
#pragma unroll
    for (int q = 0; q < 3; ++q) u[q] = lanes_sum<LANES>(u[q]);
    if (p >= 0 && sub == LANES - 1) {
      double yy[3];
      sym3_mul(hi, u, yy);
      if (!back) {
        double* o = ptab + PT * (size_t)p + 4;
        o[0] = yy[0]; o[1] = yy[1]; o[2] = yy[2];
        acc[0] += u[0] * yy[0] + u[1] * yy[1] + u[2] * yy[2];
      } else {
        const double d0 = -(y0[3 * (size_t)p] + yy[0]);
        const double d1 = -(y0[3 * (size_t)p + 1] + yy[1]);
        const double d2 = -(y0[3 * (size_t)p + 2] + yy[2]);
        double* o = ptab_trial + PT * (size_t)p;
        o[0] = X.x + d0; o[1] = X.y + d1; o[2] = X.z + d2;
        const double D0 = fmax(Hpp[6 * (size_t)p], DIAG_FLOOR), D1 = fmax(Hpp[6 * (size_t)p + 3], DIAG_FLOOR),
                     D2 = fmax(Hpp[6 * (size_t)p + 5], DIAG_FLOOR);
        acc[0] += bp[3 * (size_t)p] * d0 + bp[3 * (size_t)p + 1] * d1 + bp[3 * (size_t)p + 2] * d2;
        acc[1] += D0 * d0 * d0 + D1 * d1 * d1 + D2 * d2 * d2;
        acc[2] += d0 * d0 + d1 * d1 + d2 * d2;
        acc[3] += X.x * X.x + X.y * X.y + X.z * X.z;
      }
    }
  }
  if (!table_ready) {                      // a workgroup without a single slot: the copy must still land before it leaves
    fill_cam_table_wait();
    if (MODE == 0 && s_fin) { if (!cu.fuse) return; back = true; }       // (fused: its four zero sums are still owed)
  }
  if (MODE == 0) BA_STAMP(0, 5);
  // the PCG pass carries one sum (u . y), the back substitution four
  if (back) {
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = wave_total_dpp(acc[q]);
    block_combine<4, PT_THREADS, 4>(acc, sm);
    if (threadIdx.x == 0) { for (int q = 0; q < 4; ++q) partB[4 * (wk.blk_base + rb) + q] = acc[q]; }
  } else {
    acc[0] = wave_total_dpp(acc[0]);
    block_combine<1, PT_THREADS, 4>(acc, sm);
    if (threadIdx.x == 0) partA[wk.blk_base + rb] = acc[0];
  }
  if (MODE == 0) { BA_STAMP(0, 6); BA_STAMP(0, 7); }
}

#define BA_SCH_PARAMS const double* __restrict__ camA, double* __restrict__ ptab, const int* __restrict__ pt_off,               \
                      const int* __restrict__ p_cam, const double2* __restrict__ p_w, const double* __restrict__ Hppinv,     \
                      const int2* __restrict__ blk_win
#define BA_SCH_TAIL double fx, double fy, int fixed_cam, double* __restrict__ partA, int kit, const PcgState* __restrict__ st, \
                    const double* __restrict__ partV, int nblkV, double tol2, int min_iters, const double* __restrict__ y0,    \
                    const double* __restrict__ Hpp, const double* __restrict__ bp, double* __restrict__ ptab_trial,            \
                    double* __restrict__ partB, long long* __restrict__ host_flag, long long flag_base,                     \
                    double* __restrict__ verdict, const double* __restrict__ partG, int nG, const double* __restrict__ partGc, \
                    int nGc, double* __restrict__ gmax_out, CamUpdateArgs cu
#define BA_SCH_TAIL_ARGS fx, fy, fixed_cam, partA, kit, st, partV, nblkV, tol2, min_iters, y0, Hpp, bp, ptab_trial, partB,       \
                         host_flag, flag_base, verdict, partG, nG, partGc, nGc, gmax_out, cu
#define BA_SCH_RIDER_ARGS kit, st, partV, nblkV, tol2, min_iters, host_flag, flag_base, verdict, partG, nG, partGc, nGc, gmax_out, cu
// The workgroups in front of the point workgroups of a back-substitution launch (MODE 1), or of a PCG point pass that may
// turn into one (MODE 0, cu.fuse): the camera update (riders).  True: this workgroup was a rider and is done.
//   MODE 1: workgroup 0 also clears the riding verdict's damping word (ScalarsArgs::lam_slot).
//   MODE 0: wave 0 runs the PCG probe like every point workgroup; the camera update runs only in the launch that finds PCG
//           finished -- together with the cleared word.
template <class CM, int MODE>
__device__ __forceinline__ bool
pt_schur_rider(int n_rider, int kit, const PcgState* __restrict__ st, const double* __restrict__ partV, int nblkV, double tol2,
               int min_iters, long long* __restrict__ host_flag, long long flag_base, double* __restrict__ verdict,
               const double* __restrict__ partG, int nG, const double* __restrict__ partGc, int nGc, double* __restrict__ gmax_out,
               const CamUpdateArgs& cu) {
  if (MODE == 1 && blockIdx.x == 0 && threadIdx.x == 0 && cu.lam_slot) cu.lam_slot[0] = 0.0;
  // MODE 1: the riders are the FIRST workgroups of the launch.  MODE 0 (a PCG point pass that may go on as the back
  // substitution): the LAST ones -- in all but one launch per LM iteration they only probe and leave, and at the front they
  // held the point workgroups' dispatch back (0.6 us per launch); workgroup 0, a point workgroup again, publishes the verdict
  const int ridx = (MODE == 0) ? (int)blockIdx.x - ((int)gridDim.x - n_rider) : (int)blockIdx.x;
  if (ridx < 0 || ridx >= n_rider) return false;
  extern __shared__ __align__(16) double tab[];
  if (MODE == 0) {
    // the waves without a camera group leave at once; each of the others probes for itself (the same words, the same
    // verdict in every wave) -- no workgroup barrier in the launches that only probe
    if ((int)(threadIdx.x >> 6) >= cu.groups) return true;
    if (!pcg_probe(kit, st, partV, nblkV, tol2, min_iters, host_flag, flag_base, verdict, partG, nG, partGc, nGc, gmax_out)) return true;
    if (ridx == 0 && threadIdx.x == 0 && cu.lam_slot) cu.lam_slot[0] = 0.0;
  }
  cam_update_rider<CM>(cu, ridx, tab);
  return true;
}
template <class CM, bool ROBUST, int MODE, bool ALL_LDS, int LANES, typename JT>
__global__ void __launch_bounds__(PT_THREADS)
k_pt_schur(BA_SCH_PARAMS, PtWork wk, BA_SCH_TAIL) {
  const int n_rider = (MODE == 1 || cu.fuse) ? cu.n_blocks : 0;           // the camera update's workgroups (pt_schur_rider: where they sit)
  if (pt_schur_rider<CM, MODE>(n_rider, BA_SCH_RIDER_ARGS)) return;
  pt_schur_body<CM, ROBUST, MODE, ALL_LDS, LANES, JT>(camA, ptab, pt_off, p_cam, p_w, Hppinv, blk_win, wk,
                                                  (int)blockIdx.x - (MODE == 1 ? n_rider : 0), (int)gridDim.x - n_rider, BA_SCH_TAIL_ARGS);
}
// short and long tracks in one launch (see k_pt_linearize_both)
template <class CM, bool ROBUST, int MODE, bool ALL_LDS, typename JT>
__global__ void __launch_bounds__(PT_THREADS)
k_pt_schur_both(BA_SCH_PARAMS, PtWork wk, int nblk_short, PtWork wl, BA_SCH_TAIL) {
  const int n_rider = (MODE == 1 || cu.fuse) ? cu.n_blocks : 0;
  if (pt_schur_rider<CM, MODE>(n_rider, BA_SCH_RIDER_ARGS)) return;
  const int bid = (int)blockIdx.x - (MODE == 1 ? n_rider : 0);
  if (bid < nblk_short)
    pt_schur_body<CM, ROBUST, MODE, ALL_LDS, LPP, JT>(camA, ptab, pt_off, p_cam, p_w, Hppinv, blk_win, wk, bid, nblk_short,
                                                  BA_SCH_TAIL_ARGS);
  else
    pt_schur_body<CM, ROBUST, MODE, ALL_LDS, LPP_LONG, JT>(camA, ptab, pt_off, p_cam, p_w, Hppinv, blk_win, wl,
                                                       bid - nblk_short, (int)gridDim.x - n_rider - nblk_short, BA_SCH_TAIL_ARGS);
}
#undef BA_SCH_PARAMS
#undef BA_SCH_TAIL
#undef BA_SCH_TAIL_ARGS
#undef BA_SCH_RIDER_ARGS

// -------------------------------------------------------------------------------------
// reduced-camera-system vector kernels (one thread per camera)
// -------------------------------------------------------------------------------------
// ---- device-side all-reduce of the reduced camera system's product (multi-rank jobs, BA_IPC=1) ----------------------
// Once per PCG iteration every rank owes every other rank its folded Schur product W y (NB Nc doubles) and its u.y word:
// 48 KB at the headline size, a message whose all-reduce is pure latency (an RCCL launch + a ring over xGMI: 10-20 us).
// Here the exchange happens INSIDE the vector kernel (k_pcg_step), workgroup by workgroup, with no kernel of its own:
// workgroup b owns VC consecutive cameras on every rank, so it only ever needs the other ranks' workgroup b.  It folds its
// cameras' partitions (fixed order), STORES the record [u.y, 0 | NB VC sums] straight into slot (parity, own rank, b) of
// every peer's receive buffer (buffers exported with hipIpcGetMemHandle when the communicator comes up, fine-grained
// device memory: stores go through to the fabric, loads are not cached), fences, stores the exchange's sequence number
// into the peers' flag word for (parity, own rank, b), waits for the `world` flag words of its own buffer and adds the
// `world` records in RANK ORDER -- every rank computes the same bits (and the same as the host-staged test transport,
// which also adds in rank order).  Slots are double-buffered by the parity of the exchange number: workgroup b of a rank
// can be at most one exchange ahead of a peer's workgroup b (its next wait needs that peer's next flag, stored only after
// the peer's previous k_pcg_step has finished), so the record it overwrites two exchanges later has been read.
constexpr int IPC_MAX_WORLD = 8;
constexpr int IPC_MAX_BLOCKS = 512;             // camera-vector workgroups a flag array holds per (parity, sender)
struct IpcPeers {
  double* recv[IPC_MAX_WORLD];                  // every rank's receive buffer as mapped in THIS process ([rank]: the own one)
  unsigned long long* flags[IPC_MAX_WORLD];
};
struct IpcStep {                                // one exchange (k_pcg_step); on == 0: single rank or the base transport
  IpcPeers P;
  int on, rank, world, parity;
  long long seq;
  size_t stride;                                // doubles per (parity, sender) slot of a receive buffer
};
constexpr long long IPC_WAIT_TICKS = 1000000000; // 10 s of the 100 MHz wall clock: a peer that never sends
// consumer side (whole wave): lane s < world waits for sender s's flag of (parity, workgroup b) to reach seq; false = timed out
__device__ inline bool ipc_wait(const unsigned long long* __restrict__ flags, int world, int parity, int b, long long seq) {
  bool ok = true;
  const int s = threadIdx.x & 63;
  if (s < world) {
    const unsigned long long* f = flags + ((size_t)parity * world + s) * IPC_MAX_BLOCKS + b;
    if (__hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) < (unsigned long long)seq) {
      const long long t0 = (long long)wall_clock64();
      int spins = 0;
      while (__hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) < (unsigned long long)seq) {
        __builtin_amdgcn_s_sleep(2);
        if ((++spins & 255) == 0 && (long long)wall_clock64() - t0 > IPC_WAIT_TICKS) { ok = false; break; }
      }
    }
  }
  // (the record loads are system-scope atomic loads of fine-grained memory -- never served from a cache -- issued behind the
  // loop that saw the flags: no acquire fence, whose L2 invalidate the rest of the kernel would pay for)
  asm volatile("" ::: "memory");
  return __all(ok);
}

// ---- cooperative staging for the camera-vector kernels ---------------------------------------------
// A camera-vector workgroup (one wave) owns VEC_CAMS consecutive cameras, whose rows are CONTIGUOUS in every
// per-camera array.  A thread per camera reading its own row issues one 8-byte load per word with 16 live
// lanes, each lane on its own cache line (k_pcg_step: ~120 such loads, 3.7 of its 4.6 us by in-kernel
// stamps).  Instead all 64 lanes copy the workgroup's slice of every array with 16-byte coalesced loads --
// every load issued before the first LDS store -- and the per-camera arithmetic then reads LDS.
struct VecSlice { const double* src; int len; };        // len doubles from src (16-byte aligned)
template <int NL>
__device__ inline void slice_load(const VecSlice& sl, double2 (&v)[NL]) {     // NL * 64 double2 cover the slice
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int u = 0; u < NL; ++u) {
    const int i = u * 64 + lane;
    v[u] = make_double2(0.0, 0.0);
    if (2 * i + 1 < sl.len) v[u] = ((const double2*)sl.src)[i];
    else if (2 * i < sl.len) v[u].x = sl.src[2 * i];
  }
}
template <int NL>
__device__ inline void slice_store_lds(double* __restrict__ lds, int cap, const double2 (&v)[NL]) {   // cap: doubles reserved (even)
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int u = 0; u < NL; ++u) {
    const int i = u * 64 + lane;
    if (2 * i < cap) ((double2*)lds)[i] = v[u];
  }
}
// LDS -> global, len doubles (dst 16-byte aligned)
__device__ inline void slice_write_back(double* __restrict__ dst, const double* __restrict__ lds, int len) {
  const int lane = threadIdx.x & 63;
  for (int i = lane; 2 * i < len; i += 64) {
    if (2 * i + 1 < len) ((double2*)dst)[i] = ((const double2*)lds)[i];
    else dst[2 * i] = lds[2 * i];
  }
}
// The same in ONE round: every LDS read is issued before the first store (slice_write_back's loop waits for each read in
// turn: one LDS round trip per 64 double2, 13 of them at the end of k_pcg_setup)
template <int NL>
__device__ inline void slice_load_lds(const double* __restrict__ lds, int cap, double2 (&v)[NL]) {   // cap: doubles reserved (even)
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int u = 0; u < NL; ++u) {
    const int i = u * 64 + lane;
    v[u] = make_double2(0.0, 0.0);
    if (2 * i < cap) v[u] = ((const double2*)lds)[i];
  }
}
template <int NL>
__device__ inline void slice_store(double* __restrict__ dst, int len, const double2 (&v)[NL]) {     // len doubles to dst (16-byte aligned)
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int u = 0; u < NL; ++u) {
    const int i = u * 64 + lane;
    if (2 * i + 1 < len) ((double2*)dst)[i] = v[u];
    else if (2 * i < len) dst[2 * i] = v[u].x;
  }
}
static_assert(BalCam::VC == 16 || BalCam::VC == 8 || BalCam::VC == 4, "camera-vector workgroups: 4, 8 or 16 cameras per wave");
constexpr int slice_chunks(int doubles) { return (doubles + 127) / 128; }      // double2 per lane that cover a slice

// PCG setup at damping lambda: Hccd = Hcc + lam Dc (fixed camera: identity), Schur-Jacobi
// or Jacobi preconditioner Minv = (Hccd - E)^-1, right-hand side g = -(bc - W y0), and the
// (FINALIZE: first folds the fresh linearisation partials into Hcc | bc, single rank)
// first PCG vectors: x = 0, r = g, z = Minv r, p = s = 0, vtil, gamma/zeta partials.
// use_schur_diag: 0 = Jacobi blocks, 1 = Schur-Jacobi blocks from partE, 2 = KEEP the blocks in Minv (built for an earlier
// damped system, ba_options.precond_lag): partE is not read, nothing is inverted, Minv is not written.
// The partial sums (linearisation, E, Wy0) come either as NPART partitions (nparts = NPART) or already folded and
// all-reduced in partition 0 (nparts = 1; the other partitions are stale then).  CM: the camera model (block size NB = 6 or 9, table row layout).
template <class CM, bool FINALIZE>
__global__ void __launch_bounds__(VEC_BLOCK)
k_pcg_setup(const double* __restrict__ partL, double* __restrict__ Hcc, double* __restrict__ bc, const double* __restrict__ part6,
            const double* __restrict__ partE, int nparts, const double* __restrict__ cs, double lambda,
            int use_schur_diag, int n_cams, int fixed_cam, double* __restrict__ Hccd, double* __restrict__ Minv,
            double* __restrict__ gvec, double* __restrict__ x, double* __restrict__ r, double* __restrict__ p,
            double* __restrict__ s, double* __restrict__ z, double* __restrict__ vtil,
            double* __restrict__ partV, PcgState* __restrict__ st, double* __restrict__ partGc,
            double* __restrict__ vx, const unsigned short* __restrict__ cam_held, CamPriors pr,
            const int* __restrict__ cam_gl) {
  // cam_gl (shared intrinsics, null = none): a grouped camera leaves its per-camera terms here and k_shared_sum /
  // k_shared_finish behind this kernel put the group sums in their place (see "shared intrinsics" below)
  constexpr int NB = CM::NB, NH = CM::NH, NL = CM::NL, VC = CM::VC;
  // LDS image of the workgroup's VC cameras.  Inputs: partition-folded sums (a: NL of the linearisation when
  // FINALIZE, e: NH Schur-Jacobi, w6: NB of W y0), Hcc | bc (when not FINALIZE), cs.  Outputs staged for a
  // coalesced write-back: Hcc | bc (FINALIZE), Hccd, Minv, g = r, z (x = p = s = 0 written directly).
  __shared__ double l_a[NL * VC], l_e[NH * VC], l_w6[NB * VC], l_cs[CS * VC], l_hcc[NH * VC], l_bc[NB * VC],
      l_hd[NH * VC], l_mi[NH * VC], l_g[NB * VC], l_z[NB * VC];
  const int c0 = blockIdx.x * VC;
  const int nc = min(VC, n_cams - c0);
  const int c = vec_camera<VC>(n_cams);
  const int lane = threadIdx.x;
  BA_STAMP(3, 0); BA_STAMP(3, 1);
  // ---- cooperative loads: every word of the workgroup's slices, lane-strided and coalesced; the partition
  // sums run k = 0, 1, ... in every element (the same fixed order as a thread-per-camera loop)
  {
    double2 vc[slice_chunks(CS * VC)], vh[slice_chunks(NH * VC)], vb[slice_chunks(NB * VC)];
    slice_load(VecSlice{cs + CS * (size_t)c0, CS * nc}, vc);
    if (use_schur_diag == 2) {                       // kept preconditioner blocks: straight into their LDS image
      double2 vm[slice_chunks(NH * VC)];
      slice_load(VecSlice{Minv + NH * (size_t)c0, NH * nc}, vm);
      slice_store_lds(l_mi, NH * VC, vm);
    }
    if (!FINALIZE) {
      slice_load(VecSlice{Hcc + NH * (size_t)c0, NH * nc}, vh);
      slice_load(VecSlice{bc + NB * (size_t)c0, NB * nc}, vb);
    }
    constexpr int NA = (NL * VC + 63) / 64, NE = (NH * VC + 63) / 64, NW = (NB * VC + 63) / 64;
    double sa[NA], se[NE], sw[NW];
#pragma unroll
    for (int j = 0; j < NA; ++j) sa[j] = 0.0;
#pragma unroll
    for (int j = 0; j < NE; ++j) se[j] = 0.0;
#pragma unroll
    for (int j = 0; j < NW; ++j) sw[j] = 0.0;
    const int la = NL * nc, le = NH * nc, lw = NB * nc;
    // ONE round of loads: every partition's words are requested before the first add.  The kernel is a single wave
    // lifetime of cold loads (the partitions were written from other XCDs one launch earlier), so each round of loads
    // that is waited for is a trip to memory on its critical path; a wave per workgroup has the registers for all
    // NPART * (NA + NE + NW) words in flight.  The loads carry no predicate -- a predicated load sits in a branch of its
    // own, and the compiler waits for it there: a lane past the end of the slice reads the slice's last word, a
    // partition past nparts reads partition 0 (both in bounds, both discarded), and the predicate selects afterwards.
    double ta[NPART][NA], te[NPART][NE], tw[NPART][NW];
#pragma unroll
    for (int k = 0; k < NPART; ++k) {
      const size_t row0 = (size_t)(k < nparts ? k : 0) * n_cams + c0;
      if (FINALIZE) {
        const double* pa = partL + row0 * NL;
#pragma unroll
        for (int j = 0; j < NA; ++j) ta[k][j] = pa[min(j * 64 + lane, la - 1)];
      }
      const double* pw = part6 + row0 * NB;
#pragma unroll
      for (int j = 0; j < NW; ++j) tw[k][j] = pw[min(j * 64 + lane, lw - 1)];
    }
    if (use_schur_diag == 1) {
#pragma unroll
      for (int k = 0; k < NPART; ++k) {
        const double* pe = partE + ((size_t)(k < nparts ? k : 0) * n_cams + c0) * NH;
#pragma unroll
        for (int j = 0; j < NE; ++j) te[k][j] = pe[min(j * 64 + lane, le - 1)];
      }
    }
#pragma unroll
    for (int k = 0; k < NPART; ++k) {
#pragma unroll
      for (int j = 0; j < NA; ++j) ta[k][j] = (FINALIZE && k < nparts && j * 64 + lane < la) ? ta[k][j] : 0.0;
#pragma unroll
      for (int j = 0; j < NE; ++j) te[k][j] = (use_schur_diag == 1 && k < nparts && j * 64 + lane < le) ? te[k][j] : 0.0;
#pragma unroll
      for (int j = 0; j < NW; ++j) tw[k][j] = (k < nparts && j * 64 + lane < lw) ? tw[k][j] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < NPART; ++k) {                  // k = 0, 1, ... into a zero, in every element
#pragma unroll
      for (int j = 0; j < NA; ++j) sa[j] += ta[k][j];
#pragma unroll
      for (int j = 0; j < NE; ++j) se[j] += te[k][j];
#pragma unroll
      for (int j = 0; j < NW; ++j) sw[j] += tw[k][j];
    }
#pragma unroll
    for (int j = 0; j < NA; ++j) { const int i = j * 64 + lane; if (i < NL * VC) l_a[i] = sa[j]; }
#pragma unroll
    for (int j = 0; j < NE; ++j) { const int i = j * 64 + lane; if (i < NH * VC) l_e[i] = se[j]; }
#pragma unroll
    for (int j = 0; j < NW; ++j) { const int i = j * 64 + lane; if (i < NB * VC) l_w6[i] = sw[j]; }
    slice_store_lds(l_cs, CS * VC, vc);
    if (!FINALIZE) {
      slice_store_lds(l_hcc, NH * VC, vh);
      slice_store_lds(l_bc, NB * VC, vb);
    }
  }
  BA_STAMP(3, 2);
  __syncthreads();
  double acc[2] = {0, 0};
  double gmc = 0.0;
  const int t = threadIdx.x;
  if (c < n_cams) {
    const double* M = l_cs + CS * t + 12;
    const bool fixed = c == fixed_cam;
    const unsigned held = cam_held_bits(cam_held, c);
    if (FINALIZE) lin_finalize_sums<NB>(l_a + NL * t, M, fixed, l_hcc + NH * t, l_bc + NB * t, held, &pr, c);
    double h[NH], m[NH], inv[NH];
    for (int q = 0; q < NH; ++q) h[q] = l_hcc[NH * t + q];
    if (fixed) {
      for (int q = 0; q < NH; ++q) h[q] = 0.0;
      for (int i = 0; i < NB; ++i) h[UT(NB, i, i)] = 1.0;
    } else {
      for (int i = 0; i < NB; ++i) h[UT(NB, i, i)] += lambda * fmax(h[UT(NB, i, i)], DIAG_FLOOR);
      if (held) held_identity<NB>(held, h);
    }
    for (int q = 0; q < NH; ++q) { l_hd[NH * t + q] = h[q]; m[q] = h[q]; }
    if (use_schur_diag == 2) {
      for (int q = 0; q < NH; ++q) inv[q] = l_mi[NH * t + q];
    } else {
      if (use_schur_diag && !fixed) {
        double A[NB][NB];
        for (int i = 0; i < NB; ++i) for (int j = 0; j < NB; ++j) A[i][j] = l_e[NH * t + ST(NB, i, j)];
        m_congruence<NB>(M, A);
        for (int i = 0; i < NB; ++i) for (int j = i; j < NB; ++j) m[UT(NB, i, j)] -= A[i][j];
        if (held) held_identity<NB>(held, m);
      }
      // member of a group (shared intrinsics): the pose block alone is inverted -- coupling 0 and an identity in the 3 x 3
      // corner, which the Cholesky factors keep apart -- and the corner's own entries go out in its place for the group sum
      double m3[6];
      bool grouped = false;
      if constexpr (NB > 6) {
        grouped = cam_gl && cam_gl[c] >= 0;
        if (grouped) {
          for (int i = 0; i < 3; ++i) for (int j = i; j < 3; ++j) { m3[U3(i, j)] = m[UT(NB, 6 + i, 6 + j)]; m[UT(NB, 6 + i, 6 + j)] = (i == j) ? 1.0 : 0.0; }
          for (int i = 0; i < 6; ++i) for (int j = 6; j < NB; ++j) m[UT(NB, i, j)] = 0.0;
        }
      }
      spdN_inverse<NB>(m, inv);
      if constexpr (NB > 6) {
        if (grouped) {
          for (int i = 0; i < 3; ++i) for (int j = i; j < 3; ++j) inv[UT(NB, 6 + i, 6 + j)] = m3[U3(i, j)];
          for (int i = 0; i < 6; ++i) for (int j = 6; j < NB; ++j) inv[UT(NB, i, j)] = 0.0;
        }
      }
      for (int q = 0; q < NH; ++q) l_mi[NH * t + q] = inv[q];
    }
    double wy[NB], g[NB], zz[NB], hz[NB];
    {
      const double* a = l_w6 + NB * t;
      wy[0] = M[0] * a[0] + M[3] * a[1] + M[6] * a[2];
      wy[1] = M[1] * a[0] + M[4] * a[1] + M[7] * a[2];
      wy[2] = M[2] * a[0] + M[5] * a[1] + M[8] * a[2];
      for (int q = 3; q < NB; ++q) wy[q] = a[q];
    }
    for (int q = 0; q < NB; ++q) g[q] = (fixed || ((held >> q) & 1u)) ? 0.0 : -(l_bc[NB * t + q] - wy[q]);
    for (int q = 0; q < NB; ++q) gmc = nanmax(gmc, fabs(l_bc[NB * t + q]));     // max |bc| (gtol test)
    symN_mul<NB>(inv, g, zz);
    symN_mul<NB>(h, zz, hz);
    for (int q = 0; q < NB; ++q) {
      l_g[NB * t + q] = g[q];
      l_z[NB * t + q] = zz[q];
      acc[0] += g[q] * zz[q];
      acc[1] += zz[q] * hz[q];
    }
    write_vtil<NB>(M, zz, vtil + CM::TA * (size_t)c + CM::VOFF);
  }
  BA_STAMP(3, 3);
  __syncthreads();
  // ---- coalesced write-back
  {
    double2 wh[slice_chunks(NH * VC)], wb[slice_chunks(NB * VC)], wd[slice_chunks(NH * VC)], wm[slice_chunks(NH * VC)],
        wg[slice_chunks(NB * VC)], wz[slice_chunks(NB * VC)];
    if (FINALIZE) {
      slice_load_lds(l_hcc, NH * VC, wh);
      slice_load_lds(l_bc, NB * VC, wb);
    }
    slice_load_lds(l_hd, NH * VC, wd);
    slice_load_lds(l_mi, NH * VC, wm);
    slice_load_lds(l_g, NB * VC, wg);
    slice_load_lds(l_z, NB * VC, wz);
    if (FINALIZE) {
      slice_store(Hcc + NH * (size_t)c0, NH * nc, wh);
      slice_store(bc + NB * (size_t)c0, NB * nc, wb);
    }
    slice_store(Hccd + NH * (size_t)c0, NH * nc, wd);
    if (use_schur_diag != 2) slice_store(Minv + NH * (size_t)c0, NH * nc, wm);
    slice_store(gvec + NB * (size_t)c0, NB * nc, wg);
    slice_store(r + NB * (size_t)c0, NB * nc, wg);
    slice_store(z + NB * (size_t)c0, NB * nc, wz);
  }
  for (int i = lane; i < NB * nc; i += 64) {
    x[NB * (size_t)c0 + i] = 0.0; p[NB * (size_t)c0 + i] = 0.0; s[NB * (size_t)c0 + i] = 0.0;
    vx[NB * (size_t)c0 + i] = 0.0;                       // the iterate in the point passes' form (see k_pcg_step)
  }
#pragma unroll
  for (int q = 0; q < 2; ++q) acc[q] = wave_total_dpp(acc[q]);
  gmc = wave_nanmax(gmc);
  if (threadIdx.x == 0) {
    partV[2 * blockIdx.x] = acc[0];
    partV[2 * blockIdx.x + 1] = acc[1];
    partGc[blockIdx.x] = gmc;
    if (blockIdx.x == 0) {
      PcgState s0 = {0.0, 0.0, 0.0, 0.0, 0, 0, 0, 0};
      st[0] = s0;
      st[1] = s0;
    }
  }
  BA_STAMP(3, 6); BA_STAMP(3, 7);
}

// ---- shared intrinsics (ba_set_shared_intrinsics) ----------------------------------------------------------------
// Cameras of a group share ONE f, k1, k2: with x = E y (E replicates a group's three entries into rows 6-8 of every
// member) the damped reduced system is (E^T S E) y = E^T g.  Every PCG vector stays in its (Nc, 9) array in replicated
// form -- rows 6-8 of every member hold the group's value, bit for bit -- so no observation-loop kernel changes.  What
// changes is the camera-vector stage: rows 6-8 of the product, of the right-hand side and of the preconditioner's
// 3 x 3 block are SUMS over a group's members (these kernels), and inner products count a shared entry once, at the
// group's leader (its lowest member).  cam_gl[c] = -1: camera c has its own intrinsics, else 2 * group + (1: leader).
// Member lists: CSR (grp_off, grp_mem), members ascending.  Every sum below runs in one fixed order -- a thread's
// members ascending, then the lanes of a wave, then the waves -- over all-reduced inputs: every rank gets the same bits.
constexpr int SHARED_BLOCK = 256;        // threads of a group's reducing workgroup (groups of any size: members are strided)
constexpr int SHARED_REC = 16;           // doubles per group of k_shared_sum's record: inv3[6] | g3[3] | z3[3] | max |bc3| | pad
template <int N>
__device__ inline void shared_block_sum(double (&a)[N], double* __restrict__ lds) {   // lds: N * SHARED_BLOCK / 64 doubles; total in every thread
  constexpr int NW = SHARED_BLOCK / 64;
  const int wv = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < N; ++q) a[q] = wave_total_dpp(a[q]);
  if ((threadIdx.x & 63) == 0)
    for (int q = 0; q < N; ++q) lds[N * wv + q] = a[q];
  __syncthreads();
#pragma unroll
  for (int q = 0; q < N; ++q) {
    double t = lds[q];
    for (int w = 1; w < NW; ++w) t += lds[N * w + q];
    a[q] = t;
  }
}
// Once per damped system, behind k_pcg_setup (one workgroup per group): sum of the members' 3 x 3 preconditioner entries
// (k_pcg_setup left them in Minv's corner; keep: the blocks are kept, the corner already holds the group's inverse), of
// rows 6-8 of g and of bc; then the group's inverse, g and z = inverse g into the group's record.
template <class CM>
__global__ void __launch_bounds__(SHARED_BLOCK)
k_shared_sum(const int* __restrict__ grp_off, const int* __restrict__ grp_mem, int keep, const double* __restrict__ Minv,
             const double* __restrict__ gvec, const double* __restrict__ bc, double* __restrict__ rec) {
  constexpr int NB = CM::NB, NH = CM::NH;
  static_assert(NB == 9, "shared intrinsics: rows 6-8 of a 9-parameter camera block");
  __shared__ double lds[12 * SHARED_BLOCK / 64];
  const int g = blockIdx.x;
  const int beg = grp_off[g], end = grp_off[g + 1];
  double a[12];
#pragma unroll
  for (int q = 0; q < 12; ++q) a[q] = 0.0;
  for (int i = beg + (int)threadIdx.x; i < end; i += SHARED_BLOCK) {
    const int c = grp_mem[i];
    if (!keep) {
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int j = r; j < 3; ++j) a[U3(r, j)] += Minv[NH * (size_t)c + UT(NB, 6 + r, 6 + j)];
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) { a[6 + q] += gvec[NB * (size_t)c + 6 + q]; a[9 + q] += bc[NB * (size_t)c + 6 + q]; }
  }
  shared_block_sum<12>(a, lds);
  if (threadIdx.x == 0) {
    double inv[6], z3[3];
    if (keep) {
      const int lead = grp_mem[beg];
      for (int r = 0; r < 3; ++r) for (int j = r; j < 3; ++j) inv[U3(r, j)] = Minv[NH * (size_t)lead + UT(NB, 6 + r, 6 + j)];
    } else spdN_inverse<3>(a, inv);
    sym3_mul(inv, a + 6, z3);
    double* o = rec + SHARED_REC * (size_t)g;
    for (int q = 0; q < 6; ++q) o[q] = inv[q];
    for (int q = 0; q < 3; ++q) { o[6 + q] = a[6 + q]; o[9 + q] = z3[q]; }
    o[12] = nanmax(nanmax(fabs(a[9]), fabs(a[10])), fabs(a[11]));
  }
}
// ... and behind that, in k_pcg_setup's geometry: the members' rows 6-8 of g = r, z, vtil and (unless kept) the corner of
// Minv take the group's values, and the workgroup's partials are written again with the leader rule: gamma = r.z counts a
// shared entry once, zeta = z.Hccd z is the expanded operator's quadratic form (a full sum), max |bc| sees the group sum.
template <class CM>
__global__ void __launch_bounds__(VEC_BLOCK)
k_shared_finish(const int* __restrict__ cam_gl, const double* __restrict__ rec, int keep, int n_cams, const double* __restrict__ Hccd,
                const double* __restrict__ bc, double* __restrict__ Minv, double* __restrict__ gvec, double* __restrict__ r,
                double* __restrict__ z, double* __restrict__ vtil, double* __restrict__ partV, double* __restrict__ partGc) {
  constexpr int NB = CM::NB, NH = CM::NH, VC = CM::VC;
  const int c = vec_camera<VC>(n_cams);
  double acc[2] = {0, 0};
  double gmc = 0.0;
  if (c < n_cams) {
    const int gl = cam_gl[c];
    double g[NB], zz[NB], hz[NB];
#pragma unroll
    for (int q = 0; q < NB; ++q) { g[q] = gvec[NB * (size_t)c + q]; zz[q] = z[NB * (size_t)c + q]; }
    if (gl >= 0) {
      const double* o = rec + SHARED_REC * (size_t)(gl >> 1);
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        g[6 + q] = o[6 + q]; zz[6 + q] = o[9 + q];
        gvec[NB * (size_t)c + 6 + q] = g[6 + q]; r[NB * (size_t)c + 6 + q] = g[6 + q]; z[NB * (size_t)c + 6 + q] = zz[6 + q];
        vtil[CM::TA * (size_t)c + CM::VOFF + 6 + q] = zz[6 + q];        // (write_vtil passes rows 3.. through)
      }
      if (!keep)
        for (int i = 0; i < 3; ++i) for (int j = i; j < 3; ++j) Minv[NH * (size_t)c + UT(NB, 6 + i, 6 + j)] = o[U3(i, j)];
      gmc = (gl & 1) ? o[12] : 0.0;
    }
    symN_mul<NB>(Hccd + NH * (size_t)c, zz, hz);
#pragma unroll
    for (int q = 0; q < NB; ++q) {
      const bool once = q < 6 || gl < 0 || (gl & 1);
      if (once) acc[0] += g[q] * zz[q];
      acc[1] += zz[q] * hz[q];
      if (q < 6 || gl < 0) gmc = nanmax(gmc, fabs(bc[NB * (size_t)c + q]));
    }
  }
#pragma unroll
  for (int q = 0; q < 2; ++q) acc[q] = wave_total_dpp(acc[q]);
  gmc = wave_nanmax(gmc);
  if (threadIdx.x == 0) {
    partV[2 * blockIdx.x] = acc[0];
    partV[2 * blockIdx.x + 1] = acc[1];
    partGc[blockIdx.x] = gmc;
  }
}
// Once per PCG iteration, between k_cam_schur (and the all-reduce of a multi-rank job) and k_pcg_step: rows 6-8 of
// w_c = Hccd_c z_c - (W y)_c summed over a group's members.  A group is cut into chunks of SHARED_BLOCK consecutive members
// (chunk_rng[2 k], [2 k + 1]: the chunk's range in grp_mem; a group's chunks are consecutive: grp_chunk[g] .. grp_chunk[g + 1]),
// one workgroup and one member per thread each, so that a group of every camera is spread over the chip instead of
// walked by one workgroup; k_pcg_step adds a group's chunk sums in chunk order for rows 6-8 of every member's w.
template <class CM>
__global__ void __launch_bounds__(SHARED_BLOCK)
k_shared_fold(const int* __restrict__ chunk_rng, const int* __restrict__ grp_mem, const double* __restrict__ Hccd,
              const double* __restrict__ z, const double* __restrict__ part6, int nparts, int n_cams, double* __restrict__ gw) {
  constexpr int NB = CM::NB, NH = CM::NH;
  static_assert(NB == 9, "shared intrinsics: rows 6-8 of a 9-parameter camera block");
  __shared__ double lds[3 * SHARED_BLOCK / 64];
  const int g = blockIdx.x;
  const int beg = chunk_rng[2 * g], end = chunk_rng[2 * g + 1];
  const size_t p6_stride = (size_t)n_cams * NB;
  double a[3] = {0, 0, 0};
  for (int i = beg + (int)threadIdx.x; i < end; i += SHARED_BLOCK) {      // (one pass: a chunk has at most SHARED_BLOCK members)
    const int c = grp_mem[i];
    double zz[NB], wy[3] = {0, 0, 0};
#pragma unroll
    for (int q = 0; q < NB; ++q) zz[q] = z[NB * (size_t)c + q];
    for (int kk = 0; kk < nparts; ++kk) {
#pragma unroll
      for (int q = 0; q < 3; ++q) wy[q] += part6[(size_t)kk * p6_stride + NB * (size_t)c + 6 + q];
    }
    const double* h = Hccd + NH * (size_t)c;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      double t = 0;
#pragma unroll
      for (int j = 0; j < NB; ++j) t += h[ST(NB, 6 + q, j)] * zz[j];
      a[q] += t - wy[q];
    }
  }
  shared_block_sum<3>(a, lds);
  if (threadIdx.x < 3) gw[3 * (size_t)g + threadIdx.x] = a[threadIdx.x];
}

// K5: one PCG iteration's vector work (Chronopoulos-Gear single-reduction CG).  With z the
// preconditioned residual and w = S z:
//   gamma = r.z (partials of the previous step), delta = z.Hccd z - u.y,
//   beta = gamma/gamma_prev, alpha = gamma / (delta - beta gamma / alpha_prev),
//   p = z + beta p, s = w + beta s, x += alpha p, r -= alpha s, z = Minv r.
// Every workgroup recomputes the scalars from the same words; workgroup 0 publishes the
// next state into the other parity slot.  uy_src: the u.y word (folded by k_cam_schur's
// extra workgroup, or all-reduced in a multi-rank job).
// SHARED (shared intrinsics, BalCam only): an instantiation of its own, so that the ungrouped kernel keeps its registers
// (248 VGPRs, two waves per SIMD; the three extra pointers and the group index cost the grouped one the second wave).
template <class CM, bool SHARED = false>
__global__ void __launch_bounds__(VEC_BLOCK)
k_pcg_step(int k, const double* __restrict__ part6, int nparts, const double* __restrict__ uy_src,
           const double* __restrict__ Hccd, const double* __restrict__ Minv, const double* __restrict__ cs,
           int n_cams, int fixed_cam, double tol2, int min_iters,
           double* __restrict__ x, double* __restrict__ r, double* __restrict__ p, double* __restrict__ s,
           double* __restrict__ z, double* __restrict__ vtil, double* __restrict__ partV, int nblkV,
           PcgState* __restrict__ st, long long* __restrict__ host_flag, long long flag_base,
           const double* __restrict__ verdict, double* __restrict__ vx,
           double model_tol, int model_min_iters, IpcStep ipc, long long* __restrict__ err_flag,
           const unsigned short* __restrict__ cam_held, const int* __restrict__ cam_gl, const double* __restrict__ gw,
           const int* __restrict__ grp_chunk) {
  // cam_gl / gw / grp_chunk (shared intrinsics, null = none): rows 6-8 of a grouped camera's w are k_shared_fold's sums
  // ipc.on (multi-rank, device-side exchange): part6 / uy_src are this rank's own sums; the other ranks' arrive in the
  // receive buffer while the kernel runs (see "device-side all-reduce" above)
  constexpr int NB = CM::NB, NH = CM::NH, VC = CM::VC;
  static_assert(VEC_BLOCK == 64, "the in-kernel exchange fences and flags from ONE wave");
  // LDS image of the workgroup's cameras: Hccd | Minv | z p s r x | part6[NPART] | cs
  __shared__ double l_h[NH * VC], l_mi[NH * VC], l_v[5][NB * VC], l_p6[NPART][NB * VC], l_cs[CS * VC];
  BA_STAMP(2, 0); BA_STAMP(2, 1);
  const int c0 = blockIdx.x * VC;
  const int nc = min(VC, n_cams - c0);                         // cameras of this workgroup (>= 1)
  const int c = vec_camera<VC>(n_cams);
  const bool live = c < n_cams && c != fixed_cam;
  // every operand is fetched before the verdict is known (one round trip for the whole kernel; an
  // early-exit launch wastes the loads)
  double uy = uy_src[0];
  {
    double2 vh[slice_chunks(NH * VC)], vm[slice_chunks(NH * VC)], vv[5][slice_chunks(NB * VC)], vp[NPART][slice_chunks(NB * VC)],
        vc[slice_chunks(CS * VC)];
    slice_load(VecSlice{Hccd + NH * (size_t)c0, NH * nc}, vh);
    slice_load(VecSlice{Minv + NH * (size_t)c0, NH * nc}, vm);
    const double* vecs[5] = {z, p, s, r, x};
#pragma unroll
    for (int q = 0; q < 5; ++q) slice_load(VecSlice{vecs[q] + NB * (size_t)c0, NB * nc}, vv[q]);
    slice_load(VecSlice{cs + CS * (size_t)c0, CS * nc}, vc);
    const size_t p6_stride = (size_t)n_cams * NB;           // partition stride of the Schur product's partial sums
#pragma unroll
    for (int kk = 0; kk < NPART; ++kk)
      slice_load(VecSlice{part6 + (size_t)kk * p6_stride + (size_t)c0 * NB, kk < nparts ? NB * nc : 0}, vp[kk]);
    slice_store_lds(l_h, NH * VC, vh);
    slice_store_lds(l_mi, NH * VC, vm);
#pragma unroll
    for (int q = 0; q < 5; ++q) slice_store_lds(l_v[q], NB * VC, vv[q]);
#pragma unroll
    for (int kk = 0; kk < NPART; ++kk) slice_store_lds(l_p6[kk], NB * VC, vp[kk]);
    slice_store_lds(l_cs, CS * VC, vc);
  }
  double gamma, zeta;
  const bool fin = pcg_verdict(verdict, k, gamma, zeta);     // left by the point pass of this iteration
  const PcgState sin = st[k & 1];
  PcgState* sout = st + ((k + 1) & 1);
  if (fin) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      PcgState o = sin;
      if (!o.done) { o.done = 1; o.iters = k; if (k == 0) o.gamma0 = gamma; }
      *sout = o;
      publish_flag(host_flag, flag_base + k + 1, o.iters + 1);
    }
    return;
  }
  BA_STAMP(2, 2);
  int nfold = nparts;                                   // partitions the per-camera fold below adds
  if (ipc.on) {
    __syncthreads();                                    // the LDS image (the partitions) is complete
    constexpr int REC = 2 + NB * VC;
    const int lane = threadIdx.x;
    const size_t mine = ((size_t)ipc.parity * ipc.world + ipc.rank) * ipc.stride + (size_t)blockIdx.x * REC;
    for (int e = lane; e < NB * VC; e += 64) {
      double a = 0.0;
      for (int kk = 0; kk < nparts; ++kk) a += l_p6[kk][e];
      for (int d = 0; d < ipc.world; ++d) __hip_atomic_store(ipc.P.recv[d] + mine + 2 + e, a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (lane < ipc.world) __hip_atomic_store(ipc.P.recv[lane] + mine, uy, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    // every store of this workgroup (one wave) has left for the fabric before the sequence number follows it (release,
    // system scope); the barrier orders the OTHER lanes' fenced stores before the lanes that publish
    __threadfence_system();
    __syncthreads();
    if (lane < ipc.world)
      __hip_atomic_store(ipc.P.flags[lane] + ((size_t)ipc.parity * ipc.world + ipc.rank) * IPC_MAX_BLOCKS + blockIdx.x,
                         (unsigned long long)ipc.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    if (!ipc_wait(ipc.P.flags[ipc.rank], ipc.world, ipc.parity, (int)blockIdx.x, ipc.seq) && err_flag && lane == 0)
      __hip_atomic_store(err_flag, 2ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    const double* own = ipc.P.recv[ipc.rank] + (size_t)ipc.parity * ipc.world * ipc.stride + (size_t)blockIdx.x * REC;
    uy = 0.0;
    for (int sdr = 0; sdr < ipc.world; ++sdr)           // the senders' records, rank order
      uy += __hip_atomic_load(own + (size_t)sdr * ipc.stride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    for (int e = lane; e < NB * VC; e += 64) {
      double a = 0.0;
      for (int sdr = 0; sdr < ipc.world; ++sdr)
        a += __hip_atomic_load(own + (size_t)sdr * ipc.stride + 2 + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      l_p6[0][e] = a;
    }
    nfold = 1;
  }
  const double delta = zeta - uy;
  const double beta = (k == 0) ? 0.0 : gamma / sin.gamma_prev;
  const double denom = (k == 0) ? delta : delta - beta * gamma / sin.alpha_prev;
  if (!(denom > 0.0) || !isfinite(denom)) {           // breakdown: keep x, stop
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      PcgState o = sin;
      o.done = 2; o.iters = k; if (k == 0) o.gamma0 = gamma;
      *sout = o;
      publish_flag(host_flag, flag_base + k + 1, k + 1);
    }
    return;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) publish_flag(host_flag, flag_base + k + 1, 0);   // verdict: keep going
  const double alpha = gamma / denom;
  __syncthreads();                                      // the LDS image is complete
  double acc[2] = {0, 0};
  const int t = threadIdx.x;
  if (live) {
    const double* M = l_cs + CS * t + 12;
    // pinhole: both blocks into registers once (42 words).  A 9-parameter camera's 90 words would fill the register file
    // (256 VGPRs + spills into AGPRs): its products read the blocks from LDS where they are
    double hreg[NB == 6 ? NH : 1], mireg[NB == 6 ? NH : 1];
    const double *h = l_h + NH * t, *mi = l_mi + NH * t;
    if (NB == 6) {
#pragma unroll
      for (int q = 0; q < NH; ++q) { hreg[q] = l_h[NH * t + q]; mireg[q] = l_mi[NH * t + q]; }
      h = hreg; mi = mireg;
    }
    double zz[NB], wy[NB], pp[NB], ss[NB], rr[NB], xx[NB], w[NB], hz[NB];
    {
      double a[NB];
#pragma unroll
      for (int q = 0; q < NB; ++q) a[q] = 0.0;
      for (int kk = 0; kk < nfold; ++kk) {
#pragma unroll
        for (int q = 0; q < NB; ++q) a[q] += l_p6[kk][NB * t + q];
      }
      wy[0] = M[0] * a[0] + M[3] * a[1] + M[6] * a[2];
      wy[1] = M[1] * a[0] + M[4] * a[1] + M[7] * a[2];
      wy[2] = M[2] * a[0] + M[5] * a[1] + M[8] * a[2];
#pragma unroll
      for (int q = 3; q < NB; ++q) wy[q] = a[q];
    }
#pragma unroll
    for (int q = 0; q < NB; ++q) {
      zz[q] = l_v[0][NB * t + q]; pp[q] = l_v[1][NB * t + q]; ss[q] = l_v[2][NB * t + q];
      rr[q] = l_v[3][NB * t + q]; xx[q] = l_v[4][NB * t + q];
    }
    symN_mul<NB>(h, zz, w);
    const unsigned held = cam_held_bits(cam_held, c);      // held rows of S: identity, so that r, z, p, s, x stay 0 there
    int gl = -1;
    if constexpr (SHARED) {
      gl = cam_gl[c];
      if (gl >= 0) {                                       // E^T S E: the group's sum, the same bits in every member
#pragma unroll
        for (int q = 6; q < NB; ++q) { w[q] = 0.0; wy[q] = 0.0; }
        for (int ch = grp_chunk[gl >> 1]; ch < grp_chunk[(gl >> 1) + 1]; ++ch) {      // chunk order: the same sum in every member
#pragma unroll
          for (int q = 6; q < NB; ++q) w[q] += gw[3 * (size_t)ch + (q - 6)];
        }
      }
    }
#pragma unroll
    for (int q = 0; q < NB; ++q) {
      w[q] = ((held >> q) & 1u) ? 0.0 : w[q] - wy[q];
      pp[q] = zz[q] + beta * pp[q];
      ss[q] = w[q] + beta * ss[q];
      xx[q] = xx[q] + alpha * pp[q];
      rr[q] -= alpha * ss[q];
    }
    symN_mul<NB>(mi, rr, zz);
    symN_mul<NB>(h, zz, hz);
#pragma unroll
    for (int q = 0; q < NB; ++q) {
      l_v[0][NB * t + q] = zz[q]; l_v[1][NB * t + q] = pp[q]; l_v[2][NB * t + q] = ss[q];
      l_v[3][NB * t + q] = rr[q]; l_v[4][NB * t + q] = xx[q];
      if (!SHARED || q < 6 || gl < 0 || (gl & 1)) acc[0] += rr[q] * zz[q];       // (a shared entry counts once, at the group's leader)
      acc[1] += zz[q] * hz[q];
    }
    write_vtil<NB>(M, zz, vtil + CM::TA * (size_t)c + CM::VOFF);
    // the iterate itself in the point passes' form, (M x_r, x_t, ..): what the back substitution multiplies with once PCG
    // has stopped -- kept current here so that no kernel has to run between the last PCG iteration and the step
    write_vtil<NB>(M, xx, vx + NB * (size_t)c);
  }
  __syncthreads();
  {                                                     // the five vectors back, coalesced (fixed camera: unchanged image)
    double* vecs[5] = {z, p, s, r, x};
#pragma unroll
    for (int q = 0; q < 5; ++q) slice_write_back(vecs[q] + NB * (size_t)c0, l_v[q], NB * nc);
  }
  BA_STAMP(2, 3);
#pragma unroll
  for (int q = 0; q < 2; ++q) acc[q] = wave_total_dpp(acc[q]);
  if (threadIdx.x == 0) {
    double* pv = partV + (size_t)((k + 1) & 1) * 2 * nblkV;
    pv[2 * blockIdx.x] = acc[0];
    pv[2 * blockIdx.x + 1] = acc[1];
    if (blockIdx.x == 0) {
      PcgState o = sin;
      o.gamma_prev = gamma; o.alpha_prev = alpha;
      o.gamma0 = (k == 0) ? gamma : sin.gamma0;
      o.iters = k + 1;
      // model test (Nash & Sofer): this iteration lowered q by 1/2 alpha gamma; stop when (k + 1) times that is no more
      // than model_tol of the whole decrease so far
      const double dq = 0.5 * alpha * gamma;
      o.q_tot = ((k == 0) ? 0.0 : sin.q_tot) + dq;
      o.stop_model = (model_tol > 0.0 && k + 1 >= model_min_iters && (double)(k + 1) * dq <= model_tol * o.q_tot) ? 1 : 0;
      *sout = o;
    }
  }
  BA_STAMP(2, 6); BA_STAMP(2, 7);
}

// K7a: camera update.  cams_trial = cams + dc (BAL: also intr_trial = intr + the last three entries of dc), camera
// state and table row of the trial cameras, vtil = (M dc_r, dc_t, ..) into camA for the back substitution,
// camera-side scalars -> partC[block][5]: bc.dc, sum Dc dc^2, dc.r_pcg, |dc|^2, |cams|^2
// Body for camera group `blk` (VC cameras), run by ONE wave (`active`: this wave has a group); every thread of the
// workgroup passes the barriers (the body also runs inside 1024-thread workgroups of the back-substitution launch, one
// group per wave for the first CU_GROUPS waves, see "riders").  lds: this wave's cam_update_lds_doubles<CM>() doubles
// of LDS, 16-byte aligned.
template <class CM>
__device__ void cam_update_body(const CamUpdateArgs& a, int blk, bool active, double* __restrict__ lds) {
  constexpr int NB = CM::NB, NH = CM::NH, VC = CM::VC;
  // LDS image of the workgroup's VC cameras (coalesced staging, see slice_load): cams | dc rpcg bc | Hcc | cs,
  // outputs cams_trial | cs_trial staged for a coalesced write-back
  double* l_cam = lds;
  double* l_in = l_cam + 6 * VC;              // [3][NB * VC]
  double* l_hcc = l_in + 3 * NB * VC;
  double* l_cs = l_hcc + NH * VC;
  double* l_ct = l_cs + CS * VC;
  double* l_cst = l_ct + 6 * VC;
  const int n_cams = a.n_cams, fixed_cam = a.fixed_cam;
  const bool w0 = active;
  const int lane = threadIdx.x & 63;
  const int c0 = blk * VC;
  const int nc = min(VC, n_cams - c0);
  const int c = (lane < VC) ? c0 + lane : n_cams;
  if (w0) {
    double2 v0[slice_chunks(6 * VC)], vi[3][slice_chunks(NB * VC)], vh[slice_chunks(NH * VC)], vc[slice_chunks(CS * VC)];
    const double* ins[3] = {a.dc, a.rpcg, a.bc};
    slice_load(VecSlice{a.cams + 6 * (size_t)c0, 6 * nc}, v0);
#pragma unroll
    for (int q = 0; q < 3; ++q) slice_load(VecSlice{ins[q] + NB * (size_t)c0, NB * nc}, vi[q]);
    slice_load(VecSlice{a.Hcc + NH * (size_t)c0, NH * nc}, vh);
    slice_load(VecSlice{a.cs + CS * (size_t)c0, CS * nc}, vc);
    slice_store_lds(l_cam, 6 * VC, v0);
#pragma unroll
    for (int q = 0; q < 3; ++q) slice_store_lds(l_in + q * NB * VC, NB * VC, vi[q]);
    slice_store_lds(l_hcc, NH * VC, vh);
    slice_store_lds(l_cs, CS * VC, vc);
  }
  __syncthreads();
  double acc[5] = {0, 0, 0, 0, 0};
  const int t = lane;
  if (w0 && c < n_cams) {
    double d[NB];
    for (int q = 0; q < NB; ++q) d[q] = (c == fixed_cam) ? 0.0 : l_in[NB * t + q];
    double it3[3] = {0.0, 0.0, 0.0};                   // trial intrinsics (models with per-camera intrinsics)
    const int gl = (NB > 6 && a.cam_gl) ? a.cam_gl[c] : -1;
    for (int q = 0; q < NB; ++q) {
      const double xq = q < 6 ? l_cam[6 * t + q] : a.intr[3 * (size_t)c + (q - 6)];
      if (q < 6) l_ct[6 * t + q] = xq + d[q];
      else it3[q - 6] = xq + d[q];
      acc[0] += l_in[2 * NB * VC + NB * t + q] * d[q];
      acc[1] += fmax(l_hcc[NH * t + UT(NB, q, q)], DIAG_FLOOR) * d[q] * d[q];
      if (q < 6 || gl < 0 || (gl & 1)) {               // (the y problem's sums: a shared entry once)
        acc[2] += d[q] * ((c == fixed_cam) ? 0.0 : l_in[NB * VC + NB * t + q]);
        acc[3] += d[q] * d[q];
        acc[4] += xq * xq;
      }
    }
    if (NB > 6) {
      for (int q = 0; q < NB - 6; ++q) a.intr_trial[3 * (size_t)c + q] = it3[q];
    }
    write_vtil<NB>(l_cs + CS * t + 12, d, a.vtil + CM::TA * (size_t)c + CM::VOFF);
    // The five sums and the trial intrinsics are not touched by camera_state, which alone fills the 128 registers of a
    // 1024-thread launch: kept live across it they were spilled to scratch, and a point-pass launch with riders had a
    // private segment for their sake.  They wait in this camera's own dc | rpcg rows instead, which nobody reads again.
    double* park = l_in + NB * t;
#pragma unroll
    for (int q = 0; q < 5; ++q) park[q] = acc[q];
    if (NB > 6) {
#pragma unroll
      for (int q = 0; q < 3; ++q) park[NB * VC + q] = it3[q];
    }
    camera_state(l_ct + 6 * t, l_cst + CS * t);
    if (NB > 6) {
#pragma unroll
      for (int q = 0; q < 3; ++q) it3[q] = park[NB * VC + q];
    }
    CM::table_row(l_cst + CS * t, it3, a.camA_trial + CM::TA * (size_t)c);
#pragma unroll
    for (int q = 0; q < 5; ++q) acc[q] = park[q];
  }
  __syncthreads();
  if (w0) {
    slice_write_back(a.cams_trial + 6 * (size_t)c0, l_ct, 6 * nc);
    slice_write_back(a.cs_trial + CS * (size_t)c0, l_cst, CS * nc);
#pragma unroll
    for (int q = 0; q < 5; ++q) acc[q] = wave_total_dpp(acc[q]);
    if (lane == 0) for (int q = 0; q < 5; ++q) a.partC[5 * blk + q] = acc[q];
  }
}
// stand-alone launch (camera windows that do not all fit in LDS, a rank without landmarks)
template <class CM>
__global__ void __launch_bounds__(VEC_BLOCK)
k_cam_update(CamUpdateArgs a) {
  __shared__ __align__(16) double lds[cam_update_lds_doubles<CM>()];
  cam_update_body<CM>(a, blockIdx.x, true, lds);
}
// the same as riding workgroup `rb` of a 1024-thread launch: waves 0 .. groups-1 take one camera group each
template <class CM>
__device__ __forceinline__ void cam_update_rider(const CamUpdateArgs& a, int rb, double* __restrict__ dyn_lds) {
  const int wv = threadIdx.x >> 6;
  const int grp = rb * a.groups + wv;
  const int n_groups = (a.n_cams + CM::VC - 1) / CM::VC;
  cam_update_body<CM>(a, grp, wv < a.groups && grp < n_groups, dyn_lds + (wv < a.groups ? wv : 0) * cam_update_lds_doubles<CM>());
}

// One workgroup folds every partial-sum array of an LM step into the scalar block `scal`
// (fixed order): residual partials (nR rows x 2), point partials (nB x 4, may be 0 rows),
// camera partials (nC x 5, may be 0 rows); with st != null also the PCG verdict for
// iteration `kit` (the test pcg_finished makes).  scal_host (nullable) is a host-mapped
// mirror written in the same kernel, so the host needs no copy, only the stream sync.
// The LM step's verdict, computed where its inputs are (one source of truth for host and device): gain ratio
// rho = (cost - cost_new) / model with the model decrease of the damped, inexactly solved system
// 0.5 (lambda d^T D d - g^T d + dc.r_pcg), and the damping an ACCEPTED step continues with (Nielsen's update).
// The host takes both from here; a speculated point-half linearisation at the trial point reads res[S_LAM_NEXT]
// from device memory before the host has decided anything.
// lam_floor: the damping is not allowed below it (cap-aware damping, ba_solve: three times the damping at which an inner
// solve last ran into pcg_max_iters; 0 = no floor)
__device__ inline void lm_decide(double* __restrict__ res, double cost_cur, double lambda, double lam_floor) {
  const double cost_new = 0.5 * res[S_RHO];
  const double gTd = res[S_PT_GD] + res[S_CAM_GD], dDd = res[S_PT_DDD] + res[S_CAM_DDD], dcr = res[S_DC_R];
  const double model = 0.5 * (lambda * dDd - gTd + dcr);
  const double rho = (model > 0.0 && isfinite(cost_new)) ? (cost_cur - cost_new) / model : -1.0;
  const double t = 2.0 * rho - 1.0;
  res[S_GAIN] = rho;
  res[S_LAM_NEXT] = fmax(fmax(lambda * fmax(1.0 / 3.0, 1.0 - t * t * t), 1e-12), lam_floor);
}
// multi-rank form: the scalars are all-reduced between k_scalars and the decision; like k_scalars on a single rank,
// the kernel mirrors the block into host-mapped memory and publishes the step's sequence word (one wave)
__global__ void __launch_bounds__(64)
k_decide(double* __restrict__ scal, const double* __restrict__ reduced6, double cost_cur, double lambda, double lam_floor,
         double* __restrict__ scal_host, long long* __restrict__ host_flag, long long seq) {
  __shared__ double res[S_COUNT];
  // (reduced6: the six all-reduced sums arrived in the header of another message, k_fold_lin)
  if (threadIdx.x < S_COUNT) res[threadIdx.x] = (reduced6 && threadIdx.x < 6) ? reduced6[threadIdx.x] : scal[threadIdx.x];
  __syncthreads();
  if (threadIdx.x == 0) lm_decide(res, cost_cur, lambda, lam_floor);
  __syncthreads();
  if (threadIdx.x < S_COUNT) {
    scal[threadIdx.x] = res[threadIdx.x];
    if (scal_host) scal_host[threadIdx.x] = res[threadIdx.x];
  }
  if (host_flag) {
    __threadfence_system();
    if (threadIdx.x == 0) publish_flag(host_flag, seq, 0);
  }
}

__device__ void scalars_body(const ScalarsArgs& a) {
  const double* __restrict__ partR = a.partR; const int nR = a.nR;
  const double* __restrict__ partB = a.partB; const int nB = a.nB;
  const double* __restrict__ partC = a.partC; const int nC = a.nC;
  const PcgState* __restrict__ st = a.st;
  __shared__ double sm[11 * 16];
  // PCG verdict first (wave 1, whole wave: pcg_finished sums across its lanes): its loads are in
  // flight while the partial sums below are read
  bool pcg_fin = false;
  double pcg_iters = 0.0;
  if ((threadIdx.x >> 6) == 1 && st) {
    double g, z;
    pcg_fin = pcg_finished(a.kit, st, a.partV, a.nblkV, a.tol2, a.min_iters, g, z);
    const PcgState& s = st[a.kit & 1];
    pcg_iters = s.done ? (double)s.iters : (double)a.kit;
  }
  double v[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = threadIdx.x; i < nR; i += 1024) { const double2 t = ((const double2*)partR)[i]; v[0] += t.x; v[1] += t.y; }
  for (int i = threadIdx.x; i < nB; i += 1024) {
    const double2 t0 = ((const double2*)partB)[2 * i], t1 = ((const double2*)partB)[2 * i + 1];
    v[2] += t0.x; v[3] += t0.y; v[4] += t1.x; v[5] += t1.y;
  }
  for (int i = threadIdx.x; i < nC; i += 1024) {
#pragma unroll
    for (int q = 0; q < 5; ++q) v[6 + q] += partC[5 * i + q];
  }
#pragma unroll
  for (int q = 0; q < 11; ++q) v[q] = wave_total_dpp(v[q]);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < 11; ++q) sm[wv * 11 + q] = v[q];
  }
  __syncthreads();
  __shared__ double res[S_COUNT];
  if (threadIdx.x < S_COUNT) res[threadIdx.x] = 0.0;
  __syncthreads();
  if (threadIdx.x < 11) {
    double t = 0;
    for (int w = 0; w < 16; ++w) t += sm[w * 11 + threadIdx.x];
    const int slot = threadIdx.x < 2 ? S_SSE + threadIdx.x : (threadIdx.x < 6 ? S_PT_GD + (threadIdx.x - 2) : S_CAM_GD + (threadIdx.x - 6));
    res[slot] = t;
  }
  if (wv == 1 && st && lane == 0) {
    res[S_PCG_FIN] = pcg_fin ? 1.0 : 0.0;
    res[S_PCG_ITERS] = pcg_iters;
  }
  __syncthreads();
  if (a.decide) {
    if (threadIdx.x == 0) lm_decide(res, a.cost_cur, a.lambda, a.lam_floor);
    __syncthreads();
  }
  if (threadIdx.x < S_COUNT) {
    a.scal[threadIdx.x] = res[threadIdx.x];
    if (a.scal_host) a.scal_host[threadIdx.x] = res[threadIdx.x];   // one wave: 24 consecutive host-mapped words
  }
  // rider mode: the point workgroups of this launch wait for the next damping and for nothing else of scal[] (what later
  // kernels read of it crosses a kernel boundary) -- one device-scope store of the value itself into the word they poll
  if (a.lam_slot && threadIdx.x == 0) __hip_atomic_store(a.lam_slot, res[S_LAM_NEXT], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  // one wave wrote every host word: the same wave fences and its lane 0 publishes the sequence number behind them
  if (threadIdx.x < 64) {
    if (a.host_flag) {
      __threadfence_system();
      if (threadIdx.x == 0) publish_flag(a.host_flag, a.seq, 0);
    }
  }
}
__global__ void __launch_bounds__(1024)
k_scalars(ScalarsArgs a) { scalars_body(a); }


// test hook (BA_DEBUG_POISON_TRIAL): makes the trial cost of every LM step non-finite
__global__ void k_poison(double* __restrict__ partR) {
  if (threadIdx.x == 0 && blockIdx.x == 0) { partR[0] = __builtin_nan(""); partR[1] = __builtin_nan(""); }
}

// Not-converged PCG state for the test / bench hooks that run one pass in isolation.
__global__ void k_pcg_reset(PcgState* __restrict__ st, double* __restrict__ partV, int nblkV) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    PcgState s0 = {1.0, 1.0, 1.0, 0.0, 0, 0, 0, 0};
    st[0] = s0; st[1] = s0;
    for (int b = 0; b < 4 * nblkV; ++b) partV[b] = (b & 1) ? 0.0 : 1.0;
  }
}

// out = Hccd v - Wy   (test hook behind ba_schur_system; the fixed camera's and held rows = identity)
template <class CM>
__global__ void k_schur_combine(const double* __restrict__ Hccd, const double* __restrict__ v,
                                const double* __restrict__ part6, int nparts, const double* __restrict__ cs,
                                int n_cams, int fixed_cam, double* __restrict__ out, const unsigned short* __restrict__ cam_held) {
  constexpr int NB = CM::NB, NH = CM::NH;
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_cams) return;
  double vv[NB], w[NB], a[NB], wy[NB];
  for (int q = 0; q < NB; ++q) { vv[q] = v[NB * (size_t)c + q]; a[q] = 0.0; }
  symN_mul<NB>(Hccd + NH * (size_t)c, vv, w);
  for (int k = 0; k < nparts; ++k)
    for (int q = 0; q < NB; ++q) a[q] += part6[((size_t)k * n_cams + c) * NB + q];
  const double* M = cs + CS * (size_t)c + 12;          // Wy = [M^T a_r ; a_t ; ..]
  wy[0] = M[0] * a[0] + M[3] * a[1] + M[6] * a[2];
  wy[1] = M[1] * a[0] + M[4] * a[1] + M[7] * a[2];
  wy[2] = M[2] * a[0] + M[5] * a[1] + M[8] * a[2];
  for (int q = 3; q < NB; ++q) wy[q] = a[q];
  const unsigned held = cam_held_bits(cam_held, c);
  for (int q = 0; q < NB; ++q) out[NB * (size_t)c + q] = (c == fixed_cam || ((held >> q) & 1u)) ? vv[q] : w[q] - wy[q];
}

// vt slot of camA for an arbitrary camera vector (test hook); held entries and the fixed camera enter as zero
template <class CM>
__global__ void k_vtil(const double* __restrict__ v, const double* __restrict__ cs, int n_cams, int fixed_cam,
                       double* __restrict__ vtil, const unsigned short* __restrict__ cam_held) {
  constexpr int NB = CM::NB;
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_cams) return;
  const unsigned held = cam_held_bits(cam_held, c);
  double d[NB];
  for (int q = 0; q < NB; ++q) d[q] = (c == fixed_cam || ((held >> q) & 1u)) ? 0.0 : v[NB * (size_t)c + q];
  write_vtil<NB>(cs + CS * (size_t)c + 12, d, vtil + CM::TA * (size_t)c + CM::VOFF);
}

}  // namespace ba
