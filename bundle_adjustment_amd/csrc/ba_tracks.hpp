// N-view triangulation and filtering of whole tracks (ba_triangulate_tracks): the modelling step next to the solve --
// adjust -> re-triangulate every track from the adjusted cameras -> filter by triangulation angle, depth and
// reprojection error -> adjust (COLMAP's Retriangulate / FilterPoints3D, the point culling of OpenMVG and ORB-SLAM).
// Stand-alone kernels: they read the handle's point-ordered observation list and camera state, and none of the
// LM / Schur / PCG kernels.
//
// Per track (every lane of the track's group holds the same sums, bit for bit, so every decision is group-uniform):
//   1 bearings   pinhole ((u - cx) / fx, (v - cy) / fy, 1); BAL: r_d = |uv| / f, r (1 + k1 r^2 + k2 r^4) = r_d solved for r by
//                Newton from r = r_d, ray (p0, p1, -1).  Both are written (x, y) with the ray (x, y, 1) up to sign: the BAL
//                pair is (-p0, -p1).  No convergence in NEWTON_ITERS steps or a derivative <= 0 on the way: DEGENERATE.
//   2 DLT        rows x (R2 X + t2) - (R0 X + t0), y (R2 X + t2) - (R1 X + t1) with X = Cm + X', Cm the mean camera centre of
//                the track's observations (keeps the digits of a far, low-parallax point); the ten fp64 sums of A^T A,
//                cyclic Jacobi on the 4 x 4, eigenvector of the smallest eigenvalue with w >= 0; |w| <= 1e-12 |X_h| or a
//                non-finite entry: DEGENERATE.
//   3 refinement Marquardt-damped Gauss-Newton on 0.5 sum C^2 rho((r / C)^2) over the scalar residuals, IRLS with the
//                solve's weights (robust_loss): (H + lam diag H) dx = -g by a 3 x 3 Cholesky (a pivot <= 0: DEGENERATE);
//                lam starts at 1e-4, a step that does not raise the cost is taken (lam / 10, floor 1e-12), any other
//                (a non-finite cost included) is dropped (lam * 10); either way it counts against refine_iters, and
//                |dx| <= 1e-14 |X| ends the iteration.  "Does not raise" allows for the rounding of the two sums:
//                cost_trial <= cost (1 + TRK_COST_SLACK).  A pixel of 640 carries 1.4e-13 of rounding, which a residual of
//                0.5 px turns into 3e-13 of its square; compared bit for bit, the last steps towards the stationary point
//                -- whose decrease is smaller than that -- are taken or dropped by chance, and the iteration stalls at a
//                gradient of 1e-5 on a flat track (measured: DESIGN.md 4h).
//   4 measures   at the final point, from the sums of the pass that was accepted: rms, the largest |r_i|, views with depth <=
//                min_depth; the largest angle over all pairs of views between the unit vectors u_i from the point to the
//                camera centres, found as the largest |u_i - u_j|^2 (monotone in the angle and exact for small ones, where
//                a cosine has no digits left) and turned into an angle once: 2 atan2(|u_i - u_j|, |u_i + u_j|).
//   5 status     the first failing test in enum order (ba_track_status).
// Two launch forms, the handle's own split of the tracks: TRK_G lanes per track for those of at most long_thr observations
// (DPP quad / half-row sums; the angle's inner loop reads the centres from the camera-centre table, which sits in L2), one
// wave per track of long_pts (DPP wave sums; the unit vectors of TRK_STAGE views at a time staged in LDS).
#pragma once
#include "ba_kernels.hpp"
#include "ba_linalg.hpp"

namespace ba {

enum : int { TRK_OK = 0, TRK_FEW_VIEWS = 1, TRK_DEGENERATE = 2, TRK_BEHIND = 3, TRK_LOW_ANGLE = 4, TRK_HIGH_ERROR = 5 };
constexpr int TRK_G = 8;            // lanes per short track
constexpr int TRK_THREADS = 256;    // threads per workgroup, short tracks
constexpr int TRK_OUT = 8;          // doubles per point slot: x y z | angle rms max | status | -
constexpr int TRK_STAGE = 512;      // unit vectors a wave stages in LDS at a time (12 KB)
constexpr int TRK_NEWTON_ITERS = 25;
constexpr double TRK_COST_SLACK = 1e-12;
constexpr int TRK_NSUM = 13;        // H (6) g (3) cost sse | max |r|^2 | views behind

struct TrackArgs {
  const double* cs;        // camera state, CS doubles per camera
  const double* intr;      // (f, k1, k2)[Nc] of the BAL camera, else null
  const double* ctr;       // camera centres -R^T t, 4 doubles per camera
  const int* pt_off;
  const int* p_cam;
  UvArr uv;
  const int* list;         // long form: the point slots to do; short form: null (every slot of at most `thr` observations)
  int n_items, thr;
  double fx, fy, cx, cy;
  int loss, iters;
  double fscale, min_angle, max_px, min_depth;
  double* out;             // TRK_OUT doubles per point slot
};

__global__ void k_track_centres(const double* __restrict__ cs, int n_cams, double* __restrict__ ctr) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_cams) return;
  double* o = ctr + 4 * (size_t)c;
  cam_centre(cs + CS * (size_t)c, o);
  o[3] = 0.0;
}

// sums / maxima over the lanes of a track's group, the same bits in every lane.  8 lanes: two quad permutes and the
// half-row mirror (a butterfly: every lane adds the same two numbers at every level); 64: ba_dpp.hpp's wave total / maximum.
constexpr int DPP_QUAD_1032 = 0xB1, DPP_QUAD_2301 = 0x4E, DPP_ROW_HALF_MIRROR = 0x141;
template <int G> __device__ __forceinline__ double trk_sum(double x);
template <> __device__ __forceinline__ double trk_sum<8>(double x) {
  x += dpp_f64<DPP_QUAD_1032, 0xf>(x);
  x += dpp_f64<DPP_QUAD_2301, 0xf>(x);
  x += dpp_f64<DPP_ROW_HALF_MIRROR, 0xf>(x);
  return x;
}
template <> __device__ __forceinline__ double trk_sum<64>(double x) { return wave_total_dpp(x); }
template <int G> __device__ __forceinline__ double trk_max(double x);
// (of non-negative numbers: a lane without a source reads 0)
template <> __device__ __forceinline__ double trk_max<8>(double x) {
  x = fmax(x, dpp_f64<DPP_QUAD_1032, 0xf>(x));
  x = fmax(x, dpp_f64<DPP_QUAD_2301, 0xf>(x));
  x = fmax(x, dpp_f64<DPP_ROW_HALF_MIRROR, 0xf>(x));
  return x;
}
template <> __device__ __forceinline__ double trk_max<64>(double x) { return wave_max_dpp(x); }

// the view's (x, y) of step 1; false: the BAL inversion failed
template <class CM>
__device__ __forceinline__ bool trk_bearing(const double (&cam)[CM::CAM], const double2 uv, const TrackArgs& a, double& x, double& y) {
  if constexpr (CM::ID == 0) {
    x = (uv.x - a.cx) / a.fx;
    y = (uv.y - a.cy) / a.fy;
    return true;
  } else {
    const double f = cam[12], k1 = cam[13], k2 = cam[14];
    const double qx = uv.x / f, qy = uv.y / f;
    const double rd = sqrt(qx * qx + qy * qy);
    double r = rd;
    bool ok = false;
    for (int it = 0; it < TRK_NEWTON_ITERS; ++it) {
      const double r2 = r * r;
      const double dF = 1.0 + r2 * (3.0 * k1 + 5.0 * k2 * r2);
      if (!(dF > 0.0)) break;
      const double dr = (r * (1.0 + r2 * (k1 + k2 * r2)) - rd) / dF;
      r -= dr;
      if (fabs(dr) <= 1e-15 * fabs(r)) { ok = true; break; }
    }
    const double r2 = r * r;
    ok = ok && (1.0 + r2 * (3.0 * k1 + 5.0 * k2 * r2) > 0.0) && r >= 0.0;
    const double sc = rd > 0.0 ? r / rd : 1.0;
    x = -qx * sc;
    y = -qy * sc;
    return ok;
  }
}

__device__ __forceinline__ void trk_unit(const double* __restrict__ ctr, int c, const double (&X)[3], double (&u)[3]) {
  const double* C = ctr + 4 * (size_t)c;
  const double d0 = C[0] - X[0], d1 = C[1] - X[1], d2 = C[2] - X[2];
  const double inv = 1.0 / sqrt(d0 * d0 + d1 * d1 + d2 * d2);
  u[0] = d0 * inv; u[1] = d1 * inv; u[2] = d2 * inv;
}

// One track on the G lanes [l = 0 .. G) of its group; stage: the wave's LDS (G = 64 only).
template <class CM, int G>
__device__ __forceinline__ void track_solve(const TrackArgs& a, const int s, const int l, double* __restrict__ stage) {
  const int beg = a.pt_off[s], end = a.pt_off[s + 1], n = end - beg;
  const double nan = HY_NAN;
  double* o = a.out + TRK_OUT * (size_t)s;
  double cam[CM::CAM];
  // distinct cameras, mean camera centre
  double Cm[3] = {0, 0, 0};
  {
    double differ = 0.0;
    const int c0 = n > 0 ? a.p_cam[beg] : 0;
    for (int j = beg + l; j < end; j += G) {
      const int c = a.p_cam[j];
      differ += (c != c0) ? 1.0 : 0.0;
      const double* C = a.ctr + 4 * (size_t)c;
      Cm[0] += C[0]; Cm[1] += C[1]; Cm[2] += C[2];
    }
    differ = trk_sum<G>(differ);
#pragma unroll
    for (int q = 0; q < 3; ++q) Cm[q] = trk_sum<G>(Cm[q]);
    if (differ == 0.0) {
      if (l == 0) { o[0] = nan; o[1] = nan; o[2] = nan; o[3] = nan; o[4] = nan; o[5] = nan; o[6] = (double)TRK_FEW_VIEWS; }
      return;
    }
    const double in = 1.0 / (double)n;
#pragma unroll
    for (int q = 0; q < 3; ++q) Cm[q] *= in;
  }
  // A^T A of the DLT rows
  double X[3];
  bool degenerate = false;
  {
    double m[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    double bad = 0.0;
    for (int j = beg + l; j < end; j += G) {
      const int c = a.p_cam[j];
      CM::load_cam_vec(a.cs, a.intr, c, cam);
      double xy[2];
      if (!trk_bearing<CM>(cam, a.uv[(size_t)j], a, xy[0], xy[1])) bad += 1.0;
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        double row[4];
#pragma unroll
        for (int q = 0; q < 3; ++q) row[q] = xy[r] * cam[6 + q] - cam[3 * r + q];
        row[3] = (xy[r] * cam[11] - cam[9 + r]) + (row[0] * Cm[0] + row[1] * Cm[1] + row[2] * Cm[2]);
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
          for (int q = p; q < 4; ++q) m[UT(4, p, q)] += row[p] * row[q];
      }
    }
    bad = trk_sum<G>(bad);
#pragma unroll
    for (int q = 0; q < 10; ++q) m[q] = trk_sum<G>(m[q]);
    double A[4][4], V[4][4];
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int q = 0; q < 4; ++q) A[p][q] = m[ST(4, p, q)];
    jacobi_eig<4, 16>(A, V);
    int best = 0;
    double lo = A[0][0];
    if (A[1][1] < lo) { lo = A[1][1]; best = 1; }
    if (A[2][2] < lo) { lo = A[2][2]; best = 2; }
    if (A[3][3] < lo) { lo = A[3][3]; best = 3; }
    double Xh[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {           // (selection without dynamic register indexing)
      Xh[k] = V[k][0];
      if (best == 1) Xh[k] = V[k][1];
      if (best == 2) Xh[k] = V[k][2];
      if (best == 3) Xh[k] = V[k][3];
    }
    const double w = fabs(Xh[3]), sg = Xh[3] < 0.0 ? -1.0 : 1.0;
    const double nrm = sqrt(Xh[0] * Xh[0] + Xh[1] * Xh[1] + Xh[2] * Xh[2] + Xh[3] * Xh[3]);
    degenerate = bad > 0.0 || !(w > 1e-12 * nrm) || !(nrm < 1.79e308);
#pragma unroll
    for (int q = 0; q < 3; ++q) X[q] = Cm[q] + sg * Xh[q] / w;
    if (degenerate) {
      if (l == 0) { o[0] = nan; o[1] = nan; o[2] = nan; o[3] = nan; o[4] = nan; o[5] = nan; o[6] = (double)TRK_DEGENERATE; }
      return;
    }
  }
  // refinement; the pass at the trial point also gives the measures of step 4
  double acc[TRK_NSUM], cur[TRK_NSUM];
  {
    double Xt[3] = {X[0], X[1], X[2]};
    double lam = 1e-4;
    bool first = true, small = false;
    int it = 0;
    for (;;) {
#pragma unroll
      for (int q = 0; q < TRK_NSUM; ++q) acc[q] = 0.0;
      for (int j = beg + l; j < end; j += G) {
        const int c = a.p_cam[j];
        CM::load_cam_vec(a.cs, a.intr, c, cam);
        const double2 uv = a.uv[(size_t)j];
        typename CM::template Obs<double> g;
        CM::template geom<false, double, double>(cam, Xt[0], Xt[1], Xt[2], a.fx, a.fy, g);
        double ru, rv;
        CM::residual(g, uv.x, uv.y, a.fx, a.fy, a.cx, a.cy, ru, rv);
        const double* Pm = CM::pm(g);
        double w0 = 1.0, w1 = 1.0, t0 = ru * ru, t1 = rv * rv;
        if (a.loss != LOSS_LINEAR) {
          robust_loss<true>(a.loss, ru, a.fscale, t0, w0);
          robust_loss<true>(a.loss, rv, a.fscale, t1, w1);
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const double wa0 = w0 * Pm[q], wa1 = w1 * Pm[3 + q];
#pragma unroll
          for (int r = q; r < 3; ++r) acc[U3(q, r)] += wa0 * Pm[r] + wa1 * Pm[3 + r];
          acc[6 + q] -= wa0 * ru + wa1 * rv;       // Jp = -Pm
        }
        acc[9] += t0 + t1;
        const double e2 = ru * ru + rv * rv;
        acc[10] += e2;
        acc[11] = fmax(acc[11], e2);
        const double pz = cam[6] * Xt[0] + cam[7] * Xt[1] + cam[8] * Xt[2] + cam[11];
        acc[12] += ((CM::ID == 0 ? pz : -pz) > a.min_depth) ? 0.0 : 1.0;
      }
#pragma unroll
      for (int q = 0; q < TRK_NSUM; ++q) acc[q] = (q == 11) ? trk_max<G>(acc[q]) : trk_sum<G>(acc[q]);
      if (first || acc[9] <= cur[9] * (1.0 + TRK_COST_SLACK)) {
#pragma unroll
        for (int q = 0; q < TRK_NSUM; ++q) cur[q] = acc[q];
        X[0] = Xt[0]; X[1] = Xt[1]; X[2] = Xt[2];
        if (!first) lam = fmax(0.1 * lam, 1e-12);
      } else {
        lam *= 10.0;
      }
      first = false;
      if (small || it >= a.iters) break;
      ++it;
      // (H + lam diag H) dx = -g
      const double h00 = cur[0] * (1.0 + lam), h11 = cur[3] * (1.0 + lam), h22 = cur[5] * (1.0 + lam);
      if (!(h00 > 0.0)) { degenerate = true; break; }
      const double l00 = sqrt(h00), l10 = cur[1] / l00, l20 = cur[2] / l00;
      const double d1 = h11 - l10 * l10;
      if (!(d1 > 0.0)) { degenerate = true; break; }
      const double l11 = sqrt(d1), l21 = (cur[4] - l20 * l10) / l11;
      const double d2 = h22 - l20 * l20 - l21 * l21;
      if (!(d2 > 0.0)) { degenerate = true; break; }
      const double l22 = sqrt(d2);
      const double y0 = -cur[6] / l00, y1 = (-cur[7] - l10 * y0) / l11, y2 = (-cur[8] - l20 * y0 - l21 * y1) / l22;
      const double dx2 = y2 / l22, dx1 = (y1 - l21 * dx2) / l11, dx0 = (y0 - l10 * dx1 - l20 * dx2) / l00;
      Xt[0] = X[0] + dx0; Xt[1] = X[1] + dx1; Xt[2] = X[2] + dx2;
      small = sqrt(dx0 * dx0 + dx1 * dx1 + dx2 * dx2) <= 1e-14 * sqrt(X[0] * X[0] + X[1] * X[1] + X[2] * X[2]);
    }
  }
  // largest |u_i - u_j|^2 over the pairs of views
  double d2max = 0.0;
  if constexpr (G == 64) {
    for (int c0 = beg; c0 < end; c0 += TRK_STAGE) {
      const int cn = min(TRK_STAGE, end - c0);
      __syncthreads();                        // (one wave per workgroup: the wave's own barrier)
      for (int k = l; k < cn; k += G) {
        double u[3];
        trk_unit(a.ctr, a.p_cam[c0 + k], X, u);
        stage[3 * k] = u[0]; stage[3 * k + 1] = u[1]; stage[3 * k + 2] = u[2];
      }
      __syncthreads();
      for (int j = beg + l; j < end; j += G) {
        if (j <= c0) continue;                // (pairs k < j only)
        double u[3];
        trk_unit(a.ctr, a.p_cam[j], X, u);
        const int kn = min(cn, j - c0);
        for (int k = 0; k < kn; ++k) {
          const double e0 = u[0] - stage[3 * k], e1 = u[1] - stage[3 * k + 1], e2 = u[2] - stage[3 * k + 2];
          d2max = fmax(d2max, e0 * e0 + e1 * e1 + e2 * e2);
        }
      }
    }
  } else {
    for (int j = beg + l; j < end; j += G) {
      double u[3];
      trk_unit(a.ctr, a.p_cam[j], X, u);
      for (int k = beg; k < j; ++k) {
        double v[3];
        trk_unit(a.ctr, a.p_cam[k], X, v);
        const double e0 = u[0] - v[0], e1 = u[1] - v[1], e2 = u[2] - v[2];
        d2max = fmax(d2max, e0 * e0 + e1 * e1 + e2 * e2);
      }
    }
  }
  d2max = trk_max<G>(d2max);
  if (l == 0) {
    const double angle = 2.0 * atan2(sqrt(d2max), sqrt(fmax(4.0 - d2max, 0.0))) * (180.0 / 3.14159265358979323846);
    const double rms = sqrt(cur[10] / (double)n), emax = sqrt(cur[11]);
    int st = TRK_OK;
    if (degenerate) st = TRK_DEGENERATE;
    else if (cur[12] > 0.0) st = TRK_BEHIND;
    else if (a.min_angle > 0.0 && angle < a.min_angle) st = TRK_LOW_ANGLE;
    else if (a.max_px > 0.0 && emax > a.max_px) st = TRK_HIGH_ERROR;
    o[0] = X[0]; o[1] = X[1]; o[2] = X[2]; o[3] = angle; o[4] = rms; o[5] = emax; o[6] = (double)st;
  }
}

// short tracks: TRK_G lanes each, TRK_THREADS / TRK_G tracks per workgroup
template <class CM>
__global__ void __launch_bounds__(TRK_THREADS) k_tracks_short(const TrackArgs a) {
  const int s = blockIdx.x * (TRK_THREADS / TRK_G) + threadIdx.x / TRK_G;
  if (s >= a.n_items) return;                                        // (whole groups leave: the DPP sums stay inside a group)
  if (a.pt_off[s + 1] - a.pt_off[s] > a.thr) return;
  track_solve<CM, TRK_G>(a, s, threadIdx.x % TRK_G, nullptr);
}
// long tracks: one wave, one workgroup each
template <class CM>
__global__ void __launch_bounds__(64) k_tracks_long(const TrackArgs a) {
  __shared__ double stage[3 * TRK_STAGE];
  if ((int)blockIdx.x >= a.n_items) return;
  track_solve<CM, 64>(a, a.list[blockIdx.x], threadIdx.x, stage);
}

// point slots -> the caller's point order
__global__ void k_tracks_unpermute(const double* __restrict__ out, const int* __restrict__ slot, int n_pts, double* __restrict__ xyz,
                                   double* __restrict__ meas, unsigned char* __restrict__ status) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pts) return;
  const double* s = out + TRK_OUT * (size_t)slot[p];
#pragma unroll
  for (int q = 0; q < 3; ++q) { xyz[3 * (size_t)p + q] = s[q]; meas[(size_t)q * n_pts + p] = s[3 + q]; }
  status[p] = (unsigned char)(int)s[6];
}
// write_points: the point table ba_set_params would build from the merged array (OK points that are not held take the
// triangulated position, every other point keeps its own; the table's other words start at 0 as they do there)
__global__ void k_tracks_merge(const double* __restrict__ out, const unsigned char* __restrict__ held, const double* __restrict__ ptab_cur,
                               int n_pts, double* __restrict__ ptab0) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_pts) return;
  const double* t = out + TRK_OUT * (size_t)s;
  const bool take = (int)t[6] == TRK_OK && !(held && held[s]);
  const double* src = take ? t : ptab_cur + PT * (size_t)s;
  const double x = src[0], y = src[1], z = src[2];
  double* o = ptab0 + PT * (size_t)s;
  o[0] = x; o[1] = y; o[2] = z;
  o[3] = 0; o[4] = 0; o[5] = 0; o[6] = 0; o[7] = 0;
}

}  // namespace ba
