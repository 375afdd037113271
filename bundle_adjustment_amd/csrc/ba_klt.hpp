// Pyramidal Lucas-Kanade point tracking (ba_track_klt), by the definition in include/ba_hip.h.  Sums are integers, everything else
// is fp64 with every operation rounded on its own (`#pragma clang fp contract(off)` where it is computed, as in ba_orb.hpp), so a
// numpy restatement decides every case identically and no result depends on how the window is split over lanes.
//
// Device images are level-major: level l holds the level image of every image a pair names (its slot s), at off[l] + s w_l h_l.
// Gradients are not stored: a point's wave recomputes the Scharr values of its window from the pyramid.
// Launches of one call (L = the top level):
//   k_klt_down    L   level l from level l - 1 of every slot: a KLT_TILE_W x KLT_TILE_H tile of the level per workgroup, a thread
//                     per pixel; the (2 TW + 3) x (2 TH + 3) source pixels in LDS (reflected at the border), the 1 4 6 4 1 row sums
//                     (exact 16-bit) in LDS, then the column sums.
//   k_klt_track   1   a wave (= a workgroup) per point, walking the levels from the top.  Per level the (n + 3)^2 pixels of image a
//                     around the window go to LDS, then the Scharr gradients and the pixel at the (n + 1)^2 clamped sample
//                     positions (16-bit), then each lane takes the window elements lane, lane + 64, ... (EPL of them: 7 at
//                     half_window 10, 16 at 15) and keeps T, Gx, Gy of those in registers for the level's iterations.  An iteration
//                     stages the (n + 1)^2 pixels of image b in LDS, every lane interpolates its elements, and the two sums are
//                     reduced over the wave.  With fb_max_px > 0 the same wave tracks an OK point back with the slots swapped.
//                     Every branch is uniform over the wave: it depends only on wave totals and on the point.
// Per-lane partial sums are int32: |d| <= 8162 and |Gx|, |Gy| <= 4082 (a weight may overshoot 16384 by one), so the EPL <= 16
// terms of a lane add up to at most 16 * 8162 * 4082 < 2^30 in magnitude.  The wave totals are taken in fp64 (ba_dpp.hpp): the
// partials and every sum of them are integers below 64 * 2^30 < 2^53, so every addition is exact in any order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ba_dpp.hpp"

namespace ba {

constexpr int KLT_MAX_LEVELS = 9;     // max_level <= 8
constexpr int KLT_MAX_HALF = 15;      // half_window <= 15: n <= 31
constexpr int KLT_TILE_W = 32;        // tile of k_klt_down
constexpr int KLT_TILE_H = 8;
constexpr int KLT_THREADS = 256;
constexpr int KLT_PS = 2 * KLT_MAX_HALF + 4;      // row stride of the template's pixel patch in LDS, (n + 3) <= 34
constexpr int KLT_GS = 2 * KLT_MAX_HALF + 2;      // row stride of the sample arrays in LDS, (n + 1) <= 32
static_assert(KLT_TILE_W * KLT_TILE_H == KLT_THREADS, "k_klt_down: a thread per pixel of the tile");

enum { KLT_OK = 0, KLT_OUT = 1, KLT_FLAT = 2, KLT_FB_FAIL = 3 };

struct KltArgs {
  int n_levels, hw, n, max_iters, fb, n_pairs;
  int w[KLT_MAX_LEVELS], h[KLT_MAX_LEVELS];
  long long off[KLT_MAX_LEVELS];     // first pixel of level l (of slot 0)
  double eps2, min_eig, fb_max;
  unsigned char* pyr;
  const int* pair_slot;              // [n_pairs][2]
  const long long* pt_off;           // [n_pairs + 1]
  const float* prev;
  const float* guess;                // or null
  float* next; unsigned char* status; float* err; float* fb_err;
};

__device__ __forceinline__ int klt_clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }

// r of the definition; the clamp binds only for the pixels of a tile beyond the image, whose results are not written
__device__ __forceinline__ int klt_reflect(int i, int n) {
  i = i < 0 ? -i : i;
  i = i >= n ? 2 * n - 2 - i : i;
  return klt_clamp(i, 0, n - 1);
}

__global__ __launch_bounds__(KLT_THREADS) void k_klt_down(KltArgs a, int l) {
  constexpr int SW = 2 * KLT_TILE_W + 3, SH = 2 * KLT_TILE_H + 3;
  __shared__ unsigned char pix[SH * SW];
  __shared__ unsigned short tmp[SH * KLT_TILE_W];
  const int ws = a.w[l - 1], hs = a.h[l - 1], wd = a.w[l], hd = a.h[l];
  const int tx0 = blockIdx.x * KLT_TILE_W, ty0 = blockIdx.y * KLT_TILE_H;
  const unsigned char* src = a.pyr + a.off[l - 1] + (long long)blockIdx.z * ws * hs;
  for (int e = threadIdx.x; e < SH * SW; e += KLT_THREADS) {
    const int sy = 2 * ty0 - 2 + e / SW, sx = 2 * tx0 - 2 + e % SW;
    pix[e] = src[(long long)klt_reflect(sy, hs) * ws + klt_reflect(sx, ws)];
  }
  __syncthreads();
  for (int e = threadIdx.x; e < SH * KLT_TILE_W; e += KLT_THREADS) {
    const unsigned char* q = pix + (e / KLT_TILE_W) * SW + 2 * (e % KLT_TILE_W);
    tmp[e] = (unsigned short)(q[0] + 4 * q[1] + 6 * q[2] + 4 * q[3] + q[4]);      // <= 16 * 255
  }
  __syncthreads();
  const int lx = threadIdx.x % KLT_TILE_W, ly = threadIdx.x / KLT_TILE_W;
  const int gx = tx0 + lx, gy = ty0 + ly;
  if (gx >= wd || gy >= hd) return;
  const unsigned short* t = tmp + 2 * ly * KLT_TILE_W + lx;
  const unsigned v = t[0] + 4u * t[KLT_TILE_W] + 6u * t[2 * KLT_TILE_W] + 4u * t[3 * KLT_TILE_W] + t[4 * KLT_TILE_W];
  a.pyr[a.off[l] + (long long)blockIdx.z * wd * hd + (long long)gy * wd + gx] = (unsigned char)((v + 128u) >> 8);
}

struct KltWeights { int w00, w01, w10, w11; };

// the four 14-bit weights of the fractions a (columns) and b (rows)
__device__ __forceinline__ KltWeights klt_weights(double a, double b) {
#pragma clang fp contract(off)
  const double ca = 1.0 - a, cb = 1.0 - b;
  double t = ca * cb;
  KltWeights k;
  k.w00 = (int)rint(t * 16384.0);
  t = a * cb;
  k.w01 = (int)rint(t * 16384.0);
  t = ca * b;
  k.w10 = (int)rint(t * 16384.0);
  k.w11 = 16384 - k.w00 - k.w01 - k.w10;
  return k;
}

template <typename T>
__device__ __forceinline__ int klt_lerp(const T* p, const KltWeights& k, int shift) {      // p: the element's top-left sample, stride KLT_GS
  return (k.w00 * (int)p[0] + k.w01 * (int)p[1] + k.w10 * (int)p[KLT_GS] + k.w11 * (int)p[KLT_GS + 1] + (1 << (shift - 1))) >> shift;
}

__device__ __forceinline__ bool klt_inside(double x, double y, int w, int h) {      // (written so that a NaN is outside)
  return 0.0 <= x && x <= (double)(w - 1) && 0.0 <= y && y <= (double)(h - 1);
}

__device__ __forceinline__ double klt_total(int v) { return wave_total_dpp((double)v); }

struct KltLds {
  unsigned char pa[KLT_PS * KLT_PS];      // image a around the window: pa[r][c] = P_a(ix - 1 + c, iy - 1 + r), coordinates clamped
  short gx[KLT_GS * KLT_GS];              // Ix, Iy, P of image a at the (n + 1)^2 clamped sample positions
  short gy[KLT_GS * KLT_GS];
  unsigned char pc[KLT_GS * KLT_GS];
  unsigned char pb[KLT_GS * KLT_GS];      // image b at the (n + 1)^2 clamped sample positions of an iteration
};

// the (n + 1)^2 pixels of level image B (w x h) under the window whose top-left corner is (cx, cy), into s.pb; -> the weights
__device__ __forceinline__ KltWeights klt_stage_b(KltLds& s, const unsigned char* B, int w, int h, int n, double cx, double cy, int lane) {
#pragma clang fp contract(off)
  const double fx = floor(cx), fy = floor(cy);
  const int jx = (int)fx, jy = (int)fy;
  __syncthreads();      // the readers of the patch before this one are done
  for (int e = lane; e < (n + 1) * (n + 1); e += 64) {
    const int r = e / (n + 1), c = e % (n + 1);
    s.pb[r * KLT_GS + c] = B[(long long)klt_clamp(jy + r, 0, h - 1) * w + klt_clamp(jx + c, 0, w - 1)];
  }
  __syncthreads();
  return klt_weights(cx - fx, cy - fy);
}

// One point from slot sa into slot sb.  (px, py): the position in a, inside the image; (qx, qy): in, the start in b in level-0
// pixels; out, the result.  -> the status; err is set when that is KLT_OK.
template <int EPL>
__device__ __forceinline__ int klt_point(const KltArgs& a, KltLds& s, int sa, int sb, double px, double py, double& qx, double& qy,
                                         double& err, int lane) {
#pragma clang fp contract(off)
  const int n = a.n, hw = a.hw, n2 = n * n, L = a.n_levels - 1;
  const double top = (double)(1 << L), half = (double)hw;
  qx = qx / top;
  qy = qy / top;
  int T[EPL], Gx[EPL], Gy[EPL], at[EPL];
#pragma unroll
  for (int k = 0; k < EPL; ++k) {
    const int e = lane + 64 * k;
    at[k] = e < n2 ? (e / n) * KLT_GS + e % n : -1;      // the element's top-left sample; -1: the lane has no such element
  }
  for (int l = L; l >= 0; --l) {
    const int w = a.w[l], h = a.h[l];
    const unsigned char* A = a.pyr + a.off[l] + (long long)sa * w * h;
    const unsigned char* B = a.pyr + a.off[l] + (long long)sb * w * h;
    const double sc = (double)(1 << l);
    const double cx = px / sc - half, cy = py / sc - half;
    const double fx = floor(cx), fy = floor(cy);
    const int ix = (int)fx, iy = (int)fy;
    const KltWeights ka = klt_weights(cx - fx, cy - fy);
    __syncthreads();
    for (int e = lane; e < (n + 3) * (n + 3); e += 64) {
      const int r = e / (n + 3), c = e % (n + 3);
      s.pa[r * KLT_PS + c] = A[(long long)klt_clamp(iy - 1 + r, 0, h - 1) * w + klt_clamp(ix - 1 + c, 0, w - 1)];
    }
    __syncthreads();
    // A sample position (X, Y) = clamp(ix + c, iy + r) and its neighbours clamp(X +- 1, Y +- 1) are image pixels within the
    // staged range (p lies inside the image, so -hw <= ix <= w - 1 - hw): patch column X' - (ix - 1).  The clamp to the patch
    // never binds.
    for (int e = lane; e < (n + 1) * (n + 1); e += 64) {
      const int r = e / (n + 1), c = e % (n + 1);
      const int X = klt_clamp(ix + c, 0, w - 1), Y = klt_clamp(iy + r, 0, h - 1);
      const int x0 = klt_clamp(X - (ix - 1), 0, n + 2), xm = klt_clamp(max(X - 1, 0) - (ix - 1), 0, n + 2), xp = klt_clamp(min(X + 1, w - 1) - (ix - 1), 0, n + 2);
      const int y0 = klt_clamp(Y - (iy - 1), 0, n + 2), ym = klt_clamp(max(Y - 1, 0) - (iy - 1), 0, n + 2), yp = klt_clamp(min(Y + 1, h - 1) - (iy - 1), 0, n + 2);
      const unsigned char *rm = s.pa + ym * KLT_PS, *r0 = s.pa + y0 * KLT_PS, *rp = s.pa + yp * KLT_PS;
      const int mm = rm[xm], m0 = rm[x0], mp = rm[xp], zm = r0[xm], zp = r0[xp], pm = rp[xm], p0 = rp[x0], pp = rp[xp];
      s.gx[r * KLT_GS + c] = (short)(3 * (mp - mm) + 10 * (zp - zm) + 3 * (pp - pm));      // |.| <= 16 * 255
      s.gy[r * KLT_GS + c] = (short)(3 * (pm - mm) + 10 * (p0 - m0) + 3 * (pp - mp));
      s.pc[r * KLT_GS + c] = r0[x0];
    }
    __syncthreads();
    int s11 = 0, s12 = 0, s22 = 0;
#pragma unroll
    for (int k = 0; k < EPL; ++k) {
      const bool live = at[k] >= 0;
      const int o = live ? at[k] : 0;
      const int t = klt_lerp(s.pc + o, ka, 9), u = klt_lerp(s.gx + o, ka, 14), v = klt_lerp(s.gy + o, ka, 14);
      T[k] = live ? t : 0; Gx[k] = live ? u : 0; Gy[k] = live ? v : 0;
      s11 += Gx[k] * Gx[k]; s12 += Gx[k] * Gy[k]; s22 += Gy[k] * Gy[k];
    }
    const double A11 = klt_total(s11), A12 = klt_total(s12), A22 = klt_total(s22);
    const double t1 = A11 * A22, t2 = A12 * A12;
    const double D = t1 - t2;
    double dd = A11 - A22;
    dd = dd * dd;
    const double f4 = 4.0 * t2;
    const double root = sqrt(dd + f4);
    double ev = (A11 + A22 - root) / (double)(2 * n2);
    ev = ev / 1048576.0;
    if (!(D > 0.0) || ev < a.min_eig) {
      if (l == 0) return KLT_FLAT;
      qx = 2.0 * qx; qy = 2.0 * qy;
      continue;
    }
    double pdx = 0.0, pdy = 0.0;
    for (int it = 0; it < a.max_iters; ++it) {
      if (!klt_inside(qx, qy, w, h)) {
        if (l == 0) return KLT_OUT;
        break;
      }
      const KltWeights kb = klt_stage_b(s, B, w, h, n, qx - half, qy - half, lane);
      int s1 = 0, s2 = 0;
#pragma unroll
      for (int k = 0; k < EPL; ++k) {
        const int d = klt_lerp(s.pb + max(at[k], 0), kb, 9) - T[k];      // (a lane without the element: Gx = Gy = 0)
        s1 += d * Gx[k]; s2 += d * Gy[k];
      }
      const double b1 = klt_total(s1), b2 = klt_total(s2);
      double u1 = A12 * b2, u2 = A22 * b1;
      const double dx = (u1 - u2) / D;
      u1 = A12 * b1; u2 = A11 * b2;
      const double dy = (u1 - u2) / D;
      qx = qx + dx; qy = qy + dy;
      u1 = dx * dx; u2 = dy * dy;
      if (u1 + u2 <= a.eps2) break;
      if (it > 0 && fabs(dx + pdx) < 0.01 && fabs(dy + pdy) < 0.01) {
        u1 = 0.5 * dx; u2 = 0.5 * dy;
        qx = qx - u1; qy = qy - u2;
        break;
      }
      pdx = dx; pdy = dy;
    }
    if (l > 0) { qx = 2.0 * qx; qy = 2.0 * qy; }
  }
  const int w = a.w[0], h = a.h[0];
  if (!klt_inside(qx, qy, w, h)) return KLT_OUT;
  const KltWeights kb = klt_stage_b(s, a.pyr + (long long)sb * w * h, w, h, n, qx - half, qy - half, lane);
  int sum = 0;
#pragma unroll
  for (int k = 0; k < EPL; ++k) sum += at[k] >= 0 ? abs(klt_lerp(s.pb + max(at[k], 0), kb, 9) - T[k]) : 0;
  err = klt_total(sum) / (32.0 * (double)n2);
  return KLT_OK;
}

template <int EPL>
__global__ __launch_bounds__(64) void k_klt_track(KltArgs a) {
#pragma clang fp contract(off)
  __shared__ KltLds s;
  const long long i = blockIdx.x;
  const int lane = threadIdx.x;
  int lo = 0, hi = a.n_pairs;      // the pair with pt_off[lo] <= i < pt_off[lo + 1]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (a.pt_off[mid] <= i) lo = mid; else hi = mid;
  }
  int s0 = a.pair_slot[2 * lo], s1 = a.pair_slot[2 * lo + 1];
  const float nanf_ = __int_as_float(0x7fc00000);
  const float fpx = a.prev[2 * i], fpy = a.prev[2 * i + 1];
  const double px = (double)fpx, py = (double)fpy;
  const int W = a.w[0], H = a.h[0];
  float nx = fpx, ny = fpy, ferr = nanf_, fberr = nanf_;
  int st = KLT_OUT;
  if (klt_inside(px, py, W, H)) {
    double qx = a.guess ? (double)a.guess[2 * i] : px, qy = a.guess ? (double)a.guess[2 * i + 1] : py, e = 0.0;
    double ax = px, ay = py;
    for (int pass = 0; pass < 2; ++pass) {      // forward; then, for an OK point under the forward-backward check, back
      const int r = klt_point<EPL>(a, s, s0, s1, ax, ay, qx, qy, e, lane);
      if (pass == 0) {
        st = r;
        nx = (float)qx; ny = (float)qy;
        if (r != KLT_OK) break;
        ferr = (float)e;
        if (!a.fb) break;
        ax = (double)nx; ay = (double)ny;
        qx = ax; qy = ay;
        const int t = s0; s0 = s1; s1 = t;
        if (!klt_inside(ax, ay, W, H)) { st = KLT_FB_FAIL; break; }      // (never: an OK point lies inside, and so does its float32)
      } else if (r != KLT_OK) {
        st = KLT_FB_FAIL;
      } else {
        const double dx = (double)(float)qx - px, dy = (double)(float)qy - py;
        const double u1 = dx * dx, u2 = dy * dy;
        const double dist = sqrt(u1 + u2);
        fberr = (float)dist;
        if (dist > a.fb_max) st = KLT_FB_FAIL;
      }
    }
  }
  if (lane == 0) {
    a.next[2 * i] = nx; a.next[2 * i + 1] = ny;
    a.status[i] = (unsigned char)st;
    a.err[i] = ferr;
    a.fb_err[i] = fberr;
  }
}

}  // namespace ba
