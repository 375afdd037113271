// ORB feature extraction (ba_orb_extract): image pyramid, FAST-9 with non-maximum suppression, Harris ranking, intensity-centroid
// orientation and steered BRIEF on a blurred pyramid -- the published algorithm, by the definition in include/ba_hip.h.  Every
// stage is integer arithmetic, or fp64 with every operation rounded on its own (`#pragma clang fp contract(off)` where it is
// computed, as in ba_match_guided.hpp), so a numpy restatement decides every case identically.  Nothing here depends on the order
// in which workgroups run: the only atomics are integer counts, and both selections are by a total order.
//
// Device images are level-major: level l holds the level image of every image of the batch, image b at off[l] + b w_l h_l.
// Launches of one call (L = the levels that have an interior; all images of the batch in each):
//   k_orb_resize       L - 1   level l from level l - 1 (fixed-point bilinear), a lane per pixel.
//   k_orb_fast         L       a ORB_TILE_W x ORB_TILE_H tile per workgroup: pixels with a 4-pixel halo in LDS, the FAST score of the
//                              tile and a 1-pixel halo into LDS (a four-pixel reject, then sliding minima / maxima over the 16
//                              arcs), the suppression, the score image (0 where the pixel is no candidate) and the 256-bin
//                              histogram of the candidates' scores per (image, level) (integer atomics, LDS first).
//   k_orb_cut          1       a lane per (image, level): the stage-1 cut score T, the number of score-T candidates kept in raster
//                              order, the numbers kept by both stages, the first output row of every level, n_kp.
//   k_orb_rowcount     1       a wave per level row: the candidates above the cut and on it.
//   k_orb_scan         1       a workgroup per (image, level): exclusive scans over the rows of the ties, then of the kept.
//   k_orb_compact      1       a wave per level row: the kept candidates' raster indices into the stage-1 list, in raster order.
//   k_orb_harris       1       a lane per kept candidate: Hs (int64).
//   k_orb_rank         1       a lane per kept candidate: its rank under (Hs descending, raster ascending) by counting, the
//                              list streamed through LDS; ranks below the quota write octave, level_xy, xy, size, response.
//   k_orb_blur         L       the 7 x 7 integer Gaussian of a tile (3-pixel halo, exact 16-bit row sums in LDS).
//   k_orb_describe     1       a wave per keypoint: the patch moments (two patch rows per step, integer butterfly), (c, s) and
//                              the angle, then four tests per lane, two lanes per descriptor byte.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ba {

constexpr int ORB_MAX_LEVELS = 16;
constexpr int ORB_TILE_W = 64;      // tile of k_orb_fast and k_orb_blur
constexpr int ORB_TILE_H = 16;
constexpr int ORB_THREADS = 256;
constexpr int ORB_KP_PER_BLOCK = 4;   // k_orb_describe: a wave per keypoint

// The default test pairs (x1, y1, x2, y2): BRIEF's "G II" sampling, both points isotropic Gaussian with sigma = 31 / 5, rounded.
// NOT OpenCV's learned pattern.  Generated once by
//   rng = numpy.random.default_rng(31); rows, seen = [], set()
//   while len(rows) < 256:
//       t = tuple(int(v) for v in numpy.rint(rng.normal(0.0, 31.0 / 5.0, 4)))
//       if max(abs(v) for v in t) > 13 or t[:2] == t[2:] or t in seen: continue
//       seen.add(t); rows.append(t)
static const int8_t kOrbDefaultPattern[256][4] = {
    {-2,2,4,-6}, {7,-6,11,7}, {-4,4,3,-11}, {4,-4,-2,-4}, {-3,0,1,-10}, {-2,-8,-8,-2}, {5,4,-4,-4}, {-5,1,6,0},
    {4,2,9,-12}, {-13,-1,4,-3}, {3,-7,-8,-4}, {5,4,-4,1}, {-4,0,-7,0}, {-5,0,-4,-5}, {1,-2,0,-3}, {4,-5,5,8},
    {-2,11,13,3}, {-8,-10,-1,11}, {4,5,-2,-5}, {2,-7,-1,3}, {0,3,-3,4}, {3,-10,-6,-4}, {4,2,2,1}, {4,6,-3,-10},
    {4,-1,0,-1}, {-7,-9,6,7}, {6,1,2,-3}, {0,-2,-3,1}, {11,-12,4,4}, {-8,2,1,-3}, {10,-2,2,2}, {-5,-2,3,-3},
    {-11,-8,2,-2}, {-2,8,1,-4}, {0,13,-7,11}, {9,-1,-2,9}, {2,-3,11,1}, {2,0,-2,1}, {-2,3,7,7}, {7,9,5,-4},
    {6,-10,-4,2}, {-10,9,-6,-9}, {-5,-5,0,-1}, {6,-1,1,-6}, {3,-5,-12,8}, {-7,-7,-5,4}, {-9,-2,4,12}, {-2,0,-5,12},
    {-1,0,1,-6}, {0,-8,9,-1}, {-1,7,-8,9}, {9,-5,4,-1}, {5,0,-6,4}, {-1,1,6,8}, {4,-9,4,-2}, {7,-1,9,3},
    {0,2,-11,4}, {1,-7,3,2}, {2,-1,5,5}, {1,0,-3,-4}, {4,-3,-9,2}, {7,-2,5,3}, {-6,2,-1,4}, {7,-1,1,5},
    {8,1,4,3}, {-4,10,5,1}, {7,3,-3,6}, {0,4,6,6}, {12,1,-1,-4}, {-4,4,3,-5}, {-4,-3,10,-6}, {2,-10,-1,9},
    {-8,7,-11,1}, {-7,0,-1,5}, {2,1,-3,3}, {-5,-4,-4,4}, {-3,3,4,5}, {10,-1,7,2}, {4,-1,8,-6}, {0,6,-7,8},
    {6,-1,0,0}, {0,8,3,-8}, {-4,0,9,1}, {0,6,4,2}, {-4,-2,5,0}, {3,3,2,0}, {4,5,9,3}, {-3,-4,4,-9},
    {-3,7,-2,-4}, {-3,6,9,7}, {4,2,-1,0}, {-10,-3,4,-1}, {5,-9,-3,-6}, {7,-1,-2,-7}, {-7,-1,-5,8}, {-6,-5,2,10},
    {0,0,7,3}, {-1,8,11,-4}, {6,8,-5,4}, {0,7,7,-13}, {-1,9,3,-6}, {-3,-7,2,-8}, {8,5,11,7}, {6,6,4,-12},
    {0,-10,2,3}, {1,9,-7,6}, {-6,3,4,-3}, {-5,7,-3,8}, {-3,5,5,1}, {-2,3,7,4}, {9,4,-4,-1}, {1,11,-6,2},
    {9,7,-1,-1}, {-11,-10,-5,5}, {5,8,6,5}, {1,-5,8,-2}, {-1,2,-7,4}, {2,-5,2,-8}, {4,-3,2,-6}, {-5,-1,5,1},
    {7,5,-5,-2}, {3,6,-5,-4}, {5,7,4,-4}, {-11,-5,5,-13}, {-3,7,7,1}, {-2,2,4,-2}, {-5,-4,-5,0}, {0,4,4,-1},
    {-13,4,-6,11}, {1,3,-3,-3}, {-3,5,-7,6}, {-2,4,-6,0}, {-11,-4,-1,-6}, {-1,1,1,-13}, {-2,-1,-5,-6}, {12,5,6,7},
    {-6,-2,-11,1}, {-12,-4,5,3}, {-6,-6,8,3}, {-3,1,1,-7}, {-3,-13,1,1}, {6,6,-3,10}, {-5,6,-3,-4}, {3,-2,3,4},
    {3,9,0,3}, {10,4,-5,8}, {4,-5,-5,-2}, {11,1,-4,9}, {-4,-5,-1,2}, {0,4,2,-1}, {3,-5,-6,2}, {-10,4,-2,5},
    {1,-5,-4,-2}, {8,9,-1,1}, {-5,9,2,-4}, {-8,3,12,1}, {2,1,9,6}, {-3,-11,1,-4}, {1,-10,-2,-1}, {-10,1,11,2},
    {3,4,-11,9}, {-8,-13,3,5}, {9,7,2,2}, {5,2,3,-13}, {-1,-2,3,-5}, {6,5,-7,0}, {2,0,7,2}, {10,-4,10,-2},
    {3,-12,-5,7}, {0,0,-7,5}, {-6,9,4,-3}, {-5,-3,2,2}, {-10,2,-7,11}, {-12,6,-7,2}, {7,3,-7,-10}, {9,-5,5,7},
    {-10,12,-1,-1}, {-6,1,3,7}, {6,6,-1,-1}, {1,1,8,6}, {-1,-6,-12,-1}, {0,-12,-2,2}, {1,-9,-4,-9}, {9,0,1,7},
    {-12,-7,9,6}, {12,4,-3,5}, {-3,0,-1,-5}, {13,4,1,2}, {-4,-2,1,2}, {-13,8,-13,-6}, {-9,1,-11,6}, {4,6,5,-2},
    {1,-6,-3,3}, {-8,-2,-3,6}, {3,-3,5,12}, {7,1,1,-6}, {-3,2,2,-9}, {-8,-8,-7,-4}, {-1,-7,-4,-12}, {-2,1,-4,-10},
    {-5,1,-1,1}, {0,-5,-6,-2}, {-4,-4,2,1}, {-3,6,-1,-2}, {5,1,-10,2}, {-10,-2,1,4}, {-6,-3,4,12}, {12,5,10,-4},
    {-2,5,5,-10}, {7,-6,-1,-7}, {-2,6,-8,-4}, {0,3,10,1}, {7,-4,4,-7}, {-7,-7,-5,-2}, {-11,0,3,-12}, {-10,-7,-6,10},
    {-8,-11,2,-11}, {1,5,-6,-5}, {-6,8,4,3}, {5,0,-4,2}, {5,-1,-2,-6}, {8,5,1,1}, {2,0,6,1}, {5,0,-4,7},
    {7,10,-3,-4}, {-12,0,-5,7}, {-7,6,-8,-1}, {8,-3,2,4}, {1,3,6,7}, {-8,-1,-13,2}, {-4,2,-11,-7}, {3,4,-2,-3},
    {4,-10,-3,-6}, {1,13,8,1}, {2,-1,-6,-4}, {0,7,1,-2}, {-13,-5,10,1}, {-2,10,0,-12}, {-3,9,7,-2}, {8,3,7,5},
    {1,-2,-2,0}, {5,5,9,-1}, {2,-12,-4,-4}, {0,1,-3,3}, {-3,0,-4,1}, {-3,-1,-5,-8}, {8,-5,7,-2}, {0,1,-5,-10},
    {5,1,-10,-4}, {-4,7,3,0}, {7,3,-5,-9}, {6,-11,7,-11}, {-4,8,5,7}, {-9,-2,0,-3}, {-4,2,0,-6}, {-4,-2,0,-2}
};

struct OrbCut {       // per (image, level)
  int T;              // stage-1 cut score: candidates above it are kept, those on it in raster order while n_tie lasts
  int n_tie;
  int K;              // kept by stage 1 (<= 2 quota)
  int m;              // kept by stage 2 (<= quota)
  int out0;           // first output row of the level within its image
};

struct OrbArgs {
  int n_levels, n_features, edge, thr, n_images;
  int rows, list_cap;             // sum of h_l; sum of 2 quota_l
  int w[ORB_MAX_LEVELS], h[ORB_MAX_LEVELS], quota[ORB_MAX_LEVELS];
  int row0[ORB_MAX_LEVELS];       // first row of level l among the level rows of one image
  int list0[ORB_MAX_LEVELS];      // first entry of level l in the stage-1 list of one image
  long long off[ORB_MAX_LEVELS];  // first pixel of level l (of image 0)
  double scale[ORB_MAX_LEVELS];
  unsigned char* pyr;
  unsigned char* score;
  unsigned char* blur;
  unsigned* hist;                 // [image][level][256]
  OrbCut* cut;                    // [image][level]
  int* row_a;                     // [image][rows]  candidates above the cut; after k_orb_scan: kept before the row
  int* row_b;                     // [image][rows]  candidates on the cut;    after k_orb_scan: ties before the row
  int* list;                      // [image][list_cap]  raster indices kept by stage 1
  long long* hs;                  // [image][list_cap]
  const signed char* pattern;     // [256][4]
  // outputs, stride n_features rows per image
  int* n_kp;
  float* xy; float* size; float* angle; float* response;
  int* octave; int* level_xy;
  double* cs;
  unsigned char* desc;
};

__device__ __forceinline__ long long orb_img(const OrbArgs& a, int l, int b) {
  return a.off[l] + (long long)b * a.w[l] * a.h[l];
}

// source indices and the 11-bit weight of the second one for destination index i of an axis resized from n_src to n_dst
__device__ __forceinline__ void orb_axis(int n_src, int n_dst, int i, int& i0, int& i1, unsigned& a1) {
#pragma clang fp contract(off)
  const double ratio = (double)n_src / (double)n_dst;
  const double s = ((double)i + 0.5) * ratio - 0.5;
  const double fl = floor(s);
  double f = s - fl;
  const int k = (int)fl;
  if (k < 0 || k > n_src - 1) f = 0.0;
  i0 = min(max(k, 0), n_src - 1);
  i1 = min(max(k + 1, 0), n_src - 1);
  a1 = (unsigned)rint(f * 2048.0);
}

__global__ __launch_bounds__(ORB_THREADS) void k_orb_resize(OrbArgs a, int l) {
  const int wd = a.w[l], hd = a.h[l], ws = a.w[l - 1], hs = a.h[l - 1];
  const int i = blockIdx.x * ORB_THREADS + threadIdx.x;
  if (i >= wd * hd) return;
  const int x = i % wd, y = i / wd;
  int x0, x1, y0, y1;
  unsigned ax, ay;
  orb_axis(ws, wd, x, x0, x1, ax);
  orb_axis(hs, hd, y, y0, y1, ay);
  const unsigned char* src = a.pyr + orb_img(a, l - 1, blockIdx.y);
  const unsigned r0 = (2048u - ax) * src[(long long)y0 * ws + x0] + ax * src[(long long)y0 * ws + x1];
  const unsigned r1 = (2048u - ax) * src[(long long)y1 * ws + x0] + ax * src[(long long)y1 * ws + x1];
  a.pyr[orb_img(a, l, blockIdx.y) + i] = (unsigned char)(((2048u - ay) * r0 + ay * r1 + (1u << 21)) >> 22);
}

// FAST-9 score of the pixel at p (row stride S): max over the 16 arcs of 9 ring pixels of max(min(ring - v), min(v - ring)),
// or 0 when the four compass pixels already show that it cannot exceed thr (every arc of 9 holds at least two of them).
template <int S>
__device__ __forceinline__ int orb_fast_score(const unsigned char* p, int thr) {
  const int v = p[0];
  const int c0 = p[-3 * S], c4 = p[3], c8 = p[3 * S], c12 = p[-3];
  const int hi = v + thr, lo = v - thr;
  const int nb = (c0 > hi) + (c4 > hi) + (c8 > hi) + (c12 > hi), nd = (c0 < lo) + (c4 < lo) + (c8 < lo) + (c12 < lo);
  if (nb < 2 && nd < 2) return 0;
  int d[16];
  d[0] = c0 - v;             d[1] = p[-3 * S + 1] - v;  d[2] = p[-2 * S + 2] - v;  d[3] = p[-S + 3] - v;
  d[4] = c4 - v;             d[5] = p[S + 3] - v;       d[6] = p[2 * S + 2] - v;   d[7] = p[3 * S + 1] - v;
  d[8] = c8 - v;             d[9] = p[3 * S - 1] - v;   d[10] = p[2 * S - 2] - v;  d[11] = p[S - 3] - v;
  d[12] = c12 - v;           d[13] = p[-S - 3] - v;     d[14] = p[-2 * S - 2] - v; d[15] = p[-3 * S - 1] - v;
  int mn2[16], mx2[16], mn4[16], mx4[16], mn8[16], mx8[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) { mn2[k] = min(d[k], d[(k + 1) & 15]); mx2[k] = max(d[k], d[(k + 1) & 15]); }
#pragma unroll
  for (int k = 0; k < 16; ++k) { mn4[k] = min(mn2[k], mn2[(k + 2) & 15]); mx4[k] = max(mx2[k], mx2[(k + 2) & 15]); }
#pragma unroll
  for (int k = 0; k < 16; ++k) { mn8[k] = min(mn4[k], mn4[(k + 4) & 15]); mx8[k] = max(mx4[k], mx4[(k + 4) & 15]); }
  int best = -255;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    best = max(best, min(mn8[k], d[(k + 8) & 15]));        // min(ring - v) over the arc k .. k + 8
    best = max(best, -max(mx8[k], d[(k + 8) & 15]));       // min(v - ring)
  }
  return best;
}

__global__ __launch_bounds__(ORB_THREADS) void k_orb_fast(OrbArgs a, int l) {
  constexpr int PW = ORB_TILE_W + 8, PH = ORB_TILE_H + 8, SW = ORB_TILE_W + 2, SH = ORB_TILE_H + 2;
  __shared__ unsigned char pix[PH * PW];
  __shared__ unsigned char sc[SH * SW];
  __shared__ unsigned hist[256];
  const int w = a.w[l], h = a.h[l], b = blockIdx.z;
  const int tx0 = blockIdx.x * ORB_TILE_W, ty0 = blockIdx.y * ORB_TILE_H;
  const long long img = orb_img(a, l, b);
  const unsigned char* src = a.pyr + img;
  for (int e = threadIdx.x; e < PH * PW; e += ORB_THREADS) {
    const int gy = ty0 - 4 + e / PW, gx = tx0 - 4 + e % PW;
    pix[e] = (gx >= 0 && gx < w && gy >= 0 && gy < h) ? src[(long long)gy * w + gx] : (unsigned char)0;
  }
  hist[threadIdx.x] = 0;
  __syncthreads();
  for (int e = threadIdx.x; e < SH * SW; e += ORB_THREADS) {
    const int sy = e / SW, sx = e % SW;
    const int gy = ty0 - 1 + sy, gx = tx0 - 1 + sx;
    int s = 0;
    if (gx >= 3 && gx < w - 3 && gy >= 3 && gy < h - 3) s = orb_fast_score<PW>(pix + (sy + 3) * PW + sx + 3, a.thr);
    sc[e] = (unsigned char)(s > a.thr ? s : 0);
  }
  __syncthreads();
  for (int e = threadIdx.x; e < ORB_TILE_W * ORB_TILE_H; e += ORB_THREADS) {
    const int ly = e / ORB_TILE_W, lx = e % ORB_TILE_W;
    const int gy = ty0 + ly, gx = tx0 + lx;
    if (gx >= w || gy >= h) continue;
    const unsigned char* q = sc + (ly + 1) * SW + lx + 1;
    const int v = q[0];
    bool keep = v > 0 && gx >= a.edge && gx < w - a.edge && gy >= a.edge && gy < h - a.edge;
    keep = keep && v > q[-SW - 1] && v > q[-SW] && v > q[-SW + 1] && v > q[-1] && v > q[1] && v > q[SW - 1] && v > q[SW] && v > q[SW + 1];
    a.score[img + (long long)gy * w + gx] = (unsigned char)(keep ? v : 0);
    if (keep) atomicAdd(&hist[v], 1u);
  }
  __syncthreads();
  if (hist[threadIdx.x] != 0) atomicAdd(a.hist + ((size_t)b * a.n_levels + l) * 256 + threadIdx.x, hist[threadIdx.x]);
}

__global__ __launch_bounds__(64) void k_orb_cut(OrbArgs a) {
  __shared__ int ms[ORB_MAX_LEVELS];
  const int b = blockIdx.x, l = threadIdx.x;
  OrbCut c = {256, 0, 0, 0, 0};
  if (l < a.n_levels) {
    const unsigned* hh = a.hist + ((size_t)b * a.n_levels + l) * 256;
    long long total = 0;
    for (int s = 1; s < 256; ++s) total += hh[s];
    c.K = (int)min(total, (long long)2 * a.quota[l]);
    if (c.K > 0) {
      int acc = 0;
      for (int s = 255; s >= 1; --s) {      // the largest T with at least K candidates of score >= T
        if (acc + (long long)hh[s] >= c.K) { c.T = s; c.n_tie = c.K - acc; break; }
        acc += (int)hh[s];
      }
    }
    c.m = min(c.K, a.quota[l]);
    ms[l] = c.m;
  }
  __syncthreads();
  if (l < a.n_levels) {
    for (int j = 0; j < l; ++j) c.out0 += ms[j];
    c.out0 = min(c.out0, a.n_features);
    c.m = min(c.m, a.n_features - c.out0);      // (never binds: the quotas sum to n_features; no output row beyond the image's)
    a.cut[(size_t)b * a.n_levels + l] = c;
    if (l == a.n_levels - 1) a.n_kp[b] = c.out0 + c.m;
  }
}

__device__ __forceinline__ int orb_level_of_row(const OrbArgs& a, int R) {
  int l = 0;
  while (l + 1 < a.n_levels && R >= a.row0[l + 1]) ++l;
  return l;
}

__global__ __launch_bounds__(64) void k_orb_rowcount(OrbArgs a) {
  const int R = blockIdx.x, b = blockIdx.y;
  const int l = orb_level_of_row(a, R);
  const int y = R - a.row0[l], w = a.w[l], h = a.h[l];
  int ca = 0, cb = 0;
  if (y >= a.edge && y < h - a.edge) {          // (uniform over the wave)
    const int T = a.cut[(size_t)b * a.n_levels + l].T;
    const unsigned char* row = a.score + orb_img(a, l, b) + (long long)y * w;
    for (int x0 = a.edge; x0 < w - a.edge; x0 += 64) {
      const int x = x0 + (int)threadIdx.x;
      const int v = x < w - a.edge ? (int)row[x] : 0;
      ca += __popcll(__builtin_amdgcn_ballot_w64(v > T));
      cb += __popcll(__builtin_amdgcn_ballot_w64(v == T));
    }
  }
  if (threadIdx.x == 0) {
    a.row_a[(size_t)b * a.rows + R] = ca;
    a.row_b[(size_t)b * a.rows + R] = cb;
  }
}

// exclusive scan of one value per thread over the workgroup; total = the sum
__device__ __forceinline__ int orb_block_scan(int v, int* sh, int& total) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int o = 1; o < ORB_THREADS; o <<= 1) {
    const int add = t >= o ? sh[t - o] : 0;
    __syncthreads();
    sh[t] += add;
    __syncthreads();
  }
  const int incl = sh[t];
  total = sh[ORB_THREADS - 1];
  __syncthreads();
  return incl - v;
}

__global__ __launch_bounds__(ORB_THREADS) void k_orb_scan(OrbArgs a) {
  __shared__ int sh[ORB_THREADS];
  const int l = blockIdx.x, b = blockIdx.y;
  const int n_tie = a.cut[(size_t)b * a.n_levels + l].n_tie;
  int* ra = a.row_a + (size_t)b * a.rows + a.row0[l];
  int* rb = a.row_b + (size_t)b * a.rows + a.row0[l];
  int carry_tie = 0, carry_kept = 0;
  for (int y0 = 0; y0 < a.h[l]; y0 += ORB_THREADS) {
    const int y = y0 + (int)threadIdx.x;
    const bool live = y < a.h[l];
    const int ca = live ? ra[y] : 0, cb = live ? rb[y] : 0;
    int tot;
    const int tie0 = carry_tie + orb_block_scan(cb, sh, tot);
    carry_tie += tot;
    const int kept = ca + min(max(n_tie - tie0, 0), cb);
    const int pos0 = carry_kept + orb_block_scan(kept, sh, tot);
    carry_kept += tot;
    if (live) { ra[y] = pos0; rb[y] = tie0; }
  }
}

__global__ __launch_bounds__(64) void k_orb_compact(OrbArgs a) {
  const int R = blockIdx.x, b = blockIdx.y;
  const int l = orb_level_of_row(a, R);
  const int y = R - a.row0[l], w = a.w[l], h = a.h[l];
  if (y < a.edge || y >= h - a.edge) return;      // (uniform over the wave)
  const OrbCut c = a.cut[(size_t)b * a.n_levels + l];
  int pos = a.row_a[(size_t)b * a.rows + R], tie = a.row_b[(size_t)b * a.rows + R];
  const unsigned char* row = a.score + orb_img(a, l, b) + (long long)y * w;
  int* list = a.list + (size_t)b * a.list_cap + a.list0[l];
  const unsigned long long below = (1ull << threadIdx.x) - 1ull;
  for (int x0 = a.edge; x0 < w - a.edge; x0 += 64) {
    const int x = x0 + (int)threadIdx.x;
    const int v = x < w - a.edge ? (int)row[x] : 0;
    const unsigned long long mb = __builtin_amdgcn_ballot_w64(v == c.T);
    const bool keep = v > c.T || (v == c.T && tie + __popcll(mb & below) < c.n_tie);
    const unsigned long long mk = __builtin_amdgcn_ballot_w64(keep);
    const int at = pos + __popcll(mk & below);
    if (keep && at < c.K) list[at] = y * w + x;
    pos += __popcll(mk);
    tie += __popcll(mb);
  }
}

__global__ __launch_bounds__(ORB_THREADS) void k_orb_harris(OrbArgs a) {
  const int l = blockIdx.y, b = blockIdx.z;
  const int i = blockIdx.x * ORB_THREADS + threadIdx.x;
  if (i >= a.cut[(size_t)b * a.n_levels + l].K) return;
  const int w = a.w[l];
  const int r = a.list[(size_t)b * a.list_cap + a.list0[l] + i];
  const unsigned char* p = a.pyr + orb_img(a, l, b) + (long long)(r / w) * w + r % w;
  if (r < 4 * w + 4 || r >= (a.h[l] - 4) * w - 4) return;      // (never: a candidate lies edge >= 25 pixels inside; no read outside the image)
  // rows y - 4 .. y + 4; of each, over x - 3 .. x + 3: dh = I(x + 1) - I(x - 1) and sm = I(x - 1) + 2 I(x) + I(x + 1).
  // Ix(row) = dh(row - 1) + 2 dh(row) + dh(row + 1), Iy(row) = sm(row + 1) - sm(row - 1)
  int dh[3][7] = {}, sm[3][7] = {};
  int sa = 0, sb = 0, scc = 0;
#pragma unroll
  for (int ry = -4; ry <= 4; ++ry) {
    int px[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) px[k] = p[(long long)ry * w + (k - 4)];
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      dh[0][k] = dh[1][k]; dh[1][k] = dh[2][k]; dh[2][k] = px[k + 2] - px[k];
      sm[0][k] = sm[1][k]; sm[1][k] = sm[2][k]; sm[2][k] = px[k] + 2 * px[k + 1] + px[k + 2];
    }
    if (ry >= -2) {
#pragma unroll
      for (int k = 0; k < 7; ++k) {
        const int ix = dh[0][k] + 2 * dh[1][k] + dh[2][k], iy = sm[2][k] - sm[0][k];
        sa += ix * ix; sb += iy * iy; scc += ix * iy;
      }
    }
  }
  const long long A = sa, B = sb, C = scc;
  a.hs[(size_t)b * a.list_cap + a.list0[l] + i] = 25 * (A * B - C * C) - (A + B) * (A + B);
}

__global__ __launch_bounds__(ORB_THREADS) void k_orb_rank(OrbArgs a) {
#pragma clang fp contract(off)
  __shared__ long long t_hs[ORB_THREADS];
  __shared__ int t_r[ORB_THREADS];
  const int l = blockIdx.y, b = blockIdx.z;
  const OrbCut c = a.cut[(size_t)b * a.n_levels + l];
  if ((int)blockIdx.x * ORB_THREADS >= c.K) return;      // (uniform over the workgroup)
  const int i = blockIdx.x * ORB_THREADS + threadIdx.x;
  const int* list = a.list + (size_t)b * a.list_cap + a.list0[l];
  const long long* hs = a.hs + (size_t)b * a.list_cap + a.list0[l];
  const long long none = (long long)0x8000000000000000ULL;
  const long long hi = i < c.K ? hs[i] : none;
  const int ri = i < c.K ? list[i] : 0x7fffffff;
  int rank = 0;
  for (int j0 = 0; j0 < c.K; j0 += ORB_THREADS) {
    const int j = j0 + (int)threadIdx.x;
    __syncthreads();
    t_hs[threadIdx.x] = j < c.K ? hs[j] : none;
    t_r[threadIdx.x] = j < c.K ? list[j] : 0x7fffffff;
    __syncthreads();
    const int cnt = min(ORB_THREADS, c.K - j0);
    for (int t = 0; t < cnt; ++t) {
      const long long hj = t_hs[t];
      rank += (hj > hi || (hj == hi && t_r[t] < ri)) ? 1 : 0;
    }
  }
  if (i >= c.K || rank >= c.m) return;
  const int w = a.w[l], x = ri % w, y = ri / w;
  const size_t row = (size_t)b * a.n_features + c.out0 + rank;
  const double s = a.scale[l];
  a.octave[row] = l;
  a.level_xy[2 * row] = x;
  a.level_xy[2 * row + 1] = y;
  a.xy[2 * row] = (float)((double)x * s);
  a.xy[2 * row + 1] = (float)((double)y * s);
  a.size[row] = (float)(31.0 * s);
  a.response[row] = (float)(((double)hi / 25.0) / 2598919616160000.0);      // 7140^4
}

__global__ __launch_bounds__(ORB_THREADS) void k_orb_blur(OrbArgs a, int l) {
  constexpr int PW = ORB_TILE_W + 6, PH = ORB_TILE_H + 6;
  __shared__ unsigned char pix[PH * PW];
  __shared__ unsigned short tmp[PH * ORB_TILE_W];
  const int w = a.w[l], h = a.h[l];
  const int tx0 = blockIdx.x * ORB_TILE_W, ty0 = blockIdx.y * ORB_TILE_H;
  const long long img = orb_img(a, l, blockIdx.z);
  const unsigned char* src = a.pyr + img;
  for (int e = threadIdx.x; e < PH * PW; e += ORB_THREADS) {
    const int gy = ty0 - 3 + e / PW, gx = tx0 - 3 + e % PW;
    pix[e] = (gx >= 0 && gx < w && gy >= 0 && gy < h) ? src[(long long)gy * w + gx] : (unsigned char)0;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < PH * ORB_TILE_W; e += ORB_THREADS) {
    const unsigned char* q = pix + (e / ORB_TILE_W) * PW + e % ORB_TILE_W;
    tmp[e] = (unsigned short)(18 * q[0] + 34 * q[1] + 49 * q[2] + 54 * q[3] + 49 * q[4] + 34 * q[5] + 18 * q[6]);
  }
  __syncthreads();
  for (int e = threadIdx.x; e < ORB_TILE_H * ORB_TILE_W; e += ORB_THREADS) {
    const int ly = e / ORB_TILE_W, lx = e % ORB_TILE_W;
    const int gy = ty0 + ly, gx = tx0 + lx;
    if (gx < 3 || gx >= w - 3 || gy < 3 || gy >= h - 3) continue;       // within 3 pixels of a border: never read, not written
    const unsigned short* q = tmp + ly * ORB_TILE_W + lx;
    const unsigned v = 18u * q[0] + 34u * q[ORB_TILE_W] + 49u * q[2 * ORB_TILE_W] + 54u * q[3 * ORB_TILE_W] + 49u * q[4 * ORB_TILE_W] +
                       34u * q[5 * ORB_TILE_W] + 18u * q[6 * ORB_TILE_W];
    a.blur[img + (long long)gy * w + gx] = (unsigned char)((v + 32768u) >> 16);
  }
}

__device__ __forceinline__ int orb_umax(int v) {      // half-width of the circular patch's row |v|
  return v <= 3 ? 15 : v <= 6 ? 14 : v <= 8 ? 13 : v == 9 ? 12 : v == 10 ? 11 : v == 11 ? 10 : v == 12 ? 9 : v == 13 ? 8 : v == 14 ? 6 : 3;
}

__global__ __launch_bounds__(ORB_THREADS) void k_orb_describe(OrbArgs a) {
#pragma clang fp contract(off)
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int k = blockIdx.x * ORB_KP_PER_BLOCK + (threadIdx.x >> 6);
  if (k >= a.n_kp[b]) return;                        // (uniform over the wave; no barrier below)
  const size_t row = (size_t)b * a.n_features + k;
  const int l = a.octave[row], x = a.level_xy[2 * row], y = a.level_xy[2 * row + 1], w = a.w[l];
  if (x < 22 || x >= w - 22 || y < 22 || y >= a.h[l] - 22) return;      // (never: edge >= 25; the patch and the rotated tests reach 21 pixels)
  const long long at = orb_img(a, l, b) + (long long)y * w + x;
  const unsigned char* p = a.pyr + at;
  int m10 = 0, m01 = 0;
  const int u = (lane & 31) - 15;
  for (int v0 = -15; v0 <= 15; v0 += 2) {            // lanes 0 .. 31: patch row v0, lanes 32 .. 63: row v0 + 1
    const int v = v0 + (lane >> 5);
    if (v <= 15 && u <= 15 && abs(u) <= orb_umax(abs(v))) {
      const int I = p[(long long)v * w + u];
      m10 += u * I;
      m01 += v * I;
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    m10 += __shfl_xor(m10, o, 64);
    m01 += __shfl_xor(m01, o, 64);
  }
  double c = 1.0, s = 0.0;
  if (m10 != 0 || m01 != 0) {
    const double r = sqrt((double)((long long)m10 * m10 + (long long)m01 * m01));
    c = (double)m10 / r;
    s = (double)m01 / r;
  }
  if (lane == 0) {
    double deg = atan2((double)m01, (double)m10) * (180.0 / 3.141592653589793);
    if (deg < 0) deg = deg + 360.0;
    float f = (float)deg;
    if (f >= 360.0f) f = 0.0f;
    a.angle[row] = f;
    a.cs[2 * row] = c;
    a.cs[2 * row + 1] = s;
  }
  const unsigned char* B = a.blur + at;
  unsigned nib = 0;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const signed char* q = a.pattern + 4 * (4 * lane + t);
    const double x1 = (double)q[0], y1 = (double)q[1], x2 = (double)q[2], y2 = (double)q[3];
    const int u1 = (int)rint(x1 * c - y1 * s), v1 = (int)rint(x1 * s + y1 * c);
    const int u2 = (int)rint(x2 * c - y2 * s), v2 = (int)rint(x2 * s + y2 * c);
    nib |= (B[(long long)v1 * w + u1] < B[(long long)v2 * w + u2] ? 1u : 0u) << t;
  }
  const unsigned up = (unsigned)__shfl_down((int)nib, 1, 64);
  if ((lane & 1) == 0) a.desc[32 * row + (lane >> 1)] = (unsigned char)(nib | (up << 4));
}

}  // namespace ba
