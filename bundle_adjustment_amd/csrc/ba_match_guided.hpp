// Guided descriptor matching (ba_match_guided): the Hamming 2-NN of ba_match.hpp over the train rows a geometric GATE admits.
// gate(i, j) is a predicate of query row i and train row j of a pair, evaluated in fp64 with every operation rounded on its own
// (`#pragma clang fp contract(off)` where it is computed: hipcc contracts a * b + c into v_fma_f64 / v_fmac_f64 by default, and
// did so through __dmul_rn / __dadd_rn too; the ISA of every instantiation has v_mul_f64 / v_add_f64 only), so that numpy's
// float64 decides every case identically, border cases included (include/ba_hip.h has the contract).
//
// A query's side of the gate is prepared once per query, as a RECORD of four doubles:
//   WINDOW     (px, py, rr, 0)      rr = r >= 0 ? r * r : NaN                      pass iff dx dx + dy dy <= rr
//   EPIPOLAR   (l0, l1, l2, thr)    thr = n > 0 ? (max_epi_px^2) n : NaN           pass iff e e <= thr, e = (l0 x + l1 y) + l2
// A comparison with NaN is false, so the NaN stands for the first half of the header's conjunction (r >= 0, n > 0) and for
// every non-finite input.  The train row's side is its keypoint (x, y), float32 widened to double (exact).
//
// Three launches per call, for all pairs at once; entries as in ba_match.hpp (the pairs, then with mutual the swapped pairs):
//   k_guided_prepare             grid (pairs, query blocks): lane = query, writes rec[row0 + i].
//   k_guided_partial<W, G>       grid (entries, query blocks, train splits), the structure of k_match_partial<W>.  In an entry
//                                of the call a lane holds its query's descriptor and record, and the tile carries the train
//                                rows' descriptors and keypoints; in a swapped entry a lane holds a train row's descriptor and
//                                keypoint and the tile carries the queries' descriptors and RECORDS: the same predicate with
//                                the same operands, not a second one.  Which of the two an entry is, is uniform over the
//                                workgroup; the gate kind G is a template parameter.  Per tile row the gate comes first; the
//                                popcounts run only if some lane of the wave admits the row (a wave-uniform branch on the
//                                ballot), and a lane that does not admit it pushes no key.  The split's (k1, k2) goes to part,
//                                its count of admitted rows to cnt (same index).
//   k_guided_finish              k_match_finish with the `single` rule and n_cand = the sum of the splits' counts.
#pragma once
#include <hip/hip_runtime.h>

#include "ba_linalg.hpp"
#include "ba_match.hpp"

namespace ba {

constexpr int MG_WINDOW = 1, MG_EPIPOLAR = 2;   // enum BA_GATE_* (include/ba_hip.h)

struct GuidedArgs {
  MatchArgs m;              // pairs: a swapped entry's row0 is its pair's row0 (the rows of the records its tile carries)
  const float* xy;          // [descriptor rows][2]
  const float* window;      // WINDOW: [rows][3]
  const double* F;          // EPIPOLAR: [n_pairs][9]
  double max_epi2;          // max_epi_px * max_epi_px
  double* rec;              // [rows][4]
  int* cnt;                 // admitted train rows per (query, split), indexed as part; entries of the call only
  int* n_cand;              // [rows]
  int gate, single;
};

__global__ __launch_bounds__(MT_THREADS) void k_guided_prepare(GuidedArgs a) {
#pragma clang fp contract(off)
  const MatchPair pr = a.m.pairs[blockIdx.x];
  const int i = blockIdx.y * MT_THREADS + threadIdx.x;
  if (i >= pr.nq) return;
  const long long row = pr.row0 + i;
  const double nan = HY_NAN;
  double r0, r1, r2, r3;
  if (a.gate == MG_WINDOW) {
    const double r = (double)a.window[3 * row + 2];
    r0 = (double)a.window[3 * row];
    r1 = (double)a.window[3 * row + 1];
    r2 = r >= 0.0 ? r * r : nan;
    r3 = 0.0;
  } else {
    const double* F = a.F + 9 * blockIdx.x;
    const double x1 = (double)a.xy[2 * (pr.q0 + i)], y1 = (double)a.xy[2 * (pr.q0 + i) + 1];
    r0 = (F[0] * x1 + F[1] * y1) + F[2];
    r1 = (F[3] * x1 + F[4] * y1) + F[5];
    r2 = (F[6] * x1 + F[7] * y1) + F[8];
    const double n = r0 * r0 + r1 * r1;
    r3 = n > 0.0 ? a.max_epi2 * n : nan;
  }
  double* o = a.rec + 4 * row;
  o[0] = r0; o[1] = r1; o[2] = r2; o[3] = r3;
}

// gate(i, j) from the record of query i and the keypoint of train row j
template <int G>
__device__ __forceinline__ bool mg_gate(double r0, double r1, double r2, double r3, double x, double y) {
#pragma clang fp contract(off)
  if (G == MG_WINDOW) {
    const double dx = x - r0, dy = y - r1;
    return dx * dx + dy * dy <= r2;
  } else {
    const double e = (r0 * x + r1 * y) + r2;
    return e * e <= r3;
  }
}

// One entry's split for one lane.  SW = false: the lane's side is a record, the tile's side keypoints (two doubles per row);
// SW = true: the lane's side is a keypoint (in r0, r1), the tile's side records (four doubles per row).
template <int W, int G, bool SW>
__device__ __forceinline__ void mg_scan(const GuidedArgs& a, const MatchPair& pr, unsigned long long* tile, double* gtile) {
  constexpr int GW = SW ? 4 : 2;
  const int s = blockIdx.z;
  const int i = blockIdx.y * MT_THREADS + threadIdx.x;
  const bool live = i < pr.nq;
  const double nan = HY_NAN;
  unsigned long long q[W];
#pragma unroll
  for (int w = 0; w < W; ++w) q[w] = live ? a.m.desc[(pr.q0 + i) * W + w] : 0ull;
  double r0 = nan, r1 = nan, r2 = nan, r3 = nan;     // a lane without a query admits nothing
  if (live) {
    if (SW) {
      r0 = (double)a.xy[2 * (pr.q0 + i)];
      r1 = (double)a.xy[2 * (pr.q0 + i) + 1];
    } else {
      const double* rc = a.rec + 4 * (pr.row0 + i);
      r0 = rc[0]; r1 = rc[1]; r2 = rc[2]; r3 = rc[3];
    }
  }
  unsigned k1 = MT_NONE, k2 = MT_NONE;
  int n_adm = 0;
  const int j_begin = s * pr.split_len, j_end = min(pr.nt, j_begin + pr.split_len);
  for (int j0 = j_begin; j0 < j_end; j0 += MT_TILE) {
    const int cnt = min(MT_TILE, j_end - j0);
    const unsigned long long* src = a.m.desc + (pr.t0 + j0) * W;
    __syncthreads();
    for (int e = threadIdx.x; e < cnt * W; e += MT_THREADS) tile[e] = src[e];
    if (SW) {
      const double* g = a.rec + 4 * (pr.row0 + j0);
      for (int e = threadIdx.x; e < cnt * 4; e += MT_THREADS) gtile[e] = g[e];
    } else {
      const float* g = a.xy + 2 * (pr.t0 + j0);
      for (int e = threadIdx.x; e < cnt * 2; e += MT_THREADS) gtile[e] = (double)g[e];
    }
    __syncthreads();
    for (int t = 0; t < cnt; ++t) {
      const double* g = gtile + t * GW;
      const bool pass = SW ? mg_gate<G>(g[0], g[1], g[2], g[3], r0, r1) : mg_gate<G>(r0, r1, r2, r3, g[0], g[1]);
      if (__builtin_amdgcn_ballot_w64(pass) != 0ull) {   // (uniform over the wave)
        unsigned d = 0;
#pragma unroll
        for (int w = 0; w < W; ++w) d += (unsigned)__popcll(q[w] ^ tile[t * W + w]);
        mt_push(k1, k2, pass ? ((d << MT_IDX_BITS) | (unsigned)(j0 + t)) : MT_NONE);
        n_adm += pass ? 1 : 0;
      }
    }
  }
  if (live) {
    const long long at = pr.part0 + (long long)i * pr.n_splits + s;
    a.m.part[at] = make_uint2(k1, k2);
    if (!SW) a.cnt[at] = n_adm;
  }
}

template <int W, int G>
__global__ __launch_bounds__(MT_THREADS) void k_guided_partial(GuidedArgs a) {
  const MatchPair pr = a.m.pairs[blockIdx.x];
  if ((long long)blockIdx.y * MT_THREADS >= pr.nq || (int)blockIdx.z >= pr.n_splits) return;   // (uniform over the workgroup)
  __shared__ __attribute__((aligned(16))) unsigned long long tile[MT_TILE * W];
  __shared__ __attribute__((aligned(16))) double gtile[MT_TILE * 4];
  if ((int)blockIdx.x >= a.m.n_pairs) mg_scan<W, G, true>(a, pr, tile, gtile);
  else mg_scan<W, G, false>(a, pr, tile, gtile);
}

__global__ __launch_bounds__(MT_THREADS) void k_guided_finish(GuidedArgs a) {
  const MatchPair pr = a.m.pairs[blockIdx.x];
  if ((long long)blockIdx.y * MT_THREADS >= pr.nq) return;   // (uniform over the workgroup)
  const int i = blockIdx.y * MT_THREADS + threadIdx.x;
  bool good = false;
  if (i < pr.nq) {
    const long long at = pr.part0 + (long long)i * pr.n_splits;
    unsigned k1, k2;
    mt_merge(a.m.part + at, pr.n_splits, k1, k2);
    int n_cand = 0;
    for (int s = 0; s < pr.n_splits; ++s) n_cand += a.cnt[at + s];
    const int b = k1 == MT_NONE ? -1 : (int)(k1 & MT_IDX_MASK), d1 = k1 == MT_NONE ? -1 : (int)(k1 >> MT_IDX_BITS);
    const int c = k2 == MT_NONE ? -1 : (int)(k2 & MT_IDX_MASK), d2 = k2 == MT_NONE ? -1 : (int)(k2 >> MT_IDX_BITS);
    good = b >= 0;
    if (a.m.ratio > 0.0) good = good && (c >= 0 ? (double)d1 < a.m.ratio * (double)d2 : a.single != 0);
    if (a.m.max_distance >= 0) good = good && d1 <= a.m.max_distance;
    if (a.m.mutual && good) {
      const MatchPair rv = a.m.pairs[a.m.n_pairs + blockIdx.x];   // queries: this pair's train set, under the same gate
      unsigned r1, r2;
      mt_merge(a.m.part + rv.part0 + (long long)b * rv.n_splits, rv.n_splits, r1, r2);
      good = (int)(r1 & MT_IDX_MASK) == i;
    }
    const long long row = pr.row0 + i;
    a.m.best[row] = b;
    a.m.second[row] = c;
    a.m.dist1[row] = d1;
    a.m.dist2[row] = d2;
    a.m.good[row] = good ? 1 : 0;
    a.n_cand[row] = n_cand;
  }
  const int n = __syncthreads_count(good);
  if (threadIdx.x == 0 && n > 0) atomicAdd(a.m.n_good + blockIdx.x, n);
}

}  // namespace ba
