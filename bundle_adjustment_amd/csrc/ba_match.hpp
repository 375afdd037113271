// Descriptor matching (ba_match_descriptors): brute-force Hamming 2-nearest-neighbours of binary descriptors with Lowe's ratio
// test (the reference's BruteForceMatcher.match: cv2.BFMatcher(NORM_HAMMING).knnMatch(des1, des2, k = 2), then m.distance <
// 0.75 n.distance).  Stand-alone kernels: they read the call's own staging buffers and nothing of a resident problem.
//
// A descriptor is W = desc_bytes / 8 words of 64 bits.  The train descriptors of a query are ordered by the key (d, j), d the
// popcount of the XOR and j the train index; the key is packed as d << 20 | j (d <= 512 takes ten bits, j < 2^20 twenty), so
// an unsigned min orders by (d, j) and ties go to the lower index.  0xffffffff is "no neighbour".  The two lowest keys seen
// so far are kept by k2 = min(k2, max(k1, key)), k1 = min(k1, key): keys of one query are distinct, so the pair (k1, k2) is the
// two lowest keys of the SET of keys fed in, whatever their order and grouping -- which is why the split count cannot show
// in the result.
//
// Two launches per call, for all pairs at once.  An ENTRY is one (query set, train set) of the pair table: the n_pairs pairs of
// the call, followed, with mutual = 1, by the same pairs with the roles swapped.
//   k_match_partial<W>  grid (entries, query blocks, train splits), MT_THREADS threads.  A lane holds one query in W 64-bit
//                       registers (W is a template parameter: no descriptor is indexed dynamically).  The split's train
//                       descriptors go through LDS in tiles of MT_TILE; in the distance loop every lane reads the same
//                       address (broadcast).  d = sum of popcount(q ^ t) over the words.  The (k1, k2) of the split goes to
//                       part[part0 + query * n_splits + split].
//   k_match_finish      grid (pairs, query blocks): lane = query.  Merges the splits' (k1, k2), unpacks best / second / dist1 /
//                       dist2, applies ratio (fp64, as written in the header), max_distance and mutual (the merged k1 of row
//                       `best` of the swapped entry must name this query), writes good and adds the workgroup's count to
//                       n_good[pair] (one integer atomicAdd per workgroup: order-independent).
//
// Split rule (host, ba_match_descriptors): see match_plan in ba_hip.hip and DESIGN.md 4m.
#pragma once
#include <hip/hip_runtime.h>

namespace ba {

constexpr int MT_THREADS = 256;        // queries per workgroup (B)
constexpr int MT_TILE = 64;            // train descriptors per LDS tile (T)
constexpr int MT_MIN_SPLIT = 128;      // a train split is never shorter than this unless it is the whole set (S); whole tiles
constexpr int MT_MAX_SPLITS = 64;
constexpr int MT_MAX_WORDS = 8;        // desc_bytes <= 64
constexpr int MT_IDX_BITS = 20;        // a set holds at most 2^20 descriptors
constexpr unsigned MT_IDX_MASK = (1u << MT_IDX_BITS) - 1;
constexpr unsigned MT_NONE = 0xffffffffu;
static_assert(MT_MIN_SPLIT % MT_TILE == 0 && ((8u * 8 * MT_MAX_WORDS) << MT_IDX_BITS) < MT_NONE, "whole tiles; the largest key is below MT_NONE");

struct MatchPair {        // one entry
  long long q0, t0;       // first descriptor row of the query / train set
  long long row0;         // first output row (row_off[pair]); unused by swapped entries
  long long part0;        // first (k1, k2) of the entry in `part`
  int nq, nt;
  int split_len;          // train descriptors per split, a multiple of MT_TILE
  int n_splits;           // ceil(nt / split_len); 0 when nt = 0
};

struct MatchArgs {
  const unsigned long long* desc;   // every set, W words per row
  const MatchPair* pairs;           // [n_pairs] or, with mutual, [2 n_pairs]
  uint2* part;
  int n_pairs, mutual, max_distance;
  double ratio;
  int* best;                        // [rows] each
  int* second;
  int* dist1;
  int* dist2;
  unsigned char* good;              // [rows]
  int* n_good;                      // [n_pairs], zeroed before the launch
};

__device__ __forceinline__ void mt_push(unsigned& k1, unsigned& k2, unsigned key) {
  k2 = min(k2, max(k1, key));
  k1 = min(k1, key);
}

template <int W>
__global__ __launch_bounds__(MT_THREADS) void k_match_partial(MatchArgs a) {
  const MatchPair pr = a.pairs[blockIdx.x];
  const int s = blockIdx.z;
  if ((long long)blockIdx.y * MT_THREADS >= pr.nq || s >= pr.n_splits) return;   // (uniform over the workgroup)
  __shared__ __attribute__((aligned(16))) unsigned long long tile[MT_TILE * W];
  const int i = blockIdx.y * MT_THREADS + threadIdx.x;
  const bool live = i < pr.nq;
  unsigned long long q[W];
#pragma unroll
  for (int w = 0; w < W; ++w) q[w] = live ? a.desc[(pr.q0 + i) * W + w] : 0ull;
  unsigned k1 = MT_NONE, k2 = MT_NONE;
  const int j_begin = s * pr.split_len, j_end = min(pr.nt, j_begin + pr.split_len);
  for (int j0 = j_begin; j0 < j_end; j0 += MT_TILE) {
    const int cnt = min(MT_TILE, j_end - j0);
    const unsigned long long* src = a.desc + (pr.t0 + j0) * W;
    __syncthreads();
    for (int e = threadIdx.x; e < cnt * W; e += MT_THREADS) tile[e] = src[e];
    __syncthreads();
#pragma unroll 4
    for (int t = 0; t < cnt; ++t) {
      unsigned d = 0;
#pragma unroll
      for (int w = 0; w < W; ++w) d += (unsigned)__popcll(q[w] ^ tile[t * W + w]);
      mt_push(k1, k2, (d << MT_IDX_BITS) | (unsigned)(j0 + t));
    }
  }
  if (live) a.part[pr.part0 + (long long)i * pr.n_splits + s] = make_uint2(k1, k2);
}

// the two lowest keys over the n splits of one query
__device__ __forceinline__ void mt_merge(const uint2* p, int n, unsigned& k1, unsigned& k2) {
  k1 = k2 = MT_NONE;
  for (int s = 0; s < n; ++s) {
    const uint2 v = p[s];
    mt_push(k1, k2, v.x);
    mt_push(k1, k2, v.y);
  }
}

__global__ __launch_bounds__(MT_THREADS) void k_match_finish(MatchArgs a) {
  const MatchPair pr = a.pairs[blockIdx.x];
  if ((long long)blockIdx.y * MT_THREADS >= pr.nq) return;   // (uniform over the workgroup)
  const int i = blockIdx.y * MT_THREADS + threadIdx.x;
  bool good = false;
  if (i < pr.nq) {
    unsigned k1, k2;
    mt_merge(a.part + pr.part0 + (long long)i * pr.n_splits, pr.n_splits, k1, k2);
    const int b = k1 == MT_NONE ? -1 : (int)(k1 & MT_IDX_MASK), d1 = k1 == MT_NONE ? -1 : (int)(k1 >> MT_IDX_BITS);
    const int c = k2 == MT_NONE ? -1 : (int)(k2 & MT_IDX_MASK), d2 = k2 == MT_NONE ? -1 : (int)(k2 >> MT_IDX_BITS);
    good = b >= 0;
    if (a.ratio > 0.0) good = good && c >= 0 && (double)d1 < a.ratio * (double)d2;
    if (a.max_distance >= 0) good = good && d1 <= a.max_distance;
    if (a.mutual && good) {
      const MatchPair rv = a.pairs[a.n_pairs + blockIdx.x];   // queries: this pair's train set
      unsigned r1, r2;
      mt_merge(a.part + rv.part0 + (long long)b * rv.n_splits, rv.n_splits, r1, r2);
      good = (int)(r1 & MT_IDX_MASK) == i;
    }
    const long long row = pr.row0 + i;
    a.best[row] = b;
    a.second[row] = c;
    a.dist1[row] = d1;
    a.dist2[row] = d2;
    a.good[row] = good ? 1 : 0;
  }
  const int n = __syncthreads_count(good);
  if (threadIdx.x == 0 && n > 0) atomicAdd(a.n_good + blockIdx.x, n);
}

}  // namespace ba
