// L2 descriptor matching (ba_match_l2): exact brute-force 2-nearest-neighbours of uint8 descriptors (SIFT / RootSIFT as COLMAP
// stores them, quantised learned descriptors) under the squared Euclidean distance, on the integer matrix cores.  Surface,
// entries, splits and the finish are ba_match_descriptors' (ba_match.hpp); only the metric and the partial kernel differ.
//
// Arithmetic.  With x' = x ^ 0x80 read as int8 (x - 128): d(q, t) = |q'|^2 + |t'|^2 - 2 q'.t'.  A byte difference is unchanged
// by the common shift, so this IS sum (q - t)^2; every term is exact in int32 (|q'.t'| <= 256 * 128^2 = 2^22).  The MFMA is fed
// the train side as t' and the query side as q" = q ^ 0x7f read as int8 (127 - q = -q' - 1, which stays in int8 where -q' does
// not), so its result is a = t'.q" = -q'.t' - sum t' and d = |q'|^2 + (|t'|^2 + 2 sum t') + 2 a: the dot product enters with a
// plus sign.  k_l2_norms gives |x'|^2 and |x'|^2 + 2 sum x' of every row of the call, once; v_mfma_i32_32x32x32_i8 gives a.
//
// Layout of one MFMA.  A = 32 train rows (the rows of C), B = 32 queries (the columns of C), k = 32 bytes.  Lane l = (r = l & 31,
// h = l >> 5) loads bytes 32 s + 16 h .. + 15 of row r for k-step s, for A and for B alike: a dot product does not change under a
// common permutation of k, so the result does not rest on the i8 A/B k-map, only on the C map, col = lane & 31, row = (reg & 3)
// + 8 (reg >> 2) + 4 (lane >> 5).  A lane therefore holds 16 train rows of ONE query in its accumulators, and the running pair of
// that query stays in the lane; lanes l and l + 32 hold the same query and are merged once, at the end of the split.
//
// The key.  Selection, not the MFMA, is the cost (16 results per lane follow every W MFMAs), so a result takes three VALU
// instructions.  Train rows are numbered within a CHUNK of 2^IB rows of the split (IB = ml_idx_bits(W)); with the row's
// base = (|t'|^2 + 2 sum t') << IB | local j staged next to the tile,
//     key = (a << (IB + 1)) + base                  (one v_lshl_add_u32)
// is (d - |q'|^2) << IB | local j as a SIGNED int32: it orders one query's rows of one chunk by (d, j), since |q'|^2 is the
// lane's constant.  d - |q'|^2 = |t'|^2 - 2 q'.t' lies in (-2^n, 2^n) with 2^n > 3 * 32 W * 2^14, and IB = 31 - n.  The two
// lowest keys are kept by k2 = med3(k1, k2, key), k1 = min(k1, key) (k1 <= k2: the median is the second lowest); INT_MAX is
// "no neighbour" and the base of a padded row, whose descriptor is staged as zeros, so its key is INT_MAX exactly.
// Once per chunk the pair is unpacked, |q'|^2 added, and folded as the 64-bit key d << 20 | j (j the index in the train set)
// into the split's pair with mt_push's min / max; keys of one query are distinct, so the result is the two lowest of the SET of
// keys, whatever the tile, chunk and split geometry.  ~0 is "no neighbour".
//
//   k_l2_norms          one thread per descriptor row of the call: |x'|^2 and |x'|^2 + 2 sum x', and the row shifted in place.
//   k_l2_partial<W>     grid (entries, query blocks of ML_BLOCK, train splits), ML_THREADS threads = four waves of 32 queries, the
//                       queries in registers (W = desc_bytes / 32 is a template parameter: nothing is indexed dynamically).
//                       The split's train rows go through LDS in tiles of ML_TILE, rows 16 bytes apart from a bank multiple,
//                       with their bases, in two buffers: one barrier per tile, and a tile's loads fly for a whole tile.  The (k1, k2) of the split goes to part[part0 + query * n_splits + split].
//   k_l2_finish         k_match_finish on the 64-bit keys, the ratio test on the squares.
#pragma once
#include <hip/hip_runtime.h>

#include "ba_match.hpp"

namespace ba {

constexpr int ML_THREADS = 256;
constexpr int ML_BLOCK = 128;          // queries per workgroup (B): 32 per wave
constexpr int ML_TILE = 64;            // train descriptors per LDS tile (T): two MFMA row blocks
constexpr int ML_MIN_SPLIT = 256;      // a train split is never shorter than this unless it is the whole set (S); whole tiles
constexpr int ML_MAX_W = 8;            // desc_bytes <= 256
constexpr int ML_NONE = 0x7fffffff;
constexpr unsigned long long ML_NONE64 = ~0ull;
// index bits of the 32-bit key for descriptors of 32 W bytes: the chunk is 2^ml_idx_bits(W) train rows
constexpr int ml_idx_bits(int W) {
  int n = 0;
  while ((3ll * 32 * W << 14) > (1ll << n)) ++n;
  return 31 - n;
}
static_assert(ml_idx_bits(1) == 10 && ml_idx_bits(4) == 8 && ml_idx_bits(ML_MAX_W) == 7, "chunks of 1024 .. 128 rows");
static_assert((1 << ml_idx_bits(ML_MAX_W)) % ML_TILE == 0 && ML_MIN_SPLIT % ML_TILE == 0 && ML_TILE % 32 == 0 && ML_BLOCK * 2 == ML_THREADS,
              "whole tiles in a chunk and in a split; 32 queries per wave");
static_assert(32ll * ML_MAX_W * 255 * 255 < (1ll << 24), "the distance and a 20-bit index share a 64-bit key with room to spare");

typedef int ml_v4i __attribute__((ext_vector_type(4)));
typedef int ml_v16i __attribute__((ext_vector_type(16)));

struct L2Args {
  MatchArgs m;                 // m.part holds two 64-bit keys per (query, split): see l2_part
  const int* norm;             // |x'|^2 of every descriptor row of the call (the row as a query)
  const int* tbase;            // |x'|^2 + 2 sum x' (the row as a train descriptor)
};
__device__ __forceinline__ ulonglong2* l2_part(const MatchArgs& m) { return (ulonglong2*)m.part; }

// One thread per descriptor row of the call: the row shifted in place (x' = x ^ 0x80: the call's own copy, which no other call
// reads), |x'|^2 and |x'|^2 + 2 sum x'
__global__ __launch_bounds__(256) void k_l2_norms(uint4* desc, int* norm, int* tbase, long long n_rows, int vec_per_row) {
  const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
  if (row >= n_rows) return;
  int sum = 0, lin = 0;
  for (int c = 0; c < vec_per_row; ++c) {
    uint4 v = desc[row * vec_per_row + c];
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int x = (int)((w[e] >> (8 * b)) & 0xffu) - 128;
        sum += x * x;
        lin += x;
      }
    v.x ^= 0x80808080u; v.y ^= 0x80808080u; v.z ^= 0x80808080u; v.w ^= 0x80808080u;
    desc[row * vec_per_row + c] = v;
  }
  norm[row] = sum;
  tbase[row] = sum + 2 * lin;
}

__device__ __forceinline__ void ml_push(int& k1, int& k2, int key) {
  asm("v_med3_i32 %0, %1, %2, %3" : "=v"(k2) : "v"(k1), "v"(k2), "v"(key));
  k1 = min(k1, key);
}
__device__ __forceinline__ void ml_push64(unsigned long long& k1, unsigned long long& k2, unsigned long long key) {
  k2 = min(k2, max(k1, key));
  k1 = min(k1, key);
}
// a chunk's key as the split's: d = (key >> IB) + |q'|^2, j = the chunk's first row + the key's local index
template <int IB>
__device__ __forceinline__ unsigned long long ml_widen(int key, int qn, int chunk_j0) {
  const unsigned long long d = (unsigned)((key >> IB) + qn), j = (unsigned)(chunk_j0 + (key & ((1 << IB) - 1)));
  return key == ML_NONE ? ML_NONE64 : (d << MT_IDX_BITS) | j;
}

// (the waves per SIMD asked for keep the kernel within 256 registers, where the compiler leaves the accumulators in VGPRs, which the
// VALU reads directly, and within the register count of the occupancy each width reaches anyway)
template <int W>
__global__ __launch_bounds__(ML_THREADS, W <= 2 ? 7 : W <= 4 ? 6 : W <= 6 ? 5 : 4) void k_l2_partial(L2Args a) {
  constexpr int D = 32 * W, ROW = D + 16, VEC = 2 * W, IB = ml_idx_bits(W), CHUNK = 1 << IB;
  constexpr int NV = (ML_TILE * VEC + ML_THREADS - 1) / ML_THREADS;              // 16-byte vectors of a tile per thread
  const MatchPair pr = a.m.pairs[blockIdx.x];
  const int s = blockIdx.z;
  if ((long long)blockIdx.y * ML_BLOCK >= pr.nq || s >= pr.n_splits) return;   // (uniform over the workgroup)
  __shared__ __attribute__((aligned(16))) unsigned char tiles[2][ML_TILE * ROW];     // the tile computed on and the one staged next
  __shared__ __attribute__((aligned(16))) int bases[2][ML_TILE];
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int i = blockIdx.y * ML_BLOCK + (threadIdx.x >> 6) * 32 + r;
  const bool live = i < pr.nq;
  const uint4* desc = (const uint4*)a.m.desc;                 // rows of x' (k_l2_norms shifted them in place)
  const uint4* qrow = desc + (pr.q0 + min(i, pr.nq - 1)) * VEC + h;   // a padded query computes on the last row and writes nothing
  ml_v4i q[W];
#pragma unroll
  for (int k = 0; k < W; ++k) {
    const uint4 v = qrow[2 * k];
    q[k] = ml_v4i{(int)~v.x, (int)~v.y, (int)~v.z, (int)~v.w};                    // q" = q ^ 0x7f = ~q'
  }
  const int qn = a.norm[pr.q0 + min(i, pr.nq - 1)];
  int k1 = ML_NONE, k2 = ML_NONE;
  unsigned long long g1 = ML_NONE64, g2 = ML_NONE64;
  const int j_begin = s * pr.split_len, j_end = min(pr.nt, j_begin + pr.split_len);
  // Tile n + 1 is staged into the other LDS buffer before tile n is computed on, from registers it was fetched into during
  // tile n - 1: a load has a whole tile to land, and ONE barrier per tile says both that buffer n & 1 has been read and that
  // buffer (n + 1) & 1 has been written.  A padded row is staged as zeros: its dot product is 0, and its base ML_NONE is its key.
  uint4 pv[NV];
  int pb = 0;
  auto fetch = [&](int j0) {
    const int cnt = min(ML_TILE, j_end - j0);
    const uint4* src = desc + (pr.t0 + j0) * VEC;
#pragma unroll
    for (int n = 0; n < NV; ++n) {
      const int e = threadIdx.x + n * ML_THREADS;
      pv[n] = make_uint4(0u, 0u, 0u, 0u);
      if (e < cnt * VEC) pv[n] = src[e];
    }
    if ((int)threadIdx.x < cnt) pb = a.tbase[pr.t0 + j0 + threadIdx.x];
  };
  auto stage = [&](int j0, int buf) {
    const int cnt = min(ML_TILE, j_end - j0);
#pragma unroll
    for (int n = 0; n < NV; ++n) {
      const int e = threadIdx.x + n * ML_THREADS;
      if (NV * ML_THREADS == ML_TILE * VEC || e < ML_TILE * VEC) *(uint4*)(tiles[buf] + (e / VEC) * ROW + 16 * (e % VEC)) = pv[n];
    }
    if (threadIdx.x < ML_TILE)
      bases[buf][threadIdx.x] = (int)threadIdx.x < cnt ? (pb << IB) | (((j0 - j_begin) & (CHUNK - 1)) + (int)threadIdx.x) : ML_NONE;
  };
  fetch(j_begin);
  stage(j_begin, 0);
  if (j_begin + ML_TILE < j_end) fetch(j_begin + ML_TILE);
  __syncthreads();
  int buf = 0;
  for (int j0 = j_begin; j0 < j_end; j0 += ML_TILE, buf ^= 1) {
    const int cnt = min(ML_TILE, j_end - j0);
    const int local0 = (j0 - j_begin) & (CHUNK - 1);          // the tile's first row within its chunk
    if (j0 + ML_TILE < j_end) stage(j0 + ML_TILE, buf ^ 1);
    if (j0 + 2 * ML_TILE < j_end) fetch(j0 + 2 * ML_TILE);
    const unsigned char* tile = tiles[buf];
    const int* base = bases[buf];
#pragma unroll
    for (int sub = 0; sub < ML_TILE / 32; ++sub) {
      if (sub * 32 >= cnt) break;                             // (uniform over the workgroup)
      ml_v16i acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
      for (int k = 0; k < W; ++k) {
        const ml_v4i t = *(const ml_v4i*)(tile + (sub * 32 + r) * ROW + 32 * k + 16 * h);
        acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(t, q[k], acc, 0, 0, 0);
      }
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const ml_v4i b = *(const ml_v4i*)(base + sub * 32 + 8 * g + 4 * h);     // rows 8 g + 4 h + (0 .. 3) of the block
#pragma unroll
        for (int e = 0; e < 4; ++e) ml_push(k1, k2, (acc[4 * g + e] << (IB + 1)) + b[e]);
      }
    }
    if (local0 + ML_TILE == CHUNK || j0 + ML_TILE >= j_end) {  // the chunk ends with this tile
      ml_push64(g1, g2, ml_widen<IB>(k1, qn, j0 - local0));
      ml_push64(g1, g2, ml_widen<IB>(k2, qn, j0 - local0));
      k1 = k2 = ML_NONE;
    }
    __syncthreads();
  }
  // the other half of the rows of this query
  const unsigned long long o1 = __shfl_xor(g1, 32), o2 = __shfl_xor(g2, 32);
  ml_push64(g1, g2, o1);
  ml_push64(g1, g2, o2);
  if (live && h == 0) l2_part(a.m)[pr.part0 + (long long)i * pr.n_splits + s] = make_ulonglong2(g1, g2);
}

// the two lowest keys over the n splits of one query
__device__ __forceinline__ void ml_merge(const ulonglong2* p, int n, unsigned long long& k1, unsigned long long& k2) {
  k1 = k2 = ML_NONE64;
  for (int s = 0; s < n; ++s) {
    const ulonglong2 v = p[s];
    ml_push64(k1, k2, v.x);
    ml_push64(k1, k2, v.y);
  }
}

__global__ __launch_bounds__(MT_THREADS) void k_l2_finish(L2Args args) {
  const MatchArgs& a = args.m;
  const MatchPair pr = a.pairs[blockIdx.x];
  if ((long long)blockIdx.y * MT_THREADS >= pr.nq) return;   // (uniform over the workgroup)
  const int i = blockIdx.y * MT_THREADS + threadIdx.x;
  bool good = false;
  if (i < pr.nq) {
    unsigned long long k1, k2;
    ml_merge(l2_part(a) + pr.part0 + (long long)i * pr.n_splits, pr.n_splits, k1, k2);
    const int b = k1 == ML_NONE64 ? -1 : (int)(k1 & MT_IDX_MASK), d1 = k1 == ML_NONE64 ? -1 : (int)(k1 >> MT_IDX_BITS);
    const int c = k2 == ML_NONE64 ? -1 : (int)(k2 & MT_IDX_MASK), d2 = k2 == ML_NONE64 ? -1 : (int)(k2 >> MT_IDX_BITS);
    good = b >= 0;
    if (a.ratio > 0.0) good = good && c >= 0 && (double)d1 < (a.ratio * a.ratio) * (double)d2;
    if (a.max_distance >= 0) good = good && d1 <= a.max_distance;
    if (a.mutual && good) {
      const MatchPair rv = a.pairs[a.n_pairs + blockIdx.x];   // queries: this pair's train set
      unsigned long long r1, r2;
      ml_merge(l2_part(a) + rv.part0 + (long long)b * rv.n_splits, rv.n_splits, r1, r2);
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
