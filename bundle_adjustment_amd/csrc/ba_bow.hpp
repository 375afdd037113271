// Place recognition (ba_vocab_train, ba_bow_transform, ba_bow_score): a binary vocabulary tree trained by hierarchical
// k-majority, one sparse L1-normalised bag-of-words vector per descriptor set, and the L1 score between vectors (DBoW2's, as
// used by ORB-SLAM's loop detection and COLMAP's vocabulary-tree matcher).  Stand-alone kernels: they read the call's own
// staging buffers and the vocabulary resident on the handle, nothing of a resident problem.  Integer arithmetic throughout:
// sums go through integer atomics, so no result depends on the order, the grid or the tiles.
//
// A descriptor is W = desc_bytes / 8 words of 64 bits (a template parameter, as in ba_match.hpp).  A row is assigned by the key
// d << 5 | slot, d the popcount of the XOR against a centre: an unsigned min orders by (d, slot).
//
// Training runs level by level over all nodes of a depth at once; `perm` keeps the rows ordered by node (rebuilt per level by a
// counting scatter, order within a node free), so a tile of BW_THREADS positions touches few nodes.  Per level:
//   k_vocab_seed_key   every member row offers the key (draw & ~0xFFFFFF) | row to each of its node's k slots (64-bit atomicMin;
//                      a workgroup whose rows all sit in one node folds the keys per wave first).
//   k_vocab_seed_set   per (node, slot): the winning row's descriptor becomes the centre; a slot whose row an earlier slot of
//                      the node drew is void (takes part in no assignment, stays empty).
//   k_vocab_assign<W>  lane = row: nearest usable centre of its node (centres read from global memory: neighbouring lanes read
//                      the same node's), slot written, slot sizes and the level's count of changed rows by integer atomics.
//   k_vocab_vote<W>    workgroup = tile of BW_THREADS positions staged in LDS, lane b = bit column b (two columns per lane for
//                      W > 4).  A lane owns its counters [slot][b] in LDS (no LDS atomics) and flushes the non-zero ones with
//                      global atomicAdd whenever the node changes along the tile: k * 64 W atomics per (tile, node) instead of
//                      64 W per row.
//   k_vocab_centre     per (node, slot, word): bit = 2 votes >= size for a non-empty slot.
//   k_vocab_children   lane = row: node <- the child its slot became (the host numbers the children from the slot sizes).
//   k_vocab_scatter    perm of the next level from per-node cursors.
// The transform: k_bow_descend<W> (lane = row, walks the tree), k_bow_count (dense per-set word counts), k_bow_vector (workgroup
// = set: A, then the ordered compaction of the non-zero entries).  The score: k_bow_inv_hist / k_bow_scan / k_bow_inv_scatter
// transpose the database CSR into one inverted index per database chunk (key chunk * n_words + word), k_bow_score_chunk
// (workgroup = (query, chunk)) adds min(vq, vd) into int32 accumulators in LDS with LDS atomics and selects the chunk's top k,
// k_bow_score_merge merges the chunks under the same key (score descending, index ascending).
#pragma once
#include <hip/hip_runtime.h>

namespace ba {

constexpr int BW_THREADS = 256;
constexpr int BW_MAX_K = 32;             // branching
constexpr int BW_MAX_LEVELS = 8;
constexpr int BW_ROW_BITS = 24;          // training rows < 2^24: the seed key's low bits
constexpr unsigned long long BW_ROW_MASK = (1ull << BW_ROW_BITS) - 1;
constexpr int BW_MAX_SET = 1 << 16;      // rows of one set in ba_bow_transform (ORB_MAX_FEATURES)
constexpr int BW_MAX_IDF = (1 << 17) - 1;   // c * idf < 2^33, so (a << 30) fits in 63 bits
constexpr int BW_CHUNK = 4096;           // database vectors per score workgroup (int32 accumulators in LDS)
constexpr int BW_MAX_TOPK = 64;
constexpr int BW_SCAN_THREADS = 1024, BW_SCAN_ITEMS = 4;
constexpr unsigned long long BW_GOLDEN = 0x9E3779B97F4A7C15ull;

__device__ __host__ __forceinline__ unsigned long long bw_mix(unsigned long long z) {   // the splitmix64 finaliser (ba_ransac.hpp)
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

struct VocabArgs {
  const unsigned long long* desc;   // [rows][W]
  int* perm;                        // [rows] position -> row, ordered by node
  int* node;                        // [rows] by row
  int* slot;                        // [rows] by row: slot of the last assignment of this level, -1 before the first
  int rows, k, words;               // words = W
  int lvl_begin, lvl_n;             // the nodes of this depth are lvl_begin .. lvl_begin + lvl_n - 1
  const unsigned char* open;        // [lvl_n] the node is being split
  unsigned long long* seed_key;     // [lvl_n * k]
  unsigned long long* centre;       // [lvl_n * k][W]
  unsigned char* usable;            // [lvl_n * k]
  int* size;                        // [lvl_n * k]
  int* votes;                       // [lvl_n * k][64 W]
  int* changed;                     // [1]
  const int* child;                 // [lvl_n * k] the node a slot became, -1 where the node stays a leaf
  int* cursor;                      // [nodes] first position of every node in the next perm
  unsigned long long pre[BW_MAX_K]; // mix(mix(mix(seed + G) + depth) + slot)
};

// the node of position p, relative to the level, or -1 when it is not being split
__device__ __forceinline__ int bw_open_node(const VocabArgs& a, int p, int& row) {
  if (p >= a.rows) return -1;
  row = a.perm[p];
  const int n = a.node[row] - a.lvl_begin;
  return (n >= 0 && n < a.lvl_n && a.open[n]) ? n : -1;
}
// true when every lane of the workgroup holds node n0 (the first lane's); uniform over the workgroup
__device__ __forceinline__ bool bw_uniform_node(int n, int* sh) {
  if (threadIdx.x == 0) *sh = n;
  __syncthreads();
  const int n0 = *sh;
  return __syncthreads_and(n == n0 && n >= 0) != 0;
}

__global__ __launch_bounds__(BW_THREADS) void k_vocab_seed_key(VocabArgs a) {
  __shared__ int sh_n;
  int row = 0;
  const int n = bw_open_node(a, blockIdx.x * BW_THREADS + threadIdx.x, row);
  const bool uni = bw_uniform_node(n, &sh_n);
  if (n < 0) return;        // (no barrier below)
  for (int j = 0; j < a.k; ++j) {
    unsigned long long key = (bw_mix(a.pre[j] + ((unsigned long long)row + 1) * BW_GOLDEN) & ~BW_ROW_MASK) | (unsigned long long)row;
    if (uni) {              // all 64 lanes of every wave are live and in one node
      for (int m = 32; m >= 1; m >>= 1) {
        const unsigned long long o = __shfl_xor(key, m);
        key = o < key ? o : key;
      }
      if ((threadIdx.x & 63) == 0) atomicMin(a.seed_key + (size_t)n * a.k + j, key);
    } else {
      atomicMin(a.seed_key + (size_t)n * a.k + j, key);
    }
  }
}

__global__ __launch_bounds__(BW_THREADS) void k_vocab_seed_set(VocabArgs a) {
  const int e = blockIdx.x * BW_THREADS + threadIdx.x;
  if (e >= a.lvl_n * a.k) return;
  const int n = e / a.k, j = e - n * a.k;
  if (!a.open[n]) return;
  if (a.seed_key[e] == ~0ull) { a.usable[e] = 0; return; }      // (no member offered a key: an open node has members, so never)
  const int row = (int)(a.seed_key[e] & BW_ROW_MASK);
  bool fresh = true;
  for (int i = 0; i < j; ++i) fresh = fresh && (int)(a.seed_key[(size_t)n * a.k + i] & BW_ROW_MASK) != row;
  a.usable[e] = fresh ? 1 : 0;
  for (int w = 0; w < a.words; ++w) a.centre[(size_t)e * a.words + w] = a.desc[(size_t)row * a.words + w];
}

template <int W>
__global__ __launch_bounds__(BW_THREADS) void k_vocab_assign(VocabArgs a) {
  __shared__ int sh_n;
  __shared__ int hist[BW_MAX_K];
  int row = 0;
  const int n = bw_open_node(a, blockIdx.x * BW_THREADS + threadIdx.x, row);
  if (threadIdx.x < BW_MAX_K) hist[threadIdx.x] = 0;
  const bool uni = bw_uniform_node(n, &sh_n);      // (its barriers order the zeroing of hist too)
  bool moved = false;
  if (n >= 0) {
    unsigned long long q[W];
#pragma unroll
    for (int w = 0; w < W; ++w) q[w] = a.desc[(size_t)row * W + w];
    unsigned best = 0xffffffffu;
    for (int j = 0; j < a.k; ++j) {
      const size_t e = (size_t)n * a.k + j;
      if (!a.usable[e]) continue;
      unsigned d = 0;
#pragma unroll
      for (int w = 0; w < W; ++w) d += (unsigned)__popcll(q[w] ^ a.centre[e * W + w]);
      best = min(best, (d << 5) | (unsigned)j);
    }
    const int s = best == 0xffffffffu ? 0 : (int)(best & 31u);      // (slot 0 is always usable)
    moved = a.slot[row] != s;
    a.slot[row] = s;
    if (uni) atomicAdd(&hist[s], 1);
    else atomicAdd(a.size + (size_t)n * a.k + s, 1);
  }
  const int c = __syncthreads_count(moved);
  if (threadIdx.x == 0 && c > 0) atomicAdd(a.changed, c);
  if (uni && threadIdx.x < a.k && hist[threadIdx.x] > 0) atomicAdd(a.size + (size_t)sh_n * a.k + threadIdx.x, hist[threadIdx.x]);
}

template <int W>
__global__ __launch_bounds__(BW_THREADS) void k_vocab_vote(VocabArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned long long tile[BW_THREADS * W];
  __shared__ int t_node[BW_THREADS];
  __shared__ int t_slot[BW_THREADS];
  __shared__ int cnt[BW_MAX_K * BW_THREADS];
  const int tid = threadIdx.x;
  {
    int row = 0;
    const int n = bw_open_node(a, blockIdx.x * BW_THREADS + tid, row);
    t_node[tid] = n;
    t_slot[tid] = n >= 0 ? a.slot[row] : 0;
#pragma unroll
    for (int w = 0; w < W; ++w) tile[tid * W + w] = n >= 0 ? a.desc[(size_t)row * W + w] : 0ull;
  }
  for (int j = 0; j < a.k; ++j) cnt[j * BW_THREADS + tid] = 0;
  __syncthreads();
  constexpr int BITS = 64 * W;
  for (int bit = tid; bit < BITS; bit += BW_THREADS) {
    const int word = bit >> 6, sh = bit & 63;
    int cur = -1;
    for (int t = 0; t <= BW_THREADS; ++t) {
      const int n = t < BW_THREADS ? t_node[t] : -2;        // (uniform over the workgroup; -2 flushes the last node)
      if (n == -1) continue;
      if (n != cur) {
        if (cur >= 0)
          for (int j = 0; j < a.k; ++j) {
            const int c = cnt[j * BW_THREADS + tid];
            if (c) { atomicAdd(a.votes + ((size_t)cur * a.k + j) * BITS + bit, c); cnt[j * BW_THREADS + tid] = 0; }
          }
        cur = n;
      }
      if (n >= 0) cnt[t_slot[t] * BW_THREADS + tid] += (int)((tile[t * W + word] >> sh) & 1ull);
    }
  }
}

__global__ __launch_bounds__(BW_THREADS) void k_vocab_centre(VocabArgs a) {
  const long long e = (long long)blockIdx.x * BW_THREADS + threadIdx.x;
  if (e >= (long long)a.lvl_n * a.k * a.words) return;
  const int w = (int)(e % a.words);
  const long long s = e / a.words;          // (node, slot)
  if (!a.open[s / a.k]) return;
  const int size = a.size[s];
  if (size == 0) return;                    // an empty slot keeps its centre
  const int* v = a.votes + (s * a.words + w) * 64;
  unsigned long long c = 0;
  for (int b = 0; b < 64; ++b) c |= (unsigned long long)(2 * v[b] >= size) << b;
  a.centre[e] = c;
}

__global__ __launch_bounds__(BW_THREADS) void k_vocab_children(VocabArgs a) {
  int row = 0;
  const int n = bw_open_node(a, blockIdx.x * BW_THREADS + threadIdx.x, row);
  if (n < 0) return;
  const int c = a.child[(size_t)n * a.k + a.slot[row]];
  if (c >= 0) a.node[row] = c;
  a.slot[row] = -1;
}

__global__ __launch_bounds__(BW_THREADS) void k_vocab_scatter(VocabArgs a) {
  const int row = blockIdx.x * BW_THREADS + threadIdx.x;
  if (row >= a.rows) return;
  a.perm[atomicAdd(a.cursor + a.node[row], 1)] = row;
}

// ------------------------------------------------------------------------------------------------------------ transform
struct BowArgs {
  const unsigned long long* desc;   // [rows][W]
  const long long* set_off;         // [n_sets + 1]
  const int* child0;                // the vocabulary
  const int* n_child;
  const unsigned long long* node_desc;
  const int* word_of_node;
  const int* idf_q;
  int rows, n_sets, n_words, tf;
  int s0, s1;                       // the sets of this batch
  int* word;                        // [rows]
  int* cnt;                         // [s1 - s0][n_words], zeroed
  int* out_word;                    // [rows]: set s writes from set_off[s]
  int* out_val;
  int* nnz;                         // [n_sets]
};

template <int W>
__global__ __launch_bounds__(BW_THREADS) void k_bow_descend(BowArgs a) {
  const int r = blockIdx.x * BW_THREADS + threadIdx.x;
  if (r >= a.rows) return;
  unsigned long long q[W];
#pragma unroll
  for (int w = 0; w < W; ++w) q[w] = a.desc[(size_t)r * W + w];
  int n = 0;
  for (int c0 = a.child0[0]; c0 >= 0; c0 = a.child0[n]) {       // (children follow their parent: the walk ends)
    const int nc = a.n_child[n];
    unsigned best = 0xffffffffu;
    for (int j = 0; j < nc; ++j) {
      unsigned d = 0;
#pragma unroll
      for (int w = 0; w < W; ++w) d += (unsigned)__popcll(q[w] ^ a.node_desc[(size_t)(c0 + j) * W + w]);
      best = min(best, (d << 5) | (unsigned)j);
    }
    n = c0 + (int)(best & 31u);
  }
  a.word[r] = a.word_of_node[n];
}

// the set of row r: the last s with set_off[s] <= r
__device__ __forceinline__ int bw_owner(const long long* off, int n, long long r) {
  int lo = 0, hi = n;               // off[lo] <= r < off[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (off[mid] <= r) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(BW_THREADS) void k_bow_count(BowArgs a) {
  const long long r = a.set_off[a.s0] + (long long)blockIdx.x * BW_THREADS + threadIdx.x;
  if (r >= a.set_off[a.s1]) return;
  const int s = bw_owner(a.set_off, a.n_sets, r);
  atomicAdd(a.cnt + (size_t)(s - a.s0) * a.n_words + a.word[r], 1);
}

__global__ __launch_bounds__(BW_THREADS) void k_bow_vector(BowArgs a) {
  __shared__ long long red[BW_THREADS];
  __shared__ int wave_n[BW_THREADS / 64];
  const int s = a.s0 + blockIdx.x, tid = threadIdx.x;
  const int* cnt = a.cnt + (size_t)blockIdx.x * a.n_words;
  long long sum = 0;
  for (int i = tid; i < a.n_words; i += BW_THREADS) sum += (long long)cnt[i] * (a.tf ? 4096 : a.idf_q[i]);
  red[tid] = sum;
  __syncthreads();
  for (int m = BW_THREADS / 2; m >= 1; m >>= 1) {
    if (tid < m) red[tid] += red[tid + m];
    __syncthreads();
  }
  const long long A = red[0];
  const long long base = a.set_off[s];
  int written = 0;                  // (the same in every lane)
  if (A > 0)
    for (int i0 = 0; i0 < a.n_words; i0 += BW_THREADS) {
      const int i = i0 + tid;
      int v = 0;
      if (i < a.n_words) {
        const long long ai = (long long)cnt[i] * (a.tf ? 4096 : a.idf_q[i]);
        v = (int)((ai << 30) / A);
      }
      const unsigned long long m = __ballot(v > 0);
      __syncthreads();              // (wave_n of the previous round has been read)
      if ((tid & 63) == 0) wave_n[tid >> 6] = __popcll(m);
      __syncthreads();
      int before = __popcll(m & ((1ull << (tid & 63)) - 1)), total = 0;
      for (int w = 0; w < BW_THREADS / 64; ++w) {
        if (w < (tid >> 6)) before += wave_n[w];
        total += wave_n[w];
      }
      if (v > 0) { a.out_word[base + written + before] = i; a.out_val[base + written + before] = v; }
      written += total;
    }
  if (tid == 0) a.nnz[s] = written;
}

// ---------------------------------------------------------------------------------------------------------------- score
struct ScoreArgs {
  const long long* q_off;           // query CSR
  const int* q_word;
  const int* q_val;
  const long long* d_off;           // database CSR
  const int* d_word;
  const int* d_val;
  const int* db_end;                // [nq] or null
  int nq, nd, n_words, chunk, n_chunks, top_k;
  long long d_nnz, n_keys;          // n_keys = n_chunks * n_words
  int* hist;                        // [n_keys + 1] counts, then (k_bow_scan) exclusive offsets
  int* cursor;                      // [n_keys]
  int* inv_j;                       // [d_nnz] database index within its chunk
  int* inv_v;
  unsigned long long* part;         // [nq][n_chunks][top_k] keys score << 32 | ~index, 0 = none
  int* top_idx;                     // [nq][top_k]
  int* top_score;
  int* dense;                       // [nq][nd] or null
};

__global__ __launch_bounds__(BW_THREADS) void k_bow_inv_hist(ScoreArgs a) {
  const long long e = (long long)blockIdx.x * BW_THREADS + threadIdx.x;
  if (e >= a.d_nnz) return;
  const int j = bw_owner(a.d_off, a.nd, e);
  atomicAdd(a.hist + (long long)(j / a.chunk) * a.n_words + a.d_word[e], 1);
}

// exclusive prefix sum of hist[0 .. n_keys) in place, the total in hist[n_keys]; one workgroup
__global__ __launch_bounds__(BW_SCAN_THREADS) void k_bow_scan(ScoreArgs a) {
  __shared__ int sh[BW_SCAN_THREADS];
  __shared__ int carry;
  const int tid = threadIdx.x;
  if (tid == 0) carry = 0;
  __syncthreads();
  for (long long i0 = 0; i0 < a.n_keys; i0 += BW_SCAN_THREADS * BW_SCAN_ITEMS) {
    const long long i = i0 + (long long)tid * BW_SCAN_ITEMS;
    int v[BW_SCAN_ITEMS], mine = 0;
#pragma unroll
    for (int t = 0; t < BW_SCAN_ITEMS; ++t) { v[t] = i + t < a.n_keys ? a.hist[i + t] : 0; mine += v[t]; }
    sh[tid] = mine;
    __syncthreads();
    for (int m = 1; m < BW_SCAN_THREADS; m <<= 1) {       // inclusive scan of the lanes' sums
      const int add = tid >= m ? sh[tid - m] : 0;
      __syncthreads();
      sh[tid] += add;
      __syncthreads();
    }
    int run = carry + sh[tid] - mine;
#pragma unroll
    for (int t = 0; t < BW_SCAN_ITEMS; ++t) {
      if (i + t < a.n_keys) a.hist[i + t] = run;
      run += v[t];
    }
    __syncthreads();
    if (tid == BW_SCAN_THREADS - 1) carry += sh[tid];
    __syncthreads();
  }
  if (tid == 0) a.hist[a.n_keys] = carry;
}

__global__ __launch_bounds__(BW_THREADS) void k_bow_inv_scatter(ScoreArgs a) {
  const long long e = (long long)blockIdx.x * BW_THREADS + threadIdx.x;
  if (e >= a.d_nnz) return;
  const int j = bw_owner(a.d_off, a.nd, e);
  const int c = j / a.chunk;
  const int pos = atomicAdd(a.cursor + (long long)c * a.n_words + a.d_word[e], 1);
  a.inv_j[pos] = j - c * a.chunk;
  a.inv_v[pos] = a.d_val[e];
}

__device__ __forceinline__ unsigned long long bw_key_max(unsigned long long k) {
  for (int m = 32; m >= 1; m >>= 1) {
    const unsigned long long o = __shfl_xor(k, m);
    k = o > k ? o : k;
  }
  return k;
}

__global__ __launch_bounds__(BW_THREADS) void k_bow_score_chunk(ScoreArgs a) {
  __shared__ int acc[BW_CHUNK];
  __shared__ unsigned long long wave_k[BW_THREADS / 64];
  const int q = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
  const int j0 = c * a.chunk;
  const int end = a.db_end ? min(a.nd, max(0, a.db_end[q])) : a.nd;      // entries j < end are admitted
  const int live = max(0, min(a.chunk, end - j0)), len = min(a.chunk, a.nd - j0);
  unsigned long long* part = a.part + ((size_t)q * a.n_chunks + c) * a.top_k;
  for (int t = tid; t < a.chunk; t += BW_THREADS) acc[t] = 0;
  __syncthreads();
  if (live > 0) {
    const long long qa = a.q_off[q], qb = a.q_off[q + 1];
    const int* lo = a.hist + (long long)c * a.n_words;
    // a wave per query word, its lanes over the word's list
    for (long long e = qa + (tid >> 6); e < qb; e += BW_THREADS / 64) {
      const int w = a.q_word[e];
      if (w >= a.n_words) continue;
      const int vq = a.q_val[e];
      for (int p = lo[w] + (tid & 63); p < lo[w + 1]; p += 64) {
        const int j = a.inv_j[p];
        if (j < live) atomicAdd(&acc[j], min(vq, a.inv_v[p]));
      }
    }
  }
  __syncthreads();
  if (a.dense)
    for (int t = tid; t < len; t += BW_THREADS) a.dense[(size_t)q * a.nd + j0 + t] = acc[t];
  // the chunk's top k: round r takes the largest key below the one of round r - 1 (keys are distinct: they carry the index)
  unsigned long long prev = ~0ull;
  for (int r = 0; r < a.top_k; ++r) {
    unsigned long long best = 0;
    if (prev != 0)
      for (int t = tid; t < live; t += BW_THREADS) {
        const int s = acc[t];
        const unsigned long long key = s > 0 ? ((unsigned long long)(unsigned)s << 32) | (unsigned)~(unsigned)(j0 + t) : 0ull;
        if (key < prev && key > best) best = key;
      }
    best = bw_key_max(best);
    __syncthreads();                // (wave_k of the previous round has been read)
    if ((tid & 63) == 0) wave_k[tid >> 6] = best;
    __syncthreads();
    best = 0;
    for (int w = 0; w < BW_THREADS / 64; ++w) best = wave_k[w] > best ? wave_k[w] : best;
    if (tid == 0) part[r] = best;
    prev = best;
  }
}

__global__ __launch_bounds__(BW_THREADS) void k_bow_score_merge(ScoreArgs a) {
  const int q = blockIdx.x * BW_THREADS + threadIdx.x;
  if (q >= a.nq) return;
  const unsigned long long* part = a.part + (size_t)q * a.n_chunks * a.top_k;
  const int n = a.n_chunks * a.top_k;
  unsigned long long prev = ~0ull;
  for (int r = 0; r < a.top_k; ++r) {
    unsigned long long best = 0;
    if (prev != 0)
      for (int i = 0; i < n; ++i) {
        const unsigned long long key = part[i];
        if (key < prev && key > best) best = key;
      }
    a.top_idx[(size_t)q * a.top_k + r] = best ? (int)~(unsigned)(best & 0xffffffffull) : -1;
    a.top_score[(size_t)q * a.top_k + r] = (int)(best >> 32);
    prev = best;
  }
}

}  // namespace ba
