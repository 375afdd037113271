// ba_build_tracks on the device: feature tracks from pairwise matches -- the step between the verified matches of the
// image pairs (ba_match_descriptors / ba_match_guided, ba_fundamental / ba_relative_pose / ba_homography) and the
// (cam_idx, pt_idx, uv) lists ba_triangulate_tracks and ba_set_problem start from.  OpenMVG's TracksBuilder, COLMAP's
// correspondence graph; the reference does it pair by pair with a Python dict per keyframe (src/pipeline.py,
// _add_new_keyframe / _add_new_keyframe_exhaustive: last_kf_obs_lookup / kf_obs_lookup).
//
// A node is a keypoint (node = kp_off[image] + keypoint), an edge one match.  Everything is integer, and every output
// is a function of the SET of kept edges:
//   components   a parent array with parent[v] <= v at all times.  k_tb_hook (lane = edge) walks both ends to their
//                roots and links the larger root under the smaller by compare-and-swap on a node that is still its own
//                parent, so a link once made is never lost and a root is always the smallest node of its tree.  A lane
//                whose compare-and-swap loses goes on from the parent it found there and walks again: it leaves only when
//                its two ends have one root or when its own link went in.  k_tb_compress (lane = node) points every node at
//                its root.  The host alternates the two until a hook round finds every edge with equal roots.  Every
//                value ever stored in parent[x] is smaller than x, so a walk strictly decreases, and a lane's two roots
//                only ever decrease from one attempt to the next: every device loop ends, whatever other lanes do.  No
//                kernel waits on another workgroup: a lane never polls a word for a value, every failed attempt moves
//                it on.  What one round must see of the previous one it sees by the kernel boundary; what a lane sees or
//                misses of ITS OWN round's links changes which links are made, never the components.  Rounds: a lane
//                leaves the first hook round only with its edge's ends in one tree, and trees never split, so the second
//                round finds nothing to link -- two rounds, in whatever order the atomics are served.
//   ordering     ba_set_problem's method (ba_setup.hpp): component sizes by integer atomicAdd, exclusive scan over the
//                roots in node order (k_scan_*, in chunks with a carried base), scatter in whatever order the cursors
//                hand out, every segment sorted ascending (unique keys: the sorted segment is the answer).  Three classes of
//                segment: at most 64 nodes, a wave (one key per lane); at most 12288, a workgroup's rank sort in LDS; longer
//                ("giant"), no scatter and no sort: flags of the component over all nodes, a scan, every member to its rank.
//   conflicts    in a sorted segment the nodes of one image are neighbours (an image's nodes are contiguous): a
//                conflict is a position whose predecessor in the segment lies in the same image.
//   compaction   flags per position, exclusive scan, ordered scatter into track_node / track_off / node_track.
#pragma once
#include "ba_setup.hpp"

namespace ba {

constexpr int TB_THREADS = 256;
constexpr int TB_WAVE_MAX = 64;                 // longest segment one wave sorts (one key per lane)
constexpr int TB_LDS_MAX = SETUP_RANK_LDS;      // longest segment a workgroup stages in LDS for its rank sort
constexpr int TB_SORT_GRID = 1024;              // workgroups of k_tb_sort_lds (they stride over its list)
enum { TB_IN_TRACK = 0, TB_ISOLATED = 1, TB_CONFLICT = 2, TB_SHORT = 3 };   // node_status (enum ba_trackbuild_status)
enum { TB_DROP = 0, TB_FIRST = 1 };                                          // ba_trackbuild_options.conflict

__device__ __forceinline__ int tb_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void tb_store(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// base[key] += 1 for every lane with key >= 0, one atomic per DISTINCT key of the wave (the nodes of a giant component would otherwise
// queue millions of atomics on one word).  Every lane of the wave calls it.
__device__ __forceinline__ void tb_count_by_key(int* base, int key) {
  const int lane = threadIdx.x & 63;
  unsigned long long todo = __ballot(key >= 0);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const int k = __shfl(key, leader, 64);
    const unsigned long long same = __ballot(key == k);
    if (lane == leader) atomicAdd(base + k, (int)__popcll(same));
    todo &= ~same;
  }
}

// parent[v] = v; img[v] = the image of node v (the i with kp_off[i] <= v < kp_off[i + 1]); node_track = -1, status = isolated
__global__ void __launch_bounds__(TB_THREADS)
k_tb_init(int n, const long long* __restrict__ kp_off, int n_images, int* __restrict__ parent, int* __restrict__ img,
          int* __restrict__ node_track, unsigned char* __restrict__ status) {
  const long long i = (long long)blockIdx.x * TB_THREADS + threadIdx.x;
  if (i >= n) return;
  int lo = 0, hi = n_images;                    // kp_off[lo] <= i < kp_off[hi]
  while (hi - lo > 1) {
    const int mid = lo + (hi - lo) / 2;
    if (kp_off[mid] <= i) lo = mid; else hi = mid;
  }
  parent[i] = (int)i; img[i] = lo; node_track[i] = -1; status[i] = TB_ISOLATED;
}

// use[e] = the edge takes part: kept, both ends in [0, n), ends in different images.  bad[0] = smallest kept edge with an end
// out of range (~0: none); same[0] += kept edges inside one image.
__global__ void __launch_bounds__(TB_THREADS)
k_tb_edges(const int* __restrict__ ea, const int* __restrict__ eb, const unsigned char* __restrict__ keep, long long n_edges, int n,
           const int* __restrict__ img, unsigned char* __restrict__ use, unsigned long long* __restrict__ bad,
           unsigned long long* __restrict__ same) {
  const long long e = (long long)blockIdx.x * TB_THREADS + threadIdx.x;
  if (e >= n_edges) return;
  unsigned char u = 0;
  if (!keep || keep[e]) {
    const int a = ea[e], b = eb[e];
    if (a < 0 || a >= n || b < 0 || b >= n) atomicMin(bad, (unsigned long long)e);
    else if (img[a] == img[b]) atomicAdd(same, 1ULL);
    else u = 1;
  }
  use[e] = u;
}

// One lane per edge: both roots, the larger linked under the smaller while it is still a root; a lane whose link loses to another
// lane's goes on from where that one pointed the root and tries again, until its two ends have one root or its own link is in.  Both
// ra and rb only decrease, so the loop ends; nothing here waits for another lane.  flag[0] = 1 when the roots of any edge differed.
__global__ void __launch_bounds__(TB_THREADS)
k_tb_hook(const int* __restrict__ ea, const int* __restrict__ eb, const unsigned char* __restrict__ use, long long n_edges,
          int* __restrict__ parent, int* __restrict__ flag) {
  const long long e = (long long)blockIdx.x * TB_THREADS + threadIdx.x;
  if (e >= n_edges || !use[e]) return;
  int ra = ea[e], rb = eb[e];
  bool told = false;
  for (;;) {
    for (;;) { const int p = tb_load(parent + ra); if (p >= ra) break; ra = p; }     // p < ra while ra is no root: the walk decreases
    for (;;) { const int p = tb_load(parent + rb); if (p >= rb) break; rb = p; }
    if (ra == rb) return;
    if (!told) { tb_store(flag, 1); told = true; }
    const int hi = max(ra, rb), lo = min(ra, rb);
    const int was = atomicCAS(parent + hi, hi, lo);
    if (was == hi) return;                      // linked
    if (hi == ra) ra = was; else rb = was;      // another lane linked hi under was < hi in the meantime: on from there
  }
}

// One lane per node: parent[v] = the root of v.  No link is made during this kernel, so roots stay roots; other lanes' stores only
// replace an ancestor by a higher ancestor, and a lane that sees one merely gets there sooner.
__global__ void __launch_bounds__(TB_THREADS)
k_tb_compress(int n, int* __restrict__ parent) {
  const long long i = (long long)blockIdx.x * TB_THREADS + threadIdx.x;
  if (i >= n) return;
  int p = tb_load(parent + i);
  if (p == (int)i) return;
  for (;;) { const int g = tb_load(parent + p); if (g >= p) break; p = g; }
  tb_store(parent + i, p);
}

// cnt[label[v]] += 1
__global__ void __launch_bounds__(TB_THREADS)
k_tb_sizes(int n, const int* __restrict__ label, int* __restrict__ cnt) {
  const long long i = (long long)blockIdx.x * TB_THREADS + threadIdx.x;
  tb_count_by_key(cnt, i < n ? label[i] : -1);
}
// per node: seg_len = size of the component if v is the root of one with at least two nodes, else 0; is_comp = that as a flag
__global__ void __launch_bounds__(TB_THREADS)
k_tb_roots(int n, const int* __restrict__ label, const int* __restrict__ cnt, int* __restrict__ seg_len, int* __restrict__ is_comp) {
  const long long i = (long long)blockIdx.x * TB_THREADS + threadIdx.x;
  if (i >= n) return;
  const bool root = label[i] == (int)i && cnt[i] >= 2;
  seg_len[i] = root ? cnt[i] : 0; is_comp[i] = root ? 1 : 0;
}
// bsum[0 .. nb] += base[0]: carries the running total into the next chunk of a scan longer than one k_scan_* pass
__global__ void __launch_bounds__(1024)
k_tb_scan_base(int* __restrict__ bsum, int nb, const int* __restrict__ base) {
  const int add = base[0];
  for (int i = threadIdx.x; i <= nb; i += 1024) bsum[i] += add;
}
// the list of components in root order: comp_root[c], comp_off[c] = first position of its segment; comp_off[C] = M
__global__ void __launch_bounds__(TB_THREADS)
k_tb_comp_list(int n, const int* __restrict__ is_comp, const int* __restrict__ comp_id, const int* __restrict__ seg_off,
               int* __restrict__ comp_root, int* __restrict__ comp_off) {
  const long long i = (long long)blockIdx.x * TB_THREADS + threadIdx.x;
  if (i >= n) return;
  if (is_comp[i]) { const int c = comp_id[i]; comp_root[c] = (int)i; comp_off[c] = seg_off[i]; }
  if (i == n - 1) comp_off[comp_id[n]] = seg_off[n];
}
// members of components of 2 .. lds_max nodes into their segment, in whatever order the cursors hand out (a giant component's
// members are placed in order by k_tb_giant_*)
__global__ void __launch_bounds__(TB_THREADS)
k_tb_scatter(int n, const int* __restrict__ label, const int* __restrict__ cnt, const int* __restrict__ seg_off, int lds_max, int* __restrict__ fill,
             int* __restrict__ seg) {
  const long long i = (long long)blockIdx.x * TB_THREADS + threadIdx.x;
  if (i >= n) return;
  const int r = label[i], m = cnt[r];
  if (m >= 2 && m <= lds_max) seg[seg_off[r] + atomicAdd(fill + r, 1)] = (int)i;
}

// ---- segment sorts (rank sorts: keys are unique) ------------------------------------------------------------------
// One wave per component: segments of at most wave_max (<= 64) keys, one key per lane.  Longer ones go to `big` (at most lds_max
// keys) or `giant`, in any order.  lists = {n_big, n_giant}.
__global__ void __launch_bounds__(TB_THREADS)
k_tb_sort_wave(int n_comp, const int* __restrict__ comp_off, const int* __restrict__ seg, int* __restrict__ sorted, int wave_max, int lds_max,
               int* __restrict__ big, int* __restrict__ giant, int* __restrict__ lists) {
  const long long cw = (long long)blockIdx.x * (TB_THREADS / 64) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (cw >= n_comp) return;                     // uniform over the wave
  const int c = (int)cw, b = comp_off[c], n = comp_off[c + 1] - b;
  if (n > wave_max) {
    if (lane == 0) { if (n <= lds_max) big[atomicAdd(lists, 1)] = c; else giant[atomicAdd(lists + 1, 1)] = c; }
    return;
  }
  const int key = lane < n ? seg[b + lane] : 0x7fffffff;
  int r = 0;
  for (int q = 0; q < n; ++q) r += __shfl(key, q, 64) < key;
  if (lane < n) sorted[b + r] = key;
}
// One workgroup per entry of `big`: the segment staged in LDS (n <= lds_max <= TB_LDS_MAX)
__global__ void __launch_bounds__(TB_THREADS)
k_tb_sort_lds(const int* __restrict__ big, const int* __restrict__ lists, const int* __restrict__ comp_off, const int* __restrict__ seg,
              int* __restrict__ sorted) {
  __shared__ int keys[TB_LDS_MAX];
  const int n_big = lists[0];
  for (int w = blockIdx.x; w < n_big; w += gridDim.x) {
    const int c = big[w], b = comp_off[c], n = min(comp_off[c + 1] - b, TB_LDS_MAX);
    for (int a = threadIdx.x; a < n; a += TB_THREADS) keys[a] = seg[b + a];
    __syncthreads();
    for (int a = threadIdx.x; a < n; a += TB_THREADS) {
      const int e = keys[a];
      int r = 0;
      for (int q = 0; q < n; ++q) r += keys[q] < e;
      sorted[b + r] = e;
    }
    __syncthreads();
  }
}
// Giant segments (more than lds_max nodes; chained false matches do make them), from global memory and without a sort: the rank of
// node v in its segment is the number of smaller nodes with its label.  Per giant component: flags over all N nodes, the exclusive
// scan (k_scan_*), and every member goes to its place.  O(N) per giant component, of which there are at most N / lds_max.
__global__ void __launch_bounds__(TB_THREADS)
k_tb_giant_flags(int n, const int* __restrict__ label, const int* __restrict__ giant, const int* __restrict__ comp_root, int* __restrict__ flag) {
  const long long i = (long long)blockIdx.x * TB_THREADS + threadIdx.x;
  if (i < n) flag[i] = label[i] == comp_root[giant[0]] ? 1 : 0;
}
__global__ void __launch_bounds__(TB_THREADS)
k_tb_giant_place(int n, const int* __restrict__ flag, const int* __restrict__ rank, const int* __restrict__ giant, const int* __restrict__ comp_off,
                 int* __restrict__ sorted) {
  const long long i = (long long)blockIdx.x * TB_THREADS + threadIdx.x;
  if (i < n && flag[i]) sorted[comp_off[giant[0]] + rank[i]] = (int)i;
}

// ---- conflicts, tracks, compaction ------------------------------------------------------------------------------------
// lane = position j of the sorted list: conf[j] = its predecessor in the segment lies in the same image; n_conf[c] += conf[j]
__global__ void __launch_bounds__(TB_THREADS)
k_tb_conflict(int m, const int* __restrict__ sorted, const int* __restrict__ label, const int* __restrict__ comp_id, const int* __restrict__ comp_off,
              const int* __restrict__ img, unsigned char* __restrict__ conf, int* __restrict__ n_conf) {
  const long long j = (long long)blockIdx.x * TB_THREADS + threadIdx.x;
  int key = -1;
  if (j < m) {
    const int v = sorted[j], c = comp_id[label[v]];
    const bool x = j > comp_off[c] && img[sorted[j - 1]] == img[v];
    conf[j] = x ? 1 : 0;
    if (x) key = c;
  }
  tb_count_by_key(n_conf, key);
}
// lane = component: is it a track?  stat[3] += components with a conflict, stat[4] += nodes dropped for a conflict,
// stat[5] += components dropped as short
__global__ void __launch_bounds__(TB_THREADS)
k_tb_comp_verdict(int n_comp, const int* __restrict__ comp_off, const int* __restrict__ n_conf, int policy, int min_length,
                  int* __restrict__ is_track, unsigned long long* __restrict__ stat) {
  const long long c = (long long)blockIdx.x * TB_THREADS + threadIdx.x;
  if (c >= n_comp) return;
  const int n = comp_off[c + 1] - comp_off[c], nc = n_conf[c];
  const bool dropped = policy == TB_DROP && nc > 0;
  const int kept = dropped ? 0 : n - nc;
  const bool track = !dropped && kept >= min_length;
  is_track[c] = track ? 1 : 0;
  if (nc > 0) { atomicAdd(stat + 3, 1ULL); atomicAdd(stat + 4, (unsigned long long)(dropped ? n : nc)); }
  if (!dropped && !track) atomicAdd(stat + 5, 1ULL);
}
// lane = position: out[j] = the node is a member of a track
__global__ void __launch_bounds__(TB_THREADS)
k_tb_out_flags(int m, const int* __restrict__ sorted, const int* __restrict__ label, const int* __restrict__ comp_id, const int* __restrict__ is_track,
               const unsigned char* __restrict__ conf, int* __restrict__ out) {
  const long long j = (long long)blockIdx.x * TB_THREADS + threadIdx.x;
  if (j >= m) return;
  out[j] = (is_track[comp_id[label[sorted[j]]]] && !conf[j]) ? 1 : 0;
}
// lane = position: the ordered compaction.  pos = exclusive scan of out (pos[m] = members), trk_id = exclusive scan of is_track.
__global__ void __launch_bounds__(TB_THREADS)
k_tb_emit(int m, const int* __restrict__ sorted, const int* __restrict__ label, const int* __restrict__ comp_id, const int* __restrict__ comp_off,
          const int* __restrict__ is_track, const int* __restrict__ trk_id, const int* __restrict__ n_conf, const unsigned char* __restrict__ conf,
          const int* __restrict__ pos, int policy, int* __restrict__ track_node, int* __restrict__ track_off, int* __restrict__ node_track,
          unsigned char* __restrict__ status) {
  const long long j = (long long)blockIdx.x * TB_THREADS + threadIdx.x;
  if (j >= m) return;
  const int v = sorted[j], c = comp_id[label[v]];
  if (is_track[c] && !conf[j]) {
    const int t = trk_id[c], o = pos[j];
    track_node[o] = v; node_track[v] = t; status[v] = TB_IN_TRACK;
    if (j == comp_off[c]) track_off[t] = o;     // the label: first of its segment, never a conflict
  } else {
    const bool x = policy == TB_DROP ? n_conf[c] > 0 : conf[j] != 0;
    status[v] = x ? TB_CONFLICT : TB_SHORT;     // node_track stays -1 (k_tb_init)
  }
}

}  // namespace ba
