// libba_hip.so: host side of the MI355X bundle-adjustment solve step and its C ABI
// (include/ba_hip.h).  One handle owns one GPU, one stream, every device buffer of one
// problem, and (multi-rank jobs) one RCCL communicator loaded with dlopen.
//
// LM / Schur / PCG loop (ba_solve), replacing scipy.optimize.least_squares at
// src/bundle_adjuster.py:170-174 of the reference:
//   linearise (K2a camera pass, K2b point pass)            [all-reduce Hcc | bc]
//   repeat with damping lambda until a step is accepted:
//     K3 damp + invert point blocks, y0 = Hpp^-1 bp;  rhs pass (K4b on y0) [all-reduce]
//     preconditioner (block-Jacobi of Hcc, or of the Schur diagonal)      [all-reduce]
//     PCG on S dc = g: per iteration K4a (by point), K4b (by camera) [all-reduce], K5
//     K7a camera update, K6 back substitution, K1 cost at the trial point  [all-reduce]
//     gain ratio -> accept (swap buffers) / reject (raise lambda)
#include <dlfcn.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <unistd.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <cassert>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ba_hip.h"
#include "ba_kernels.hpp"
#include "ba_triangulate.hpp"
#include "ba_small.hpp"
#include "ba_small_mw.hpp"
#include "ba_setup.hpp"
#include "ba_cov.hpp"
#include "ba_tracks.hpp"
#include "ba_similarity.hpp"
#include "ba_resect.hpp"
#include "ba_hypothesis.hpp"
#include "ba_ransac.hpp"
#include "ba_relpose.hpp"
#include "ba_homography.hpp"
#include "ba_match.hpp"
#include "ba_match_guided.hpp"
#include "ba_match_l2.hpp"
#include "ba_orb.hpp"
#include "ba_klt.hpp"
#include "ba_posegraph.hpp"
#include "ba_sim3.hpp"
#include "ba_fundamental.hpp"
#include "ba_bow.hpp"
#include "ba_trackbuild.hpp"

using namespace ba;

// ---------------------------------------------------------------------------- errors
static thread_local std::string g_err;
static int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}
static bool loss_valid(int32_t loss) { return loss >= BA_LOSS_LINEAR && loss <= BA_LOSS_ARCTAN; }
static_assert(LOSS_LINEAR == BA_LOSS_LINEAR && LOSS_HUBER == BA_LOSS_HUBER && LOSS_SOFT_L1 == BA_LOSS_SOFT_L1 &&
              LOSS_CAUCHY == BA_LOSS_CAUCHY && LOSS_ARCTAN == BA_LOSS_ARCTAN, "device loss codes (ba_device.hpp)");
#define HIPCHECK(expr)                                                                      \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess)                                                                   \
      return fail(BA_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

extern "C" const char* ba_last_error(void) { return g_err.c_str(); }

static const char* kKernelNames[BA_PROFILE_SLOTS] = {
    "cam_prepare", "residual_cam", "linearize_cam", "linearize_pt", "point_invert", "schur_pt",
    "schur_cam", "pcg_step", "precond", "backsub_pt", "misc", "allreduce", "schur_pt_then_backsub", "tracks", "resect", "resect_ransac"};
extern "C" const char* ba_kernel_name(int slot) {
  return (slot >= 0 && slot < BA_PROFILE_SLOTS) ? kKernelNames[slot] : "";
}

// ------------------------------------------------------------------------------ RCCL
struct Rccl {
  void* lib = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
};
static Rccl g_rccl;
static int load_rccl() {
  if (g_rccl.lib) return BA_OK;
  void* lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
  if (!lib) lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
  if (!lib) return fail(BA_ERR_COMM, "dlopen(librccl.so) failed: %s", dlerror());
  g_rccl.GetUniqueId = (decltype(g_rccl.GetUniqueId))dlsym(lib, "ncclGetUniqueId");
  g_rccl.CommInitRank = (decltype(g_rccl.CommInitRank))dlsym(lib, "ncclCommInitRank");
  g_rccl.AllReduce = (decltype(g_rccl.AllReduce))dlsym(lib, "ncclAllReduce");
  g_rccl.CommDestroy = (decltype(g_rccl.CommDestroy))dlsym(lib, "ncclCommDestroy");
  g_rccl.GetErrorString = (decltype(g_rccl.GetErrorString))dlsym(lib, "ncclGetErrorString");
  if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.AllReduce || !g_rccl.CommDestroy)
    return fail(BA_ERR_COMM, "librccl.so lacks an expected symbol");
  g_rccl.lib = lib;
  return BA_OK;
}

// ----------------------------------------------------------------------------- roctx
// Optional named ranges around the phases of an LM iteration (BA_ROCTX=1): they show up in rocprofv3
// --marker-trace timelines.  libroctx64 is loaded on demand; without it, or without the variable, nothing happens.
struct Roctx {
  bool tried = false;
  int (*push)(const char*) = nullptr;
  int (*pop)() = nullptr;
};
static Roctx g_roctx;
static void roctx_load() {
  if (g_roctx.tried) return;
  g_roctx.tried = true;
  if (!getenv("BA_ROCTX")) return;
  void* lib = dlopen("libroctx64.so.4", RTLD_NOW | RTLD_GLOBAL);
  if (!lib) lib = dlopen("libroctx64.so", RTLD_NOW | RTLD_GLOBAL);
  if (!lib) return;
  g_roctx.push = (int (*)(const char*))dlsym(lib, "roctxRangePushA");
  g_roctx.pop = (int (*)())dlsym(lib, "roctxRangePop");
  if (!g_roctx.push || !g_roctx.pop) { g_roctx.push = nullptr; g_roctx.pop = nullptr; }
}
struct Range {        // host-side range: covers the launches (and host waits) of one phase
  bool on;
  explicit Range(const char* name) : on(g_roctx.push != nullptr) { if (on) g_roctx.push(name); }
  ~Range() { if (on) g_roctx.pop(); }
};

// ---------------------------------------------------------------------------- handle
template <typename T>
struct DBuf {
  T* p = nullptr;
  size_t n = 0;
  // a NEW allocation comes back zero-filled (once: callers do not clear buffers on every use)
  hipError_t alloc(size_t count) {
    if (p && n >= count && count > 0) return hipSuccess;
    release();
    if (count == 0) return hipSuccess;
    // small buffers get headroom: consecutive sliding windows differ a little in size, and a hipFree + hipMalloc per
    // buffer on every growth costs more than the solve of such a window
    if (count < ((size_t)1 << 20)) count += count / 2 + 64;
    n = count;
    hipError_t e = hipMalloc((void**)&p, count * sizeof(T));
    if (e != hipSuccess) { p = nullptr; n = 0; return e; }
    // hipMemset of device memory may return before the fill has run (it is queued on the null stream, which the handle's
    // non-blocking stream does not wait for): drain it, or the zeros can land on top of the first upload.  Allocations are rare.
    e = hipMemset(p, 0, count * sizeof(T));
    if (e != hipSuccess) return e;
    return hipStreamSynchronize(nullptr);
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
  DBuf() = default;
  DBuf(const DBuf&) = delete;
  DBuf& operator=(const DBuf&) = delete;
  ~DBuf() { release(); }
};

// Grow-only pinned host buffer the stream copies from (or into) asynchronously.  mark() records the stream's last use of
// it; wait() blocks until that has landed, so the buffer may be refilled.
struct PinnedStage {
  char* p = nullptr;
  size_t cap = 0;
  hipEvent_t event = nullptr;
  bool pending = false;
  PinnedStage() = default;
  PinnedStage(const PinnedStage&) = delete;
  PinnedStage& operator=(const PinnedStage&) = delete;
  ~PinnedStage() { if (p) (void)hipHostFree(p); if (event) (void)hipEventDestroy(event); }
  void wait() { if (pending) (void)hipEventSynchronize(event); pending = false; }
  // at least `need` bytes: a smaller buffer is replaced by one of `grow_to` bytes (after draining `drain`, if given)
  hipError_t reserve(size_t need, size_t grow_to, hipStream_t drain = nullptr) {
    wait();
    if (cap >= need) return hipSuccess;
    if (p && drain) (void)hipStreamSynchronize(drain);
    if (p) (void)hipHostFree(p);
    p = nullptr; cap = 0;
    const hipError_t e = hipHostMalloc((void**)&p, grow_to, hipHostMallocDefault);
    if (e != hipSuccess) { p = nullptr; return e; }
    cap = grow_to;
    return hipSuccess;
  }
  hipError_t mark(hipStream_t stream) {
    hipError_t e = event ? hipSuccess : hipEventCreateWithFlags(&event, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(event, stream);
    pending = e == hipSuccess;
    return e;
  }
};

// The device memory of the calls that keep nothing on the device between calls: a bump arena over a list of blocks.
// Nothing is zero-filled: the bytes served another array in the call before, so a call uploads, clears or writes every word
// before a kernel reads it.
struct Scratch {
  struct Block { char* p; size_t cap; };
  struct Mark { size_t blk, off; };
  std::vector<Block> blocks;
  Mark at = {0, 0};                // where the next take starts
  size_t bytes = 0;                // the blocks' capacities together
  long long allocs = 0;            // hipMalloc calls since ba_create
  bool fresh = true, untidy = false;   // the call began on an empty arena; a call added blocks to the ones it found
  Scratch() = default;
  Scratch(const Scratch&) = delete;
  Scratch& operator=(const Scratch&) = delete;
  ~Scratch() { release(); }
  void release() {
    for (Block& b : blocks) (void)hipFree(b.p);
    blocks.clear();
    bytes = 0;
  }
  hipError_t open(size_t cap) {
    Block b = {nullptr, cap};
    const hipError_t e = hipMalloc((void**)&b.p, cap);
    if (e == hipSuccess) { blocks.push_back(b); bytes += cap; ++allocs; }
    return e;
  }
  // Starts a call.  After a call that added blocks to the ones it found, some lie unused: the stream is drained (that call may
  // have failed half way) and one block of their total size replaces them.  A first call's blocks are its takes exactly, and stay.
  hipError_t begin(hipStream_t stream) {
    at = {0, 0};
    fresh = blocks.empty();
    if (!untidy) return hipSuccess;
    untidy = false;
    const hipError_t e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return e;
    const size_t total = bytes;
    release();
    return open(total);
  }
  // n elements at a 256-byte boundary, valid until the call returns (n = 0: an address that is never read).  A take that fits
  // nowhere opens a block of its own size, so nothing handed out before moves.
  template <typename T>
  hipError_t take(size_t n, T** out) {
    const size_t need = (std::max<size_t>(n * sizeof(T), 1) + 255) & ~(size_t)255;
    while (at.blk < blocks.size() && blocks[at.blk].cap - at.off < need) at = {at.blk + 1, 0};
    if (at.blk == blocks.size()) {
      untidy = !fresh;
      const hipError_t e = open(need);
      if (e != hipSuccess) return e;
    }
    *out = (T*)(blocks[at.blk].p + at.off);
    at.off += need;
    return hipSuccess;
  }
  template <typename T, typename... Ts>
  hipError_t take(size_t n, T** out, Ts**... more) {      // several arrays of n elements each
    const hipError_t e = take(n, out);
    return e != hipSuccess ? e : take(n, more...);
  }
  // take, and the n elements queued for upload from src
  template <typename T>
  hipError_t put(hipStream_t stream, size_t n, const void* src, const T** out) {
    T* p = nullptr;
    hipError_t e = take(n, &p);
    if (e == hipSuccess && n > 0) e = hipMemcpyAsync(p, src, n * sizeof(T), hipMemcpyHostToDevice, stream);
    *out = p;
    return e;
  }
  Mark mark() const { return at; }   // rewind(mark()) gives back what was taken since
  void rewind(Mark m) { at = m; }
};

// The vocabulary tree of ba_vocab_train / ba_vocab_set as the host keeps it (ba_vocab_get reads it back from here)
struct BowVocab {
  int desc_bytes = 0, n_words = 0, branching = 0, levels = 0;
  std::vector<int32_t> child0, n_child, word_of_node, idf_q;
  std::vector<uint8_t> node_desc;
};

struct ba_handle {
  int device = 0;
  int n_cu = 256;              // compute units of the device (hipDeviceAttributeMultiprocessorCount)
  int model = 0;               // camera model of the running call: 0 = the reference's pinhole (Pinhole), 1 = BAL 9-parameter
                               // (BalCam, ba_models.hpp); every kernel of the loop is instantiated for both
  int lanes = LPP;             // lanes per point in the point passes: 2, or 4 / 8 / 16 for every point of a smaller problem
  int cam_band = 0;            // camera passes: XCD x takes camera range x (1) or partition x of every camera (0); see group_of_block
  hipStream_t stream = nullptr;
  hipStream_t stream2 = nullptr;   // second stream: test hook ba_debug_occupy only
  bool have_problem = false, have_params = false, linearized = false;
  ba_loss lin_loss = BA_LOSS_LINEAR;   // loss and f_scale of the last linearisation (ba_time_kernel)
  double lin_fscale = 1.0;
  int Nc = 0, Np = 0, Nobs = 0, fixed = -1;
  double K4[4] = {1, 1, 0, 0};
  // held parameters (ba_set_held): camera bit sets in camera order, point flags in point-slot order; the kernels get null
  // pointers while nothing is held.  held_x2: sum of the held points' |X|^2 at the current parameters -- constant, since a
  // held point never moves, and taken off the point share of |x| in the xtol test.  Host copies in the caller's orders.
  DBuf<unsigned short> cam_held;
  DBuf<unsigned char> pt_held, pt_held_in;
  bool any_cam_held = false, any_pt_held = false;
  unsigned cam_held_or = 0;        // OR of every camera's bits (pinhole solves refuse bits 6-8)
  std::vector<unsigned short> h_cam_held;
  std::vector<unsigned char> h_pt_held;
  double held_x2 = 0.0;
  DBuf<double> held_red;           // multi-rank: held_x2 summed over the shards (one all-reduce per solve)
  // shared intrinsics (ba_set_shared_intrinsics): groups of >= 2 cameras, numbered by their lowest member.  h_cam_gl[c] = -1
  // (own intrinsics) or 2 * group + (1: c is the group's leader, its lowest member); member lists CSR by group, members
  // ascending.  shared_on: a BAL solve is running with them (the kernels get null pointers otherwise).
  // The per-iteration fold cuts a group into chunks of SHARED_BLOCK members: h_chunk_rng[2 k], [2 k + 1] = chunk k's range in
  // h_grp_mem, h_grp_chunk[g] .. [g + 1] = the chunks of group g.
  std::vector<int> h_cam_gl, h_grp_off, h_grp_mem, h_chunk_rng, h_grp_chunk;
  DBuf<int> cam_gl, grp_off, grp_mem, chunk_rng, grp_chunk;
  DBuf<double> grp_rec, grp_w;     // k_shared_sum's record per group, k_shared_fold's sums per chunk
  int n_shared = 0, n_shared_chunks = 0;
  bool shared_on = false;
  // Gaussian priors (ba_set_priors): camera blocks in camera order, point blocks in point-slot order; the kernels get null
  // pointers while none are set.  Means of zero blocks are uploaded as 0 (they are never read by the caller's rule, and the
  // kernels then need no flag per block).  fold_prior_rows: PRIOR_ROWS while a solve folds the prior rows behind partR.
  DBuf<double> cam_info, cam_mean, pt_info, pt_mean, prior_in, prior_rows;
  bool any_cam_prior = false, any_pt_prior = false;
  int prior_nb = 0;
  long long prior_blocks = 0;
  int fold_prior_rows = 0;
  // observation lists (camera order, point order)
  DBuf<int> offk, c_pt, c_orig, pt_off, p_cam, slot, long_pts;
  DBuf<int> c_ptf[2], p_camf[2];  // index streams with the "weights are not (1, 1)" flag (robust loss; c_ptf pairs with c_w, p_camf with p_w)
  int long_thr = 16;           // tracks longer than this get a DPP row each (set in ba_set_problem)
  int n_long = 0, nblkL = 0;   // points with more than LONG_TRACK observations: one DPP row each, own launch
  int long_spb = PT_THREADS / LPP_LONG;   // long-track points per workgroup (a multiple of one round's 64)
  DBuf<int2> blk_win;          // per point-pass workgroup: first camera and number of cameras its points see
  bool uv_f32 = false;         // c_uv / p_uv hold float2 (every pixel of the problem is a float32 value: UvArr, ba_kernels.hpp)
  DBuf<double2> c_uv, p_uv, c_w[2], p_w[2];   // both halves of the linearisation are double-buffered: the next one is
                                              // computed speculatively at the trial point while the host decides
                                              // (camera half: c_w, c_ptf, partL [lb]; point half: p_w, p_camf, Hpp, bp, Hppinv, y0 [pb])
  // parameters (current / trial): cameras, camera state, point table
  DBuf<double> cams[2], cs[2], ptab[2], stage;
  int cur = 0;
  // camera table of the point passes, normal equations
  DBuf<double> camA[2], HccBc, Hpp[2], bp[2], Hppinv[2], y0[2], Hccd, Minv;
  int pb = 0;                  // which point-half buffer set holds the current linearisation
  // partial sums
  DBuf<double> partR, partL[2], part6, partE, partA, partB, partC, partV;
  DBuf<double> linmsg[2];            // multi-rank: a linearisation's camera half, folded, behind 8 header words (k_fold_lin)
  DBuf<double> sysmsg;               // multi-rank: the damped system's message [u.y, 0 | part6 | partE | world maxima] (k_fold_msg)
  DBuf<double> partG[2], partGc;   // per-workgroup max |bp| (point half, double-buffered like it) and max |bc| (k_pcg_setup): the gtol test
  int lb = 0;                  // which c_w / partL buffer holds the current linearisation
  // PCG vectors, comm buffers (multi-rank), scalars
  DBuf<double> gvec, x, r, p, s, z, vin, vx, scal, rbuf, gather;
  DBuf<PcgState> st;
  DBuf<double> tri;            // staging of ba_triangulate
  // ba_triangulate_tracks: per-slot results, camera centres, the BAL intrinsics of the call, caller-order outputs; the
  // launch arguments of the last call (what ba_time_kernel(BA_K_TRACKS) repeats; forgotten by ba_set_problem)
  DBuf<double> trk_out, trk_ctr, trk_intr, trk_res;
  DBuf<unsigned char> trk_status;
  TrackArgs trk_args = {};
  bool trk_valid = false, trk_bal = false;
  // What ba_resect (ba_resect.hpp) and ba_resect_ransac (ba_ransac.hpp) each keep of their last call: per-camera results, the
  // BAL intrinsics of the call, pt_known in point-slot order, cam_sel, and the launch arguments (what
  // ba_time_kernel(BA_K_RESECT / BA_K_RESECT_RANSAC) repeats).  rs_known_in, pt_known as given, is staging and shared.
  struct ResectSet {
    DBuf<double> out, intr;
    DBuf<unsigned char> known, sel;
    ResectArgs args = {};
    bool valid = false, bal = false;
  };
  ResectSet rs, rn;
  DBuf<unsigned char> rs_known_in;
  // ba_resect_ransac's own: the usable observations' records and their count per camera, the score blocks' best hypotheses,
  // the consensus bytes (camera order), obs_inlier (caller's order); rn_args.r is rn.args with the launch's pointers
  DBuf<double> rn_rec, rn_best;
  DBuf<int> rn_cnt;
  DBuf<unsigned char> rn_cons, rn_inl;
  RansacArgs rn_args = {};
  // Device memory of the calls that need no problem and keep nothing on the device between calls: the pair-shaped RANSAC
  // calls, matching, ORB, KLT tracking, the pose graph, place recognition (but for the resident vocabulary) and track building
  Scratch scratch;
  int debug_match_splits = 0;  // BA_DEBUG_MATCH_SPLITS: train splits asked for per pair instead of match_plan's own choice (tests)
  PinnedStage orb_stage;                       // what the call reads back: cs | xy size angle response | octave level_xy | n_kp | desc
  bool orb_timing = false;                     // ba_orb_stage_times: events around the stages of ba_orb_extract
  hipEvent_t orb_ev[BA_ORB_STAGES + 1] = {};
  double orb_ms[BA_ORB_STAGES] = {};
  bool klt_timing = false;                     // ba_klt_stage_times: events around the stages of ba_track_klt
  hipEvent_t klt_ev[BA_KLT_STAGES + 1] = {};
  double klt_ms[BA_KLT_STAGES] = {};
  // ba_transform / ba_align / ba_get_centres (ba_similarity.hpp): correspondences a | b | w | u | err (9 doubles each), the
  // per-workgroup partial rows, the device record (similarity, centroids, status)
  DBuf<double> sim_buf, sim_part;
  DBuf<SimRec> sim_rec;
  std::vector<ba_iter_record> pg_trace;   // ba_pose_graph: the trace of the last call
  int debug_pg_splits = 0;     // BA_DEBUG_PG_SPLITS: teams that share a hub node's incidence list instead of all 32 (tests)
  // place recognition (ba_bow.hpp): the resident vocabulary (host copy `vocab`, device arrays bw_child0 .. bw_ndesc)
  BowVocab vocab;
  DBuf<int> bw_child0, bw_nchild, bw_wordof, bw_idf;
  DBuf<unsigned long long> bw_ndesc;
  int debug_bow_chunk = 0;     // BA_DEBUG_BOW_CHUNK: database vectors per score workgroup instead of BW_CHUNK (tests)
  int debug_track_seg = 0;     // BA_DEBUG_TRACK_SEG: lowers the two segment-class thresholds of ba_build_tracks (tests)
  PinnedStage up;             // pinned arena of a window-sized problem's uploads (ba_set_problem: one copy, k_unpack_problem)
  char* h_small = nullptr;     // k_small_lm's results, host-mapped: ba_summary | int cur | trace records
  char* d_small_host = nullptr;
  size_t h_small_bytes = 0;
  long long small_seq = 0;     // sequence number of h_flags[4], which k_small_lm publishes when its results are written
  DBuf<double> intr[2];        // per-camera intrinsics (f, k1, k2) of the BAL model, current / trial like cams[]
  DBuf<double> small_V, small_gS;   // k_small_lm: V = W L (49 x 3 Np_pad, zero where unwritten), per-wave partial V V^T
  int small_np_pad = -1;
  PinnedStage par;             // pinned bounce buffer of ba_set_params / ba_get_params (window-sized problems)
  // k_small_mw (ba_small_mw.hpp): the window solver on mw_G workgroups; mw_ok: this problem fits its limits
  DBuf<int> mw_woff; DBuf<double> mw_buf; bool mw_ok = false; int mw_G = 0;
  int mw_resident[3] = {-1, -1, -1};   // workgroups of k_small_mw<2 / 3 / 4> the device holds at once (occupancy query, once per handle)
  long long stats[BA_STAT_COUNT] = {0};   // ba_get_stat
  DBuf<int> setup_i;                      // scratch of the device build of ba_set_problem (ba_setup.hpp)
  DBuf<char> up_dev;                      // device copy of the pinned upload arena `up`
  char* h_setup = nullptr;                // pinned: what that build reads back (track-length histogram, statistics, windows)
  int setup_path = 0;                     // how the current problem's layout was built: 0 host, 1 device
  DBuf<double> stat2;                     // multi-rank: the band statistic (span sum, tracks) summed over the shards
  bool banded_known = false;              // ... already decided for the problem being set (device build that fell back to the host build)
  bool banded = false;         // mean camera span of a track <= Nc / 8 (sequential captures): pcg_model_tol's automatic default
  DBuf<double> dev_lam;        // device word a riding k_scalars stores the next damping in; 0 = not yet (ba_kernels.hpp, ScalarsArgs::lam_slot)
  DBuf<double> verdict;        // PCG verdict words {gamma, zeta, finished, -} x 2 iteration parities (point pass -> camera pass, vector kernel)
  int cam_segl = 64;           // lanes per (camera, partition) segment in the PCG camera pass: 16 or 64
  int nblkP = 1, ppb = 1;
  int nblkVm[2] = {1, 1};      // camera-vector workgroups per camera model (CM::VC cameras each; [0] also k_lin_finalize's, VEC_CAMS each)
  size_t lds_bytes_m[2] = {0, 0};   // dynamic LDS of the point passes (largest window that fits), per camera model (row strides differ)
  bool jac_f32 = false;        // PCG passes recompute the Jacobian blocks in fp32 (ba_options.jacobian_precision = 1)
  bool all_lds_m[2] = {true, true};  // every point-pass workgroup's camera window fits in LDS, per camera model
  // pinned host mirror for scalars
  double* h_scal = nullptr;
  double* d_scal_host = nullptr;   // device-side address of h_scal (host-mapped, coherent)
  long long* h_flags = nullptr;    // host-mapped progress words: [0..1] PCG verdicts, [2..3] step scalars
  long long* d_flags = nullptr;
  long long flag_base = 1, step_seq = 1;
  // comm
  int rank = 0, world = 1;
  bool sys_diag = false;   // the last exchange_system carried Schur-Jacobi blocks (layout of sysmsg)
  bool multi = false;          // the multi-rank control flow is on: world > 1, or a communicator of ONE rank was forced
                               // (BA_COMM_FORCE=1: lets a single GPU execute every fold / all-reduce / decide step of the
                               // multi-rank loop through the real RCCL library)
  ncclComm_t nccl = nullptr;
  // host-staged shared-memory transport (BA_COMM=shm): a test vehicle that lets several ranks
  // share ONE GPU (RCCL refuses that), so the multi-rank control flow can be exercised end to end
  struct ShmComm* shm = nullptr;
  // device-side exchange of the per-PCG-iteration message through IPC-mapped peer buffers (BA_IPC=1; ba_kernels.hpp)
  struct IpcComm* ipc = nullptr;
  // first failed kernel launch since the last check (hipGetLastError right behind every launch)
  hipError_t launch_err = hipSuccess;
  char launch_what[160] = {0};
  int debug_lds_extra = 0;     // BA_DEBUG_LDS_EXTRA: bytes added to the point passes' dynamic LDS (tests provoke a failed launch)
  std::vector<ba_iter_record> trace;   // one record per LM iteration of the last ba_solve
  // profiling
  bool profile = false;
  std::vector<hipEvent_t> ev;
  std::vector<int> ev_slot;
  size_t ev_used = 0, n_flushes = 0;
  ba_profile prof = {};
  std::vector<float> prof_ms[BA_PROFILE_SLOTS];   // every measured duration, per slot
  ~ba_handle() {               // (the device buffers and pinned stages free themselves)
    for (void* q : {(void*)h_setup, (void*)h_small, (void*)h_scal, (void*)h_flags}) if (q) (void)hipHostFree(q);
  }
};

// What the host needs of a camera model (ba_models.hpp), indexed like ba_handle::model
struct ModelDims { int nb, nh, nl, vc; };
static constexpr ModelDims kModel[2] = {{Pinhole::NB, Pinhole::NH, Pinhole::NL, Pinhole::VC}, {BalCam::NB, BalCam::NH, BalCam::NL, BalCam::VC}};
static_assert(Pinhole::ID == 0 && BalCam::ID == 1 && VEC_CAMS == Pinhole::VC, "kModel / nblkVm are indexed by the model's ID");

// Every kernel launch goes through BA_LAUNCH: a launch the runtime refuses (dynamic LDS above the limit, an empty
// grid, ...) is not reported by a later stream synchronise, so the error is picked up right here and kept in the
// handle until the next check_launches().
static void note_launch(ba_handle* h, const char* what) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess && h->launch_err == hipSuccess) {
    h->launch_err = e;
    snprintf(h->launch_what, sizeof h->launch_what, "%s", what);
  }
}
#define BA_LAUNCH(kern, ...)                  \
  do {                                        \
    hipLaunchKernelGGL(kern, __VA_ARGS__);    \
    note_launch(h, #kern);                    \
  } while (0)
// The statement (one call or one launch) with CM = BalCam when bal, else with CM = Pinhole: how every launch and launch helper picks the
// instantiation of its camera model (ba_models.hpp) -- h->model inside the loop, the call's own flag in the stand-alone
// features (tracks, resection)
#define BA_BY_MODEL(bal, ...)                          \
  do {                                                 \
    if (bal) { using CM = BalCam; __VA_ARGS__; }       \
    else { using CM = Pinhole; __VA_ARGS__; }          \
  } while (0)
static int check_launches(ba_handle* h);
// drain the stream, then report the first launch that failed since the last check (a refused launch leaves the
// outputs stale without making the synchronise fail)
#define BA_SYNC(h)                                            \
  do {                                                        \
    HIPCHECK(hipStreamSynchronize((h)->stream));              \
    if (int rc_sync_ = check_launches(h)) return rc_sync_;    \
  } while (0)
static int check_launches(ba_handle* h) {
  if (h->launch_err == hipSuccess) return BA_OK;
  const hipError_t e = h->launch_err;
  h->launch_err = hipSuccess;
  return fail(BA_ERR_HIP, "launch of kernel %s failed: %s", h->launch_what, hipGetErrorString(e));
}

static int set_device(ba_handle* h) {
  HIPCHECK(hipSetDevice(h->device));
  return BA_OK;
}

extern "C" int ba_device_count(int* n) {
  if (!n) return fail(BA_ERR_INVALID, "null argument");
  HIPCHECK(hipGetDeviceCount(n));
  return BA_OK;
}

// the LDS-table point passes need more than the default 64 KB of dynamic LDS
template <typename F>
static hipError_t allow_big_lds(F* f) {
  return hipFuncSetAttribute((const void*)f, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_TAB_BYTES);   // the largest table a launch asks for
}

static int create_impl(ba_handle* h, int device_id) {
  HIPCHECK(hipSetDevice(device_id));
  HIPCHECK(hipDeviceGetAttribute(&h->n_cu, hipDeviceAttributeMultiprocessorCount, device_id));
  if (h->n_cu < 1) h->n_cu = 1;
  HIPCHECK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  HIPCHECK(hipHostMalloc((void**)&h->h_scal, 64 * sizeof(double), hipHostMallocMapped | hipHostMallocCoherent));
  HIPCHECK(hipHostGetDevicePointer((void**)&h->d_scal_host, h->h_scal, 0));
  HIPCHECK(hipHostMalloc((void**)&h->h_flags, 8 * sizeof(long long), hipHostMallocMapped | hipHostMallocCoherent));
  memset(h->h_flags, 0, 8 * sizeof(long long));
  HIPCHECK(hipHostGetDevicePointer((void**)&h->d_flags, h->h_flags, 0));
#define BA_BIG_LDS(K) HIPCHECK(allow_big_lds(K))
#define BA_BIG_LDS_LIN(CM, R, L) BA_BIG_LDS((k_pt_linearize<CM, R, L, 2>)); BA_BIG_LDS((k_pt_linearize<CM, R, L, 4>));        \
  BA_BIG_LDS((k_pt_linearize<CM, R, L, 8>)); BA_BIG_LDS((k_pt_linearize<CM, R, L, 16>)); BA_BIG_LDS((k_pt_linearize_both<CM, R, L>))
#define BA_BIG_LDS_SCH1(CM, R, M, L, LN) BA_BIG_LDS((k_pt_schur<CM, R, M, L, LN, double>)); BA_BIG_LDS((k_pt_schur<CM, R, M, L, LN, float>))
#define BA_BIG_LDS_SCH(CM, R, M, L) BA_BIG_LDS_SCH1(CM, R, M, L, 2); BA_BIG_LDS_SCH1(CM, R, M, L, 4); BA_BIG_LDS_SCH1(CM, R, M, L, 8);     \
  BA_BIG_LDS_SCH1(CM, R, M, L, 16); BA_BIG_LDS((k_pt_schur_both<CM, R, M, L, double>)); BA_BIG_LDS((k_pt_schur_both<CM, R, M, L, float>))
#define BA_BIG_LDS_MODEL(CM)                                                                                                            \
  BA_BIG_LDS_LIN(CM, true, true); BA_BIG_LDS_LIN(CM, true, false); BA_BIG_LDS_LIN(CM, false, true); BA_BIG_LDS_LIN(CM, false, false);   \
  BA_BIG_LDS_SCH(CM, true, 0, true); BA_BIG_LDS_SCH(CM, true, 0, false); BA_BIG_LDS_SCH(CM, false, 0, true); BA_BIG_LDS_SCH(CM, false, 0, false); \
  BA_BIG_LDS_SCH(CM, true, 1, true); BA_BIG_LDS_SCH(CM, true, 1, false); BA_BIG_LDS_SCH(CM, false, 1, true); BA_BIG_LDS_SCH(CM, false, 1, false)
  BA_BIG_LDS_MODEL(Pinhole);
  BA_BIG_LDS_MODEL(BalCam);
#undef BA_BIG_LDS_MODEL
#undef BA_BIG_LDS_SCH
#undef BA_BIG_LDS_SCH1
#undef BA_BIG_LDS_LIN
#undef BA_BIG_LDS
  if (const char* e = getenv("BA_DEBUG_LDS_EXTRA")) h->debug_lds_extra = atoi(e);
  if (const char* e = getenv("BA_DEBUG_MATCH_SPLITS")) h->debug_match_splits = atoi(e);
  if (const char* e = getenv("BA_DEBUG_PG_SPLITS")) h->debug_pg_splits = atoi(e);
  if (const char* e = getenv("BA_DEBUG_BOW_CHUNK")) h->debug_bow_chunk = atoi(e);
  if (const char* e = getenv("BA_DEBUG_TRACK_SEG")) h->debug_track_seg = atoi(e);
  return BA_OK;
}
extern "C" int ba_destroy(ba_handle* h);
extern "C" int ba_create(int device_id, ba_handle** out) {
  if (!out) return fail(BA_ERR_INVALID, "null out pointer");
  *out = nullptr;
  int n = 0;
  HIPCHECK(hipGetDeviceCount(&n));
  if (device_id < 0 || device_id >= n) return fail(BA_ERR_INVALID, "device %d not in [0,%d)", device_id, n);
  ba_handle* h = new ba_handle();
  h->device = device_id;
  if (int rc = create_impl(h, device_id)) {      // nothing half-built leaks: stream, pinned blocks and the handle go
    const std::string msg = g_err;
    ba_destroy(h);
    g_err = msg;
    return rc;
  }
  *out = h;
  return BA_OK;
}

static void flush_profile(ba_handle* h);
static void shm_destroy(ba_handle* h);
static void ipc_destroy(ba_handle* h);
static int shm_init(ba_handle* h, int rank, int world, const void* id128);
static int ipc_init(ba_handle* h, int rank, int world, const void* id128);

extern "C" int ba_destroy(ba_handle* h) {
  if (!h) return BA_OK;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  if (h->nccl && g_rccl.CommDestroy) g_rccl.CommDestroy(h->nccl);
  ipc_destroy(h);
  shm_destroy(h);
  for (auto e : h->ev) (void)hipEventDestroy(e);
  for (auto e : h->orb_ev) if (e) (void)hipEventDestroy(e);
  for (auto e : h->klt_ev) if (e) (void)hipEventDestroy(e);
  if (h->stream2) { (void)hipStreamSynchronize(h->stream2); (void)hipStreamDestroy(h->stream2); }
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;                    // every buffer the handle owns goes with it
  return BA_OK;
}

extern "C" int ba_synchronize(ba_handle* h) {
  if (!h) return fail(BA_ERR_INVALID, "null handle");
  if (set_device(h)) return BA_ERR_HIP;
  BA_SYNC(h);
  return BA_OK;
}

// ------------------------------------------------------------------------------ comm
extern "C" int ba_comm_unique_id(void* id128) {
  if (!id128) return fail(BA_ERR_INVALID, "null id buffer");
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is expected to be 128 bytes");
  { const char* e = getenv("BA_COMM");
    if (e && strcmp(e, "shm") == 0) {               // any 128 unique bytes will do
      unsigned long long seed = (unsigned long long)getpid() * 2654435761ULL ^ (unsigned long long)std::chrono::steady_clock::now().time_since_epoch().count();
      unsigned char* o = (unsigned char*)id128;
      for (int i = 0; i < 128; ++i) { seed = seed * 6364136223846793005ULL + 1442695040888963407ULL; o[i] = (unsigned char)(seed >> 33); }
      return BA_OK;
    } }
  if (int rc = load_rccl()) return rc;
  ncclUniqueId id;
  ncclResult_t r = g_rccl.GetUniqueId(&id);
  if (r != ncclSuccess) return fail(BA_ERR_COMM, "ncclGetUniqueId: %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "?");
  memcpy(id128, &id, 128);
  return BA_OK;
}

extern "C" int ba_comm_init(ba_handle* h, int rank, int world, const void* id128) {
  if (!h) return fail(BA_ERR_INVALID, "null handle");
  if (world < 1 || rank < 0 || rank >= world) return fail(BA_ERR_INVALID, "rank %d / world %d", rank, world);
  h->rank = rank;
  h->world = world;
  h->multi = world > 1 || getenv("BA_COMM_FORCE") != nullptr;
  if (!h->multi) return BA_OK;
  if (!id128) return fail(BA_ERR_INVALID, "null id buffer");
  if (set_device(h)) return BA_ERR_HIP;
  // BA_IPC=1: the per-PCG-iteration exchange goes through IPC-mapped peer buffers (device-side stores + flags, consumed
  // inside k_pcg_step) instead of the base transport's all-reduce; everything else stays on the base transport
  if (const char* e = getenv("BA_IPC")) if (atoi(e) != 0) { if (int rc = ipc_init(h, rank, world, id128)) return rc; }
  { const char* e = getenv("BA_COMM"); if (e && strcmp(e, "shm") == 0) return shm_init(h, rank, world, id128); }
  if (int rc = load_rccl()) return rc;
  ncclUniqueId id;
  memcpy(&id, id128, 128);
  ncclResult_t r = g_rccl.CommInitRank(&h->nccl, world, id, rank);
  if (r != ncclSuccess) return fail(BA_ERR_COMM, "ncclCommInitRank: %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "?");
  return BA_OK;
}

// --------------------------------------------------------------------------- profile
static hipEvent_t next_event(ba_handle* h) {
  if (h->ev_used == h->ev.size()) {
    hipEvent_t e;
    (void)hipEventCreate(&e);
    h->ev.push_back(e);
  }
  return h->ev[h->ev_used++];
}
struct Scope {   // brackets one launch with two events when profiling
  ba_handle* h;
  Scope(ba_handle* hh, int slot) : h(hh) {
    if (h->profile) {
      h->ev_slot.push_back(slot);
      (void)hipEventRecord(next_event(h), h->stream);
    }
  }
  ~Scope() {
    if (h->profile) {
      (void)hipEventRecord(next_event(h), h->stream);
      if (h->ev_used >= 8192) flush_profile(h);
    }
  }
};
static void flush_profile(ba_handle* h) {
  if (h->ev_used == 0) return;
  (void)hipStreamSynchronize(h->stream);
  for (size_t i = 0; i + 1 < h->ev_used; i += 2) {
    float ms = 0;
    (void)hipEventElapsedTime(&ms, h->ev[i], h->ev[i + 1]);
    const int slot = h->ev_slot[i / 2];
    h->prof.launches[slot] += 1;
    h->prof.total_ms[slot] += ms;
    h->prof_ms[slot].push_back(ms);
  }
  h->ev_used = 0;
  h->ev_slot.clear();
  h->n_flushes++;
}
extern "C" int ba_get_profile(ba_handle* h, ba_profile* out) {
  if (!h || !out) return fail(BA_ERR_INVALID, "null argument");
  flush_profile(h);
  for (int sl = 0; sl < BA_PROFILE_SLOTS; ++sl) {
    // working launches: within [0.5, 4] x the 90th percentile (early exits below, rare host-side
    // hiccups between the two events above)
    std::vector<float> v = h->prof_ms[sl];
    h->prof.working_launches[sl] = 0;
    h->prof.working_ms[sl] = 0;
    if (v.empty()) continue;
    std::sort(v.begin(), v.end());
    const float ref = v[(size_t)(0.9 * (v.size() - 1))];
    for (float d : v) if (d >= 0.5f * ref && d <= 4.0f * ref) { h->prof.working_launches[sl]++; h->prof.working_ms[sl] += d; }
  }
  *out = h->prof;
  return BA_OK;
}
extern "C" int ba_reset_profile(ba_handle* h) {
  if (!h) return fail(BA_ERR_INVALID, "null handle");
  flush_profile(h);
  memset(&h->prof, 0, sizeof h->prof);
  for (auto& v : h->prof_ms) v.clear();
  return BA_OK;
}

// ------------------------------------------------------------- shared-memory transport
// Same semantics as the RCCL path (in-place sum / max all-reduce of doubles, identical bits
// on every rank), implemented with a POSIX shared-memory segment and host staging.  Slow by
// design; selected with BA_COMM=shm.  Never used unless asked for.
struct ShmComm {
  static constexpr size_t SLOT = 8u << 20;         // bytes per rank
  int rank = 0, world = 1;
  char name[64] = {0};
  unsigned char* base = nullptr;
  size_t bytes = 0;
  double* stage = nullptr;                          // pinned
  unsigned gen = 0;
  std::atomic<unsigned>* counter() { return reinterpret_cast<std::atomic<unsigned>*>(base); }
  std::atomic<unsigned>* sense() { return reinterpret_cast<std::atomic<unsigned>*>(base + 64); }
  double* slot(int r) { return reinterpret_cast<double*>(base + 4096 + (size_t)r * SLOT); }
  int barrier() {
    const unsigned my = ++gen;
    if (counter()->fetch_add(1, std::memory_order_acq_rel) + 1 == (unsigned)world) {
      counter()->store(0, std::memory_order_relaxed);
      sense()->store(my, std::memory_order_release);
    } else {
      const auto t0 = std::chrono::steady_clock::now();
      unsigned spins = 0;
      while (sense()->load(std::memory_order_acquire) < my) {
        if ((++spins & 0xffff) == 0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 60.0)
          return -1;
      }
    }
    return 0;
  }
};

static int shm_init(ba_handle* h, int rank, int world, const void* id128) {
  ShmComm* c = new ShmComm();
  c->rank = rank; c->world = world;
  const unsigned char* id = (const unsigned char*)id128;
  unsigned long long tag = 1469598103934665603ULL;
  for (int i = 0; i < 128; ++i) tag = (tag ^ id[i]) * 1099511628211ULL;
  snprintf(c->name, sizeof c->name, "/ba_hip_%016llx", tag);
  c->bytes = 4096 + (size_t)world * ShmComm::SLOT;
  int fd = shm_open(c->name, O_CREAT | O_RDWR, 0600);
  if (fd < 0) { delete c; return fail(BA_ERR_COMM, "shm_open(%s) failed", c->name); }
  if (ftruncate(fd, (off_t)c->bytes) != 0) { close(fd); delete c; return fail(BA_ERR_COMM, "ftruncate failed"); }
  c->base = (unsigned char*)mmap(nullptr, c->bytes, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
  close(fd);
  if (c->base == MAP_FAILED) { delete c; return fail(BA_ERR_COMM, "mmap failed"); }
  if (hipHostMalloc((void**)&c->stage, ShmComm::SLOT) != hipSuccess) { delete c; return fail(BA_ERR_HIP, "hipHostMalloc failed"); }
  h->shm = c;
  if (c->barrier()) return fail(BA_ERR_COMM, "shm barrier timed out at init");
  return BA_OK;
}
static void shm_destroy(ba_handle* h) {
  if (!h->shm) return;
  ShmComm* c = h->shm;
  (void)c->barrier();
  if (c->stage) (void)hipHostFree(c->stage);
  if (c->base) munmap(c->base, c->bytes);
  if (c->rank == 0) shm_unlink(c->name);
  delete c;
  h->shm = nullptr;
}
static int shm_allreduce(ba_handle* h, double* buf, size_t count, bool is_max) {
  ShmComm* c = h->shm;
  if (count * sizeof(double) > ShmComm::SLOT) return fail(BA_ERR_COMM, "shm all-reduce of %zu doubles exceeds the slot", count);
  HIPCHECK(hipMemcpyAsync(c->stage, buf, count * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  BA_SYNC(h);
  memcpy(c->slot(c->rank), c->stage, count * sizeof(double));
  if (c->barrier()) return fail(BA_ERR_COMM, "shm barrier timed out");
  for (size_t i = 0; i < count; ++i) {            // rank order: identical bits on every rank
    double a = c->slot(0)[i];
    for (int r = 1; r < c->world; ++r) a = is_max ? std::max(a, c->slot(r)[i]) : a + c->slot(r)[i];
    c->stage[i] = a;
  }
  if (c->barrier()) return fail(BA_ERR_COMM, "shm barrier timed out");
  HIPCHECK(hipMemcpyAsync(buf, c->stage, count * sizeof(double), hipMemcpyHostToDevice, h->stream));
  BA_SYNC(h);      // the staging buffer is reused by the next call
  return BA_OK;
}

// ------------------------------------------------------ device-side exchange over IPC-mapped peer buffers (BA_IPC=1)
// Every rank allocates a receive buffer ([2 parities][world][stride] doubles + flag lines) in fine-grained device memory,
// exports it with hipIpcGetMemHandle and opens every peer's; the handles travel through a small POSIX shared-memory
// board named after the communicator id (one node: what bench.py --gpus N runs on).  Used for the Schur product's
// exchange inside the PCG loop (inside k_pcg_step); every other collective keeps the base transport.
struct IpcComm {
  static constexpr size_t STRIDE = 32768;             // doubles per (parity, sender) slot: messages up to 256 KB (3600 BAL cameras)
  int rank = 0, world = 1;
  char name[64] = {0};
  unsigned char* board = nullptr;                     // shm: [64-byte counter line][64-byte sense line][world x 128 bytes of handle]
  size_t board_bytes = 0;
  unsigned gen = 0;
  void* local = nullptr;                              // own receive buffer (recv doubles, then the flag lines)
  void* opened[IPC_MAX_WORLD] = {nullptr};
  IpcPeers peers;
  long long seq = 0;
  size_t recv_doubles() const { return (size_t)2 * world * STRIDE; }
  size_t bytes() const { return recv_doubles() * sizeof(double) + (size_t)2 * world * IPC_MAX_BLOCKS * sizeof(unsigned long long); }
  std::atomic<unsigned>* counter() { return reinterpret_cast<std::atomic<unsigned>*>(board); }
  std::atomic<unsigned>* sense() { return reinterpret_cast<std::atomic<unsigned>*>(board + 64); }
  int barrier() {
    const unsigned my = ++gen;
    if (counter()->fetch_add(1, std::memory_order_acq_rel) + 1 == (unsigned)world) {
      counter()->store(0, std::memory_order_relaxed);
      sense()->store(my, std::memory_order_release);
    } else {
      const auto t0 = std::chrono::steady_clock::now();
      unsigned spins = 0;
      while (sense()->load(std::memory_order_acquire) < my)
        if ((++spins & 0xffff) == 0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 60.0) return -1;
    }
    return 0;
  }
};
static void ipc_destroy(ba_handle* h) {
  if (!h->ipc) return;
  IpcComm* c = h->ipc;
  if (c->board) (void)c->barrier();                   // nobody unmaps a buffer a peer may still be storing into
  for (int r = 0; r < c->world; ++r) if (c->opened[r]) (void)hipIpcCloseMemHandle(c->opened[r]);
  if (c->local) (void)hipFree(c->local);
  if (c->board) { munmap(c->board, c->board_bytes); if (c->rank == 0) shm_unlink(c->name); }
  delete c;
  h->ipc = nullptr;
}
static int ipc_init(ba_handle* h, int rank, int world, const void* id128) {
  if (world > IPC_MAX_WORLD) return fail(BA_ERR_COMM, "BA_IPC: at most %d ranks", IPC_MAX_WORLD);
  IpcComm* c = new IpcComm();
  h->ipc = c;
  c->rank = rank; c->world = world;
  const unsigned char* id = (const unsigned char*)id128;
  unsigned long long tag = 1469598103934665603ULL;
  for (int i = 0; i < 128; ++i) tag = (tag ^ id[i]) * 1099511628211ULL;
  snprintf(c->name, sizeof c->name, "/ba_ipc_%016llx", tag);
  c->board_bytes = 128 + (size_t)world * 128;
  int fd = shm_open(c->name, O_CREAT | O_RDWR, 0600);
  if (fd < 0) return fail(BA_ERR_COMM, "shm_open(%s) failed", c->name);
  if (ftruncate(fd, (off_t)c->board_bytes) != 0) { close(fd); return fail(BA_ERR_COMM, "ftruncate failed"); }
  void* m = mmap(nullptr, c->board_bytes, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
  close(fd);
  if (m == MAP_FAILED) return fail(BA_ERR_COMM, "mmap failed");
  c->board = (unsigned char*)m;
  // fine-grained device memory: peer stores are visible to this device's loads without cache maintenance
  if (hipExtMallocWithFlags(&c->local, c->bytes(), hipDeviceMallocFinegrained) != hipSuccess) {
    (void)hipGetLastError();
    return fail(BA_ERR_COMM, "BA_IPC: fine-grained device memory for the receive buffer is not available");
  }
  HIPCHECK(hipMemset(c->local, 0, c->bytes()));
  HIPCHECK(hipDeviceSynchronize());
  hipIpcMemHandle_t mine;
  if (hipIpcGetMemHandle(&mine, c->local) != hipSuccess) { (void)hipGetLastError(); return fail(BA_ERR_COMM, "hipIpcGetMemHandle failed"); }
  static_assert(sizeof(hipIpcMemHandle_t) <= 120, "handle does not fit its board slot");
  memcpy(c->board + 128 + (size_t)rank * 128, &mine, sizeof mine);
  const int dev_of_rank = h->device;
  memcpy(c->board + 128 + (size_t)rank * 128 + 120, &dev_of_rank, sizeof(int));
  if (c->barrier()) return fail(BA_ERR_COMM, "BA_IPC: board barrier timed out");
  for (int r = 0; r < world; ++r) {
    void* base = c->local;
    if (r != rank) {
      hipIpcMemHandle_t hd;
      memcpy(&hd, c->board + 128 + (size_t)r * 128, sizeof hd);
      int peer_dev = 0;
      memcpy(&peer_dev, c->board + 128 + (size_t)r * 128 + 120, sizeof(int));
      if (peer_dev != h->device) {                      // another GPU of the node: its memory has to be reachable from this one
        int can = 0;
        (void)hipDeviceCanAccessPeer(&can, h->device, peer_dev);
        if (can) { const hipError_t e = hipDeviceEnablePeerAccess(peer_dev, 0); if (e != hipSuccess) (void)hipGetLastError(); }
      }
      if (hipIpcOpenMemHandle(&base, hd, hipIpcMemLazyEnablePeerAccess) != hipSuccess) {
        (void)hipGetLastError();
        return fail(BA_ERR_COMM, "BA_IPC: hipIpcOpenMemHandle of rank %d's buffer failed", r);
      }
      c->opened[r] = base;
    }
    c->peers.recv[r] = (double*)base;
    c->peers.flags[r] = (unsigned long long*)((double*)base + c->recv_doubles());
  }
  if (c->barrier()) return fail(BA_ERR_COMM, "BA_IPC: board barrier timed out");
  return BA_OK;
}

static int allreduce(ba_handle* h, double* buf, size_t count, bool is_max = false) {
  if (!h->multi) return BA_OK;
  Scope sc(h, BA_K_ALLREDUCE);
  if (h->shm) return shm_allreduce(h, buf, count, is_max);
  ncclResult_t r = g_rccl.AllReduce(buf, buf, count, ncclDouble, is_max ? ncclMax : ncclSum, h->nccl, h->stream);
  if (r != ncclSuccess) return fail(BA_ERR_COMM, "ncclAllReduce: %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "?");
  return BA_OK;
}

// ---------------------------------------------------------------------------- problem
// The band statistic behind pcg_model_tol's automatic default (mean camera span of a track <= Nc / 8).  Tracks are split
// over the ranks of a multi-rank job by landmark, so the sums of the shards are the whole problem's: one small all-reduce
// makes every rank decide what a single rank would.  Collective: every rank's ba_set_problem calls it exactly once.
static int decide_banded(ba_handle* h, double span_sum, double tracks, int Nc) {
  if (h->multi) {
    HIPCHECK(h->stat2.alloc(2));
    const double v[2] = {span_sum, tracks};
    HIPCHECK(hipMemcpyAsync(h->stat2.p, v, sizeof v, hipMemcpyHostToDevice, h->stream));
    if (int rc = allreduce(h, h->stat2.p, 2)) return rc;
    double w[2];
    HIPCHECK(hipMemcpyAsync(w, h->stat2.p, sizeof w, hipMemcpyDeviceToHost, h->stream));
    BA_SYNC(h);
    span_sum = w[0]; tracks = w[1];
  }
  h->banded = tracks > 0 && span_sum / tracks <= Nc / 8.0;
  h->stats[BA_STAT_BANDED] = h->banded ? 1 : 0;
  h->banded_known = true;
  return BA_OK;
}
// Point-pass grid, part 1 (needs the problem's dimensions only): lanes per point, number and length of the point ranges,
// lanes per segment of the PCG camera pass.  Shared by the host and the device build of ba_set_problem.
// Point-pass workgroups walk contiguous point ranges, PT_THREADS / LPP points per round.  When the whole camera table fits
// in LDS (so a wider range cannot overflow it) no more workgroups are started than the chip holds at once -- each then
// walks several rounds with one table fill (C3 x 10: Schur point pass 133 -> 93 us); with camera windows the ranges stay
// one round long so that the windows stay narrow.  A smaller problem (a sliding window, a shard of a multi-GPU job) gives
// every point 4, 8 or 16 lanes instead of 2 -- more workgroups, fewer observations per lane -- the most for which the
// workgroups are still all resident at once.  BA_PT_BLOCKS / BA_PT_LANES override (tuning only).
struct PtGrid { bool table_fits; int per_cu, pts_per_pass, want; };
static PtGrid config_point_grid(ba_handle* h, int Nc, int Np, int No) {
  const size_t full_table = (size_t)Nc * TA * sizeof(double);
  const bool table_fits = full_table <= (size_t)LDS_TAB_BYTES;
  const int per_cu = !table_fits ? 1 : (int)std::max<size_t>(1, std::min<size_t>(2048 / PT_THREADS, (size_t)(160 * 1024) / (full_table + 1024)));
  h->lanes = LPP;
  for (int ln = 16; ln > LPP; ln >>= 1)
    if ((Np + PT_THREADS / ln - 1) / (PT_THREADS / ln) <= h->n_cu * per_cu) { h->lanes = ln; break; }
  if (const char* e = getenv("BA_PT_LANES")) { const int v = atoi(e); if (v == 2 || v == 4 || v == 8 || v == 16) h->lanes = v; }
  const int pts_per_pass = PT_THREADS / h->lanes;
  const int want = std::max(1, (Np + pts_per_pass - 1) / pts_per_pass);
  h->nblkP = std::min(want, 4096);
  if (table_fits) h->nblkP = std::min(h->nblkP, h->n_cu * per_cu);
  if (const char* e = getenv("BA_PT_BLOCKS")) h->nblkP = std::max(1, std::min(want, atoi(e)));
  // lanes per (camera, partition) segment in the PCG camera pass: a wave, or a 16-lane row when segments are short
  // (config 5: ~48 observations per segment -- a wave would walk it in one step with a quarter of its lanes idle and
  // pay the 64-lane reduction of every sum for it; measured 13.4 -> 12.1 us, C3's ~125-observation segments keep the wave)
  h->cam_segl = (Nc > 0 && (long long)No / Nc / NPART < 64) ? 16 : 64;
  h->ppb = std::max(1, (Np + h->nblkP - 1) / h->nblkP);
  return PtGrid{table_fits, per_cu, pts_per_pass, want};
}
// part 2a: the track length above which a point gets a 16-lane row of its own (med = element Np / 2 of the sorted lengths)
static void config_long_threshold(ba_handle* h, int med) {
  h->long_thr = std::max(8, 2 * med);
  if (h->lanes != LPP) h->long_thr = 0x7fffffff;           // more lanes per point already: no separate long-track rows
}
// part 2b: how the long tracks are dealt to workgroups, and -- when ranges plus long-track workgroups would not all be
// resident at once -- the grid with the fewest rounds per workgroup
static void config_long_grid(ba_handle* h, const PtGrid& g, int Np, int n_long) {
  h->n_long = n_long;
  h->long_spb = PT_THREADS / LPP_LONG;
  if (const char* e = getenv("BA_LONG_SLOTS")) h->long_spb = std::max(1, atoi(e)) * (PT_THREADS / LPP_LONG);
  h->nblkL = (h->n_long + h->long_spb - 1) / h->long_spb;
  // A point-pass workgroup is 1024 threads at 128 VGPRs: ONE per compute unit.  When one-round ranges plus one-round
  // long-track workgroups need somewhat more workgroups than the chip has units (config 5: 306 + 175 on 256), the
  // second wave of workgroups runs on part of the chip while the rest idles, and every workgroup pays its launch and its
  // window copy for one round of work.  A round (512 points at 2 lanes, 64 long tracks at 16) is latency-bound and costs
  // about the same whatever it holds, so the cost of a launch is the largest number of ROUNDS any workgroup walks:
  // choose the long-track workgroups' size (m rounds) and the ranges' length such that everything is resident at once and
  // that number is smallest (config 5: 168 ranges of 932 points + 88 x 128 long tracks, two rounds each; Schur point
  // pass 17.0 -> 15.2 us pinhole, 20.0 -> 18.0 us BAL camera).  Much larger WINDOWED problems (more than two rounds per
  // unit) keep one-round ranges: narrow windows matter more there.
  if (!getenv("BA_PT_BLOCKS") && (!g.table_fits || h->n_long > 0)) {
    int best_m = 0, best_cost = g.table_fits ? 0x7fffffff : 3, best_nb = 0;   // (table in LDS: ranges of any length share one fill)
    const bool pick_m = !getenv("BA_LONG_SLOTS") && h->n_long > 0;
    for (int m = 1; m <= (pick_m ? 4 : 1); ++m) {
      const int spb = pick_m ? m * (PT_THREADS / LPP_LONG) : h->long_spb;
      const int nl = (h->n_long + spb - 1) / spb;
      const int avail = h->n_cu - nl;
      if (avail < 1) continue;
      const int nb = std::min(g.want, avail);
      const int rounds = ((Np + nb - 1) / nb + g.pts_per_pass - 1) / g.pts_per_pass;
      const int cost = std::max(rounds, h->n_long > 0 ? spb / (PT_THREADS / LPP_LONG) : 0);
      if (cost < best_cost) { best_cost = cost; best_m = m; best_nb = nb; }
    }
    if (best_m && g.want + h->nblkL > h->n_cu) {
      if (pick_m) { h->long_spb = best_m * (PT_THREADS / LPP_LONG); h->nblkL = (h->n_long + h->long_spb - 1) / h->long_spb; }
      h->nblkP = best_nb;
      h->ppb = (Np + best_nb - 1) / best_nb;
    }
  }
}
// Every device buffer of a problem whose size follows from the problem's dimensions and the point-pass grid alone (h->Nc,
// Np, Nobs, nblkP, nblkL, multi, world are set).  Idempotent: a buffer that is large enough is kept.
static int alloc_solver_buffers(ba_handle* h) {
  const int Nc = h->Nc, Np = h->Np, No = h->Nobs;
  const size_t nobs1 = std::max(No, 1), np1 = std::max(Np, 1);
  const size_t nbv_max = (size_t)std::max(h->nblkVm[0], h->nblkVm[1]);
  HIPCHECK(h->c_pt.alloc(nobs1)); HIPCHECK(h->c_orig.alloc(nobs1)); HIPCHECK(h->p_cam.alloc(nobs1));
  HIPCHECK(h->c_uv.alloc(nobs1)); HIPCHECK(h->p_uv.alloc(nobs1));
  HIPCHECK(h->c_w[0].alloc(nobs1)); HIPCHECK(h->c_w[1].alloc(nobs1)); HIPCHECK(h->p_w[0].alloc(nobs1)); HIPCHECK(h->p_w[1].alloc(nobs1));
  HIPCHECK(h->c_ptf[0].alloc(nobs1)); HIPCHECK(h->c_ptf[1].alloc(nobs1)); HIPCHECK(h->p_camf[0].alloc(nobs1)); HIPCHECK(h->p_camf[1].alloc(nobs1));
  for (int k = 0; k < 2; ++k) {
    HIPCHECK(h->cams[k].alloc(6 * (size_t)Nc)); HIPCHECK(h->cs[k].alloc(CS * (size_t)Nc));
    HIPCHECK(h->ptab[k].alloc(PT * np1));     // (k_pack_points writes whole records of set 0; set 1 gets X from the back
  }                                           //  substitution and y from the point half before either is read)
  HIPCHECK(h->stage.alloc(3 * np1));
  // per-camera buffers are sized for the larger camera model (BAL: 9 parameters, 45 + 9 sums, 26-double table rows)
  constexpr size_t NBX = BalCam::NB, NHX = BalCam::NH, NLX = BalCam::NL;
  HIPCHECK(h->camA[0].alloc(TA_MAX * (size_t)Nc)); HIPCHECK(h->camA[1].alloc(TA_MAX * (size_t)Nc));
  HIPCHECK(h->intr[0].alloc(3 * (size_t)Nc)); HIPCHECK(h->intr[1].alloc(3 * (size_t)Nc));
  HIPCHECK(h->HccBc.alloc(NLX * (size_t)Nc + 8));   // Hcc (NH Nc) | bc (NB Nc): one all-reduce
  for (int k = 0; k < 2; ++k) {
    HIPCHECK(h->Hpp[k].alloc(6 * np1)); HIPCHECK(h->bp[k].alloc(3 * np1)); HIPCHECK(h->Hppinv[k].alloc(6 * np1));
    HIPCHECK(h->y0[k].alloc(3 * np1));
  }
  h->pb = h->lb = 0;          // (both halves of the linearisation start in buffer set 0)
  HIPCHECK(h->Hccd.alloc(NHX * (size_t)Nc)); HIPCHECK(h->Minv.alloc(NHX * (size_t)Nc));
  HIPCHECK(h->partR.alloc(2 * (size_t)NPART * Nc + 2 * PRIOR_ROWS));   // + the prior rows of a solve with priors (k_prior_cost)
  HIPCHECK(h->partL[0].alloc(NLX * (size_t)NPART * Nc)); HIPCHECK(h->partL[1].alloc(NLX * (size_t)NPART * Nc));
  HIPCHECK(h->part6.alloc(NBX * (size_t)NPART * Nc + 8));   // + the u.y word: one all-reduce carries both
  HIPCHECK(h->partE.alloc(NHX * (size_t)NPART * Nc));
  if (h->multi) { HIPCHECK(h->linmsg[0].alloc(8 + NLX * (size_t)Nc)); HIPCHECK(h->linmsg[1].alloc(8 + NLX * (size_t)Nc)); }
  if (h->multi) HIPCHECK(h->sysmsg.alloc(2 + (size_t)(NBX + NHX) * Nc + (size_t)h->world + 8));
  HIPCHECK(h->partA.alloc(h->nblkP + h->nblkL)); HIPCHECK(h->partB.alloc(4 * (size_t)(h->nblkP + h->nblkL)));
  HIPCHECK(h->partC.alloc(5 * nbv_max)); HIPCHECK(h->partV.alloc(4 * nbv_max));
  HIPCHECK(h->partG[0].alloc(h->nblkP + h->nblkL)); HIPCHECK(h->partG[1].alloc(h->nblkP + h->nblkL)); HIPCHECK(h->partGc.alloc(nbv_max));
  DBuf<double>* v6[] = {&h->gvec, &h->x, &h->r, &h->p, &h->s, &h->z, &h->vin, &h->vx};
  for (auto b : v6) HIPCHECK(b->alloc(NBX * (size_t)Nc));
  HIPCHECK(h->scal.alloc(64));
  HIPCHECK(h->st.alloc(2));
  HIPCHECK(h->verdict.alloc(8));
  HIPCHECK(hipMemsetAsync(h->verdict.p, 0, 8 * sizeof(double), h->stream));
  HIPCHECK(h->dev_lam.alloc(2));
  // (dev_lam is cleared by every back substitution; camA rows: geometry by k_cam_prepare / k_cam_update, vt by the
  //  PCG setup before any pass reads it)
  return BA_OK;
}

// ---- ba_set_problem: a device build for large problems, the host build for the others (bit-equal where both apply)
constexpr int SETUP_HIST_BINS = 4096;
constexpr size_t SETUP_PINNED_BYTES = 128 * 1024;
constexpr long SETUP_DEVICE_MIN_OBS = 50000;   // smallest problem ba_set_problem lays out on the device (unless BA_SETUP says)
// BA_PIXELS=f64 keeps the pixel streams double2 whatever the values (A / B measurements, tests)
static bool uv_f32_wanted() {
  const char* e = getenv("BA_PIXELS");
  return !(e && strcmp(e, "f64") == 0);
}
static inline UvArr uv_arr(const ba_handle* h, const DBuf<double2>& b) { return UvArr{b.p, h->uv_f32 ? 1 : 0}; }
// out[i] = sum of in[0 .. i), out[n] = total, for any n < 2^31: k_scan_* passes of at most 1024 * SETUP_SCAN_BLOCK items, the
// running total carried into the next pass through its block sums (so an n within one pass is three launches).  in and out are
// different arrays; bsum holds 1026 ints.
static int dev_scan(ba_handle* h, const int* in, size_t n, int* bsum, int* out) {
  const size_t pass = (size_t)1024 * SETUP_SCAN_BLOCK;
  if (n == 0) { HIPCHECK(hipMemsetAsync(out, 0, sizeof(int), h->stream)); return BA_OK; }
  for (size_t c0 = 0; c0 < n; c0 += pass) {
    const int nc = (int)std::min(pass, n - c0), nb = (nc + SETUP_SCAN_BLOCK - 1) / SETUP_SCAN_BLOCK;
    BA_LAUNCH(k_scan_block_sums, dim3(nb), dim3(1024), 0, h->stream, in + c0, nc, bsum);
    BA_LAUNCH(k_scan_top, dim3(1), dim3(1024), 0, h->stream, bsum, nb);
    if (c0 > 0) BA_LAUNCH(k_tb_scan_base, dim3(1), dim3(1024), 0, h->stream, bsum, nb, (const int*)(out + c0));   // = the previous pass's total
    BA_LAUNCH(k_scan_final, dim3(nb), dim3(1024), 0, h->stream, in + c0, nc, (const int*)bsum, out + c0);
  }
  return BA_OK;
}
// BA_TIME_SETUP=1: one stderr line per stage of ba_set_problem, with the time since the previous line.  A device-build
// stage drains the stream first.
struct StageClock {
  const bool on = getenv("BA_TIME_SETUP") != nullptr;
  std::chrono::steady_clock::time_point t_prev = std::chrono::steady_clock::now();
  void operator()(const char* name, hipStream_t device_stream = nullptr) {
    if (!on) return;
    if (device_stream) (void)hipStreamSynchronize(device_stream);
    const auto t = std::chrono::steady_clock::now();
    const double ms = std::chrono::duration<double, std::milli>(t - t_prev).count();
    fprintf(stderr, "ba_set_problem %s%-*s %8.3f ms\n", device_stream ? "[device] " : "", device_stream ? 24 : 28, name, ms);
    t_prev = t;
  }
};
// The part of a problem's state both builds set alike: its dimensions ...
static void set_dimensions(ba_handle* h, int Nc, int Np, int No, const double K4[4], int fixed_cam) {
  h->Nc = Nc; h->Np = Np; h->Nobs = No; h->fixed = fixed_cam;
  memcpy(h->K4, K4, sizeof h->K4);
  for (int m = 0; m < 2; ++m) h->nblkVm[m] = (Nc + kModel[m].vc - 1) / kModel[m].vc;
}
// ... and the point passes' dynamic LDS, from every point-pass workgroup's camera window (first camera, number of cameras).
// A window is staged in LDS when its rows fit; the row stride depends on the camera model (18 doubles for the reference's
// pinhole, 26 for the BAL camera), so the LDS size and the "every window fits" flag are kept per model.
static void set_window_lds(ba_handle* h, const int2* win, size_t nwin) {
  const size_t row_bytes[2] = {Pinhole::TA * sizeof(double), BalCam::TA * sizeof(double)};
  for (int m = 0; m < 2; ++m) {
    h->lds_bytes_m[m] = 0; h->all_lds_m[m] = true;
    for (size_t b = 0; b < nwin; ++b) {
      const size_t bytes = (size_t)win[b].y * row_bytes[m];
      if (bytes <= (size_t)LDS_TAB_BYTES) h->lds_bytes_m[m] = std::max(h->lds_bytes_m[m], bytes);
      else h->all_lds_m[m] = false;
    }
  }
}
// Device build (ba_setup.hpp): one upload of the caller's arrays, every ordering derived by kernels.
// Returns BA_OK, a negative ba_status, or 1 = "not for this problem" (the caller then runs the host build; nothing the
// host build relies on has been touched).  Chosen for large problems whose whole camera table fits in LDS (the caller's
// point numbering is kept then); bit-equal to the host build (tests/test_gpu_setup.py).
static int set_problem_device(ba_handle* h, int Nc, int Np, int No, const int32_t* cam_idx, const int32_t* pt_idx, const double* uv,
                              const double K4[4], int fixed_cam) {
  StageClock clock;
  auto stage = [&](const char* name) { clock(name, h->stream); };
  if ((size_t)Np + 1 > (size_t)1024 * SETUP_SCAN_BLOCK) return 1;
  set_dimensions(h, Nc, Np, No, K4, fixed_cam);
  const PtGrid grid = config_point_grid(h, Nc, Np, No);
  if (!grid.table_fits) return 1;
  if (!h->h_setup) HIPCHECK(hipHostMalloc((void**)&h->h_setup, SETUP_PINNED_BYTES, hipHostMallocDefault));
  // observation-sized buffers the build works in; the flagged index copies serve as scratch until k_init_flagged fills them
  HIPCHECK(h->p_camf[0].alloc(No)); HIPCHECK(h->p_camf[1].alloc(No)); HIPCHECK(h->c_ptf[0].alloc(No)); HIPCHECK(h->c_ptf[1].alloc(No));
  HIPCHECK(h->p_cam.alloc(No)); HIPCHECK(h->c_pt.alloc(No)); HIPCHECK(h->c_orig.alloc(No));
  HIPCHECK(h->c_uv.alloc(No)); HIPCHECK(h->p_uv.alloc(No)); HIPCHECK(h->rbuf.alloc(2 * (size_t)No));
  HIPCHECK(h->pt_off.alloc(Np + 1)); HIPCHECK(h->offk.alloc((size_t)Nc * (NPART + 1))); HIPCHECK(h->slot.alloc(Np));
  // scratch: p_src[No] | cnt[Np+1] fill[Np] big[Np] flag[Np+1] pos[Np+1] | cam_cnt[Nc+1] cam_fill[Nc] cam_off[Nc+1] | bsum[1032] |
  //          hist[SETUP_HIST_BINS] | words[16] (0 bad, 1 n_tracks, 2 n_big) | u64[4] (0 span_sum, 1 in_partition, 2 in_band)
  const size_t o_cnt = (size_t)No, o_fill = o_cnt + Np + 1, o_big = o_fill + Np, o_flag = o_big + Np, o_pos = o_flag + Np + 1;
  const size_t o_ccnt = o_pos + Np + 1, o_cfill = o_ccnt + Nc + 1, o_coff = o_cfill + Nc, o_bsum = o_coff + Nc + 1;
  const size_t o_hist = o_bsum + 1032, o_words = o_hist + SETUP_HIST_BINS, o_u64 = (o_words + 16 + 1) & ~(size_t)1, o_end = o_u64 + 8;
  HIPCHECK(h->setup_i.alloc(o_end));
  int* const S = h->setup_i.p;
  int *d_cam = h->p_camf[0].p, *d_pt = h->p_camf[1].p, *seg = h->c_ptf[0].p, *p_pt = h->c_ptf[1].p, *p_src = S;
  unsigned long long* u64 = (unsigned long long*)(S + o_u64);
  HIPCHECK(hipMemcpyAsync(d_cam, cam_idx, (size_t)No * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHECK(hipMemcpyAsync(d_pt, pt_idx, (size_t)No * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHECK(hipMemcpyAsync(h->rbuf.p, uv, 2 * (size_t)No * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHECK(hipMemsetAsync(S + o_cnt, 0, (o_end - o_cnt) * sizeof(int), h->stream));
  HIPCHECK(hipMemsetAsync(S + o_words, 0x7f, sizeof(int), h->stream));                   // bad = 0x7f7f7f7f: "none"
  stage("upload");
  const dim3 go((No + 255) / 256), gp((Np + 255) / 256), b256(256);
  // (words: 0 first bad observation, 1 tracks, 2 big points, 3 "some pixel is not a float32 value")
  BA_LAUNCH(k_setup_hist, go, b256, 0, h->stream, (const int*)d_cam, (const int*)d_pt, No, Nc, Np, S + o_cnt, S + o_words,
            (uv_f32_wanted() && Nc > SMALL_MAX_CAMS) ? (const double2*)h->rbuf.p : (const double2*)nullptr, S + o_words + 3);
  if (int rc = dev_scan(h, S + o_cnt, Np, S + o_bsum, h->pt_off.p)) return rc;
  BA_LAUNCH(k_setup_scatter_pt, go, b256, 0, h->stream, (const int*)d_pt, No, (const int*)h->pt_off.p, S + o_fill, seg);
  BA_LAUNCH(k_setup_sort_pt, gp, b256, 0, h->stream, (const int*)h->pt_off.p, Np, (const int*)seg, (const int*)d_cam, p_src, h->p_cam.p, p_pt,
            S + o_hist, SETUP_HIST_BINS, u64, S + o_words + 1, S + o_big, S + o_words + 2);
  BA_LAUNCH(k_setup_sort_big, dim3(std::min(Np, 2048)), b256, 0, h->stream, (const int*)(S + o_big), (const int*)(S + o_words + 2),
            (const int*)h->pt_off.p, (const int*)seg, (const int*)d_cam, p_src, h->p_cam.p, p_pt, u64, S + o_words + 1);
  // read back: histogram of track lengths, words, span sum
  int* hh = (int*)h->h_setup;
  HIPCHECK(hipMemcpyAsync(hh, S + o_hist, (SETUP_HIST_BINS + 16) * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(hipMemcpyAsync(hh + SETUP_HIST_BINS + 16, u64, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
  BA_SYNC(h);
  stage("point order");
  const int bad = hh[SETUP_HIST_BINS + 0], n_tracks = hh[SETUP_HIST_BINS + 1];
  if (bad >= 0 && bad < No) {
    if (cam_idx[bad] < 0 || cam_idx[bad] >= Nc) return fail(BA_ERR_INVALID, "cam_idx[%lld]=%d out of range", (long long)bad, cam_idx[bad]);
    return fail(BA_ERR_INVALID, "pt_idx[%lld]=%d out of range", (long long)bad, pt_idx[bad]);
  }
  h->uv_f32 = uv_f32_wanted() && Nc > SMALL_MAX_CAMS && hh[SETUP_HIST_BINS + 3] == 0;
  unsigned long long span_sum;
  memcpy(&span_sum, hh + SETUP_HIST_BINS + 16, sizeof span_sum);
  // median track length = element Np / 2 of the sorted lengths
  int med = 0;
  { long long cum = 0; for (int L = 0; L < SETUP_HIST_BINS; ++L) { cum += hh[L]; if (cum > Np / 2) { med = L; break; } } }
  config_long_threshold(h, med);
  if (h->long_thr != 0x7fffffff && h->long_thr >= SETUP_HIST_BINS - 1) return 1;       // (the capped histogram cannot count those)
  int n_long = 0;
  if (h->long_thr != 0x7fffffff) for (int L = h->long_thr + 1; L < SETUP_HIST_BINS; ++L) n_long += hh[L];
  config_long_grid(h, grid, Np, n_long);
  if (int rc = decide_banded(h, (double)span_sum, (double)n_tracks, Nc)) return rc;
  h->mw_ok = false;
  HIPCHECK(h->long_pts.alloc(std::max(h->n_long, 1)));
  if (h->n_long > 0) {
    BA_LAUNCH(k_setup_long_flags, gp, b256, 0, h->stream, (const int*)h->pt_off.p, Np, h->long_thr, S + o_flag);
    if (int rc = dev_scan(h, S + o_flag, Np, S + o_bsum, S + o_pos)) return rc;
    BA_LAUNCH(k_setup_long_list, gp, b256, 0, h->stream, (const int*)h->pt_off.p, Np, h->long_thr, (const int*)(S + o_pos), h->long_pts.p);
  }
  if (h->lanes == LPP) {
    const long long nthreads = (long long)h->nblkP * ((h->ppb + 15) / 16) * 2;
    BA_LAUNCH(k_setup_bank_order, dim3((unsigned)((nthreads + 255) / 256)), b256, 0, h->stream, (const int*)h->pt_off.p, Np, h->nblkP, h->ppb,
              h->p_cam.p, p_src);
  }
  stage("long tracks + visiting order");
  // camera order (keys: positions of the point-ordered list)
  const dim3 gt((No + SETUP_CAM_TILE - 1) / SETUP_CAM_TILE);
  BA_LAUNCH(k_setup_hist_cam, gt, b256, (size_t)Nc * sizeof(int), h->stream, (const int*)h->p_cam.p, No, Nc, S + o_ccnt);
  if (int rc = dev_scan(h, S + o_ccnt, Nc, S + o_bsum, S + o_coff)) return rc;
  BA_LAUNCH(k_setup_scatter_cam, gt, b256, 2 * (size_t)Nc * sizeof(int), h->stream, (const int*)h->p_cam.p, No, Nc, (const int*)(S + o_coff),
            S + o_cfill, seg);
  BA_LAUNCH(k_setup_sort_cam, dim3(Nc), b256, 0, h->stream, (const int*)(S + o_coff), (const int*)seg, (const int*)p_pt, (const int*)p_src,
            h->c_pt.p, h->c_orig.p);
  BA_LAUNCH(k_setup_offk, dim3((Nc * (NPART + 1) + 255) / 256), b256, 0, h->stream, (const int*)(S + o_coff), Nc, h->offk.p);
  BA_LAUNCH(k_setup_xcd_stat, dim3(std::min((Nc * NPART + 3) / 4, 2 * h->n_cu)), b256, 0, h->stream, (const int*)h->offk.p, (const int*)h->c_pt.p, Nc, Np, u64 + 1);
  const int nwin = h->nblkP + h->nblkL;
  if ((size_t)nwin * sizeof(int2) + 64 > SETUP_PINNED_BYTES) return 1;
  HIPCHECK(h->blk_win.alloc(nwin));
  BA_LAUNCH(k_setup_windows, dim3(nwin), b256, 0, h->stream, (const int*)h->pt_off.p, (const int*)h->p_cam.p, Np, Nc, h->nblkP, h->ppb,
            (const int*)h->long_pts.p, h->n_long, h->long_spb, h->blk_win.p);
  HIPCHECK(hipMemcpyAsync(h->h_setup, u64 + 1, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(hipMemcpyAsync(h->h_setup + 64, h->blk_win.p, (size_t)nwin * sizeof(int2), hipMemcpyDeviceToHost, h->stream));
  // pixels into both orderings, flagged index copies, identity point numbering
  BA_LAUNCH(k_gather_uv, go, b256, 0, h->stream, (const double2*)h->rbuf.p, (const int*)p_src, No, h->p_uv.p, (int)h->uv_f32);
  BA_LAUNCH(k_gather_uv, go, b256, 0, h->stream, (const double2*)h->rbuf.p, (const int*)h->c_orig.p, No, h->c_uv.p, (int)h->uv_f32);
  BA_LAUNCH(k_init_flagged, go, b256, 0, h->stream, (const int*)h->c_pt.p, (const int*)h->p_cam.p, No, h->c_ptf[0].p, h->c_ptf[1].p,
            h->p_camf[0].p, h->p_camf[1].p);
  BA_LAUNCH(k_setup_iota, gp, b256, 0, h->stream, h->slot.p, Np);
  if (int rc = alloc_solver_buffers(h)) return rc;
  BA_SYNC(h);
  stage("camera order, windows, pixels");
  unsigned long long st2[2];
  memcpy(st2, h->h_setup, sizeof st2);
  h->cam_band = st2[1] > st2[0];
  set_window_lds(h, (const int2*)(h->h_setup + 64), nwin);
  h->setup_path = 1;
  return BA_OK;
}

// ---- host build: counting sorts of the caller's indices on the host, then one upload.  Same contract as the device build
// (BA_OK or a negative ba_status).  Each stage below works on plain vectors; only the grid helpers it shares with the
// device build (config_point_grid, config_long_*) and set_problem_host's last step write the handle.

// k_small_mw's plan: chosen (within its limits, every workgroup resident at once), workgroups, and per range boundary and
// camera the first observation of the camera's list in the range
struct MwPlan { bool ok = false; int G = 0; std::vector<int> woff; };
struct HostLayout {            // point order: pt_off, p_cam, p_src (caller's observation); camera order: cam_off, c_pt, c_orig
  std::vector<int> slot, pt_off, p_cam, p_src, long_pts, cam_off, c_pt, c_orig, offk;
  std::vector<int2> win;       // camera window (first camera, number of cameras) of every point-pass workgroup
  MwPlan mw;
};

// Internal point numbering (slot[p]: where the caller's point p sits in the point table).  When the whole camera table
// fits in LDS nothing is gained by moving points, so the caller's order is kept.  Otherwise points are sorted by the mean
// index of the cameras that observe them: consecutive points are then seen from a narrow window of cameras whenever the
// data has that locality (and per-camera partitions stay balanced when it has not).  Pure locality: results do not depend
// on it.
static std::vector<int> host_point_numbering(int Nc, int Np, int No, const int32_t* cam_idx, const int32_t* pt_idx) {
  std::vector<int> slot(Np);
  if ((size_t)Nc * TA * sizeof(double) <= (size_t)LDS_TAB_BYTES) {
    for (int p = 0; p < Np; ++p) slot[p] = p;
    return slot;
  }
  std::vector<double> sum(Np, 0.0);
  std::vector<int> n(Np, 0);
  for (int i = 0; i < No; ++i) { sum[pt_idx[i]] += cam_idx[i]; n[pt_idx[i]]++; }
  // The order a stable sort of the points by key gives, in two linear steps instead of a comparison sort with an indirect
  // key load per comparison (config 5: 9 of this stage's 13 ms): the keys lie in [0, Nc], so a stable counting sort by
  // floor(16 key) -- monotone in the key -- leaves a handful of points per bucket, finished by a stable insertion sort on
  // the exact keys
  constexpr int BK = 16;
  const size_t nbk = (size_t)(Nc + 1) * BK + 2;
  std::vector<int> bfirst(nbk + 1, 0);
  std::vector<std::pair<double, int>> order(Np);
  for (int p = 0; p < Np; ++p) {
    const double key = n[p] ? sum[p] / n[p] : (double)Nc;
    sum[p] = key;
    bfirst[(size_t)(key * BK) + 1]++;
  }
  for (size_t q = 0; q < nbk; ++q) bfirst[q + 1] += bfirst[q];
  {
    std::vector<int> fill(bfirst.begin(), bfirst.end() - 1);
    for (int p = 0; p < Np; ++p) order[fill[(size_t)(sum[p] * BK)]++] = std::make_pair(sum[p], p);
  }
  for (size_t q = 0; q < nbk; ++q)
    for (int a = bfirst[q] + 1; a < bfirst[q + 1]; ++a) {
      const std::pair<double, int> v = order[a];
      int w = a;
      while (w > bfirst[q] && order[w - 1].first > v.first) { order[w] = order[w - 1]; --w; }
      order[w] = v;
    }
  for (int r = 0; r < Np; ++r) slot[order[r].second] = r;
  return slot;
}

// Point order: stable counting sort by (internal) point, which keeps the caller's order inside a point.  Only the indices
// are permuted on the host; the pixels follow on the device (k_gather_uv, k_unpack_problem).
static void host_sort_by_point(int Np, int No, const int32_t* cam_idx, const std::vector<int>& pt, std::vector<int>& pt_off,
                               std::vector<int>& p_cam, std::vector<int>& p_src) {
  pt_off.assign(Np + 1, 0);
  for (int i = 0; i < No; ++i) pt_off[pt[i] + 1]++;
  for (int p = 0; p < Np; ++p) pt_off[p + 1] += pt_off[p];
  p_cam.resize(No); p_src.resize(No);
  std::vector<int> pc(pt_off.begin(), pt_off.end() - 1);
  for (int i = 0; i < No; ++i) {
    const int b = pc[pt[i]]++;
    p_cam[b] = cam_idx[i]; p_src[b] = i;
  }
}

// Long tracks -- more than max(8, 2 x median track length) observations -- get one DPP row (16 lanes) per point in a
// launch of their own.  Completes the point-pass grid (config_long_threshold, config_long_grid).
static std::vector<int> host_long_tracks(ba_handle* h, const PtGrid& grid, int Np, const std::vector<int>& pt_off) {
  int med = 0;
  if (Np > 0) {
    std::vector<int> len(Np);
    for (int p = 0; p < Np; ++p) len[p] = pt_off[p + 1] - pt_off[p];
    std::nth_element(len.begin(), len.begin() + Np / 2, len.end()); med = len[Np / 2];
  }
  config_long_threshold(h, med);
  std::vector<int> long_pts;
  for (int p = 0; p < Np; ++p) if (pt_off[p + 1] - pt_off[p] > h->long_thr) long_pts.push_back(p);
  config_long_grid(h, grid, Np, (int)long_pts.size());
  return long_pts;
}

// Bank-aware visiting order inside a point (2-lane point passes with the camera table in LDS), laid out for the ranges'
// final length.  A point pass reads a camera's 144-byte LDS row with nine ds_read_b128; the hardware serves such a read in
// groups of 16 lanes, and two lanes of a group collide when their rows fall into the same of 16 bank classes (row mod 16:
// the row stride is 36 dwords).  With random cameras a group sees ~3 lanes per class: SQ_LDS_BANK_CONFLICT was 64 % of
// the LDS cycles (profiles/).  The ORDER in which a point's observations are visited is free, so it is chosen here,
// greedily per group of eight points and per step, so that the sixteen rows read together are in distinct classes
// wherever the data allows.  Pure scheduling: every sum keeps a fixed order, results stay bit-reproducible.
static void bank_aware_order(const ba_handle* h, int Np, const std::vector<int>& pt_off, std::vector<int>& p_cam, std::vector<int>& p_src) {
  // ds_read_b128 is served in groups of SIXTEEN CONSECUTIVE LANES (measured on MI355X, tools/microbench/lds_b128_groups.hip:
  // rows with distinct bank classes inside every 16 consecutive lanes read as fast as a broadcast, 14.3 cycles per
  // instruction against 23.8 for random rows; distinct classes inside the lane sets {0-3,12-15,20-27} / {4-11,16-19,28-31}
  // that rounds 1-3 ordered for -- the guide's grouping -- still cost 19.9).  With 2 lanes per point: points 0-7 of a
  // 16-point chunk are one group, points 8-15 the other
  static const int group_of_pair[16] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1};
  for (int b = 0; b < h->nblkP; ++b) {
    const int p0 = std::min(Np, b * h->ppb), p1 = std::min(Np, (b + 1) * h->ppb);
    for (int c0 = p0; c0 < p1; c0 += 16) {              // one 32-lane half: 16 points, two groups of 8
      for (int g = 0; g < 2; ++g) {
        int pts[8], npts = 0;
        for (int q = 0; q < 16 && c0 + q < p1; ++q)
          if (group_of_pair[((c0 - p0) + q) & 15] == g) pts[npts++] = c0 + q;
        int maxlen = 0;
        for (int i = 0; i < npts; ++i) maxlen = std::max(maxlen, pt_off[pts[i] + 1] - pt_off[pts[i]]);
        if (maxlen > 64) continue;                      // (long tracks: their own launch, other mapping)
        // remaining observations of each point as a small list; at every step each point places up to two
        int cur[8];
        for (int i = 0; i < npts; ++i) cur[i] = pt_off[pts[i]];
        for (int step = 0; 2 * step < maxlen; ++step) {
          unsigned used = 0;                            // bank classes taken in this step
          for (int i = 0; i < npts; ++i) {
            const int end = pt_off[pts[i] + 1];
            for (int sub = 0; sub < 2 && cur[i] < end; ++sub) {
              int pick = cur[i];
              for (int j = cur[i]; j < end; ++j)
                if (!(used >> (p_cam[j] & 15) & 1u)) { pick = j; break; }
              used |= 1u << (p_cam[pick] & 15);
              std::swap(p_cam[pick], p_cam[cur[i]]);
              std::swap(p_src[pick], p_src[cur[i]]);
              ++cur[i];
            }
          }
        }
      }
    }
  }
}

// Camera order: stable counting sort of the POINT-ordered list by camera, so that every camera's observations are
// ascending in point index (needed by the partition split)
static void host_sort_by_camera(int Nc, int Np, int No, const int32_t* cam_idx, const std::vector<int>& pt_off,
                                const std::vector<int>& p_cam, const std::vector<int>& p_src, std::vector<int>& cam_off,
                                std::vector<int>& c_pt, std::vector<int>& c_orig) {
  cam_off.assign(Nc + 1, 0);
  for (int i = 0; i < No; ++i) cam_off[cam_idx[i] + 1]++;
  for (int c = 0; c < Nc; ++c) cam_off[c + 1] += cam_off[c];
  c_pt.resize(No); c_orig.resize(No);
  std::vector<int> cc(cam_off.begin(), cam_off.end() - 1);
  for (int p = 0; p < Np; ++p)
    for (int j = pt_off[p]; j < pt_off[p + 1]; ++j) {
      const int a = cc[p_cam[j]]++;
      c_pt[a] = p; c_orig[a] = p_src[j];
    }
}

// Partition split: every camera's (point-sorted) list is cut into NPART equal-count chunks.  For uniformly spread
// observations chunk k covers about the k-th eighth of the point table (what keeps it resident in XCD k's L2); for
// band-structured data the chunks stay balanced and are narrow in point index anyway.
// Returns cam_band: which workgroup -> XCD assignment of the camera passes keeps an XCD on one slice of the point table
// (group_of_block), from the observations whose point lies in the slice of their partition, and in the slice of their
// camera's range.
static bool host_partitions(int Nc, int Np, const std::vector<int>& cam_off, const std::vector<int>& c_pt, std::vector<int>& offk) {
  offk.resize((size_t)Nc * (NPART + 1));
  for (int c = 0; c < Nc; ++c) {
    const long long n = cam_off[c + 1] - cam_off[c];
    for (int k = 0; k <= NPART; ++k) offk[(size_t)c * (NPART + 1) + k] = cam_off[c] + (int)((n * k) / NPART);
  }
  long long in_partition = 0, in_band = 0;
  if (Np > 0) {
    std::vector<unsigned char> slice_of(Np);           // p * NPART / Np without a division per observation
    for (int k = 0; k < NPART; ++k)
      for (long long q = ((long long)k * Np + NPART - 1) / NPART; q < ((long long)(k + 1) * Np + NPART - 1) / NPART; ++q)
        slice_of[q] = (unsigned char)k;
    for (int c = 0; c < Nc; ++c) {
      const int cam_slice = (int)(((long long)c * NPART) / Nc);
      for (int k = 0; k < NPART; ++k)
        for (int a = offk[(size_t)c * (NPART + 1) + k]; a < offk[(size_t)c * (NPART + 1) + k + 1]; ++a) {
          const int pt_slice = slice_of[c_pt[a]];
          in_partition += pt_slice == k;
          in_band += pt_slice == cam_slice;
        }
    }
  }
  return in_band > in_partition;
}

// Band statistic: the summed camera span of the tracks and the number of tracks (sequential captures: a few cameras per
// track; random visibility: most of the range), for decide_banded
static void host_band_statistic(int Nc, int Np, const std::vector<int>& pt_off, const std::vector<int>& p_cam, double& span_sum,
                                double& tracks) {
  span_sum = tracks = 0.0;
  for (int p = 0; p < Np; ++p) {
    if (pt_off[p + 1] == pt_off[p]) continue;
    int lo = Nc, hi = -1;
    for (int j = pt_off[p]; j < pt_off[p + 1]; ++j) { lo = std::min(lo, p_cam[j]); hi = std::max(hi, p_cam[j]); }
    span_sum += hi - lo;
    tracks += 1.0;
  }
}

// The camera window (first camera, number of cameras) of every point-pass workgroup: the ranges, then the long-track
// workgroups.  A workgroup without observations gets (0, 0).
static std::vector<int2> host_windows(const ba_handle* h, int Nc, int Np, const std::vector<int>& pt_off, const std::vector<int>& p_cam,
                                      const std::vector<int>& long_pts) {
  std::vector<int2> win(h->nblkP + h->nblkL);
  auto window_of = [](int lo, int hi) { return hi < lo ? make_int2(0, 0) : make_int2(lo, hi - lo + 1); };
  for (int b = 0; b < h->nblkP; ++b) {
    const int p0 = std::min(Np, b * h->ppb), p1 = std::min(Np, (b + 1) * h->ppb);
    int lo = Nc, hi = -1;
    for (int j = pt_off[p0]; j < pt_off[p1]; ++j) { lo = std::min(lo, p_cam[j]); hi = std::max(hi, p_cam[j]); }
    win[b] = window_of(lo, hi);
  }
  for (int b = 0; b < h->nblkL; ++b) {
    int lo = Nc, hi = -1;
    for (int q = b * h->long_spb; q < std::min(h->n_long, (b + 1) * h->long_spb); ++q)
      for (int j = pt_off[long_pts[q]]; j < pt_off[long_pts[q] + 1]; ++j) { lo = std::min(lo, p_cam[j]); hi = std::max(hi, p_cam[j]); }
    win[h->nblkP + b] = window_of(lo, hi);
  }
  return win;
}

// The multi-workgroup window solver (ba_small_mw.hpp): eight cameras at most, up to 2048 landmarks in ranges of 64, no
// landmark seen twice by one camera; every camera's list is ascending in landmark index, so a range is a slice of it.
// No lower limit on landmarks (measured: no slower than k_small_lm even with one or two workgroups).  An empty plan when
// the problem is outside those limits.
static MwPlan host_window_solver_plan(ba_handle* h, int Nc, int Np, int No, const std::vector<int>& pt_off, const std::vector<int>& p_cam,
                                      const std::vector<int>& cam_off, const std::vector<int>& c_pt) {
  MwPlan plan;
  if (h->multi || Nc > MW_MAX_CAMS || Np > MW_MAX_WG * MW_PTS || No == 0) return plan;
  for (int p = 0; p < Np; ++p) {
    unsigned seen = 0;
    for (int j = pt_off[p]; j < pt_off[p + 1]; ++j) {
      if ((seen >> p_cam[j]) & 1u) return plan;
      seen |= 1u << p_cam[j];
    }
  }
  plan.G = (Np + MW_PTS - 1) / MW_PTS;
  plan.woff.assign((size_t)(plan.G + 1) * MW_MAX_CAMS, 0);
  for (int c = 0; c < MW_MAX_CAMS; ++c)
    for (int gq = 0; gq <= plan.G; ++gq) {
      int v = No;
      if (c < Nc) v = (int)(std::lower_bound(c_pt.begin() + cam_off[c], c_pt.begin() + cam_off[c + 1], gq * MW_PTS) - c_pt.begin());
      plan.woff[(size_t)gq * MW_MAX_CAMS + c] = v;
    }
  // the workgroups of k_small_mw meet at a counter barrier: the kernel is only chosen when the device can hold all of
  // them at once (occupancy query x compute units, once per handle; the launch itself is an ordinary one, and a barrier
  // that is not served in time -- somebody else holds the units -- ends in the fall-back of small_solve, not in a hang)
  const int nt = Nc <= 5 ? 0 : (Nc <= 7 ? 1 : 2);
  if (h->mw_resident[nt] < 0) {
    int per_cu = 0;
    hipError_t e = nt == 0 ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_small_mw<2>, MW_THREADS, 0)
                 : nt == 1 ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_small_mw<3>, MW_THREADS, 0)
                           : hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_small_mw<4>, MW_THREADS, 0);
    if (e != hipSuccess) { per_cu = 0; (void)hipGetLastError(); }
    h->mw_resident[nt] = per_cu * h->n_cu;
  }
  plan.ok = h->mw_resident[nt] >= plan.G;
  return plan;
}

// The host build's last step: device buffers, then the upload.  A window-sized problem (the reference's own use: a few
// thousand observations) would send a dozen small arrays, each a blocking staged transfer from pageable memory (~10 us);
// whenever the arena bound up_need allows, every array goes into ONE pinned arena instead -- one copy, and one
// k_unpack_problem deals the sections out and fills the pixel streams and flagged index copies -- and the call returns
// without waiting.  Larger problems (C3: 36 MB) copy every array directly and wait for the copies.
static int upload_host_layout(ba_handle* h, const HostLayout& L, const double* uv, StageClock& stage) {
  const int Nc = h->Nc, Np = h->Np, No = h->Nobs;
  const size_t up_need = (size_t)No * (4 * 4 + 16) + (size_t)Np * 12 + (size_t)Nc * 40 + L.win.size() * 8 + 4096;
  const bool staged = up_need <= ((size_t)4 << 20);
  h->up.wait();                // the arena's last upload has landed
  HIPCHECK(h->offk.alloc(L.offk.size())); HIPCHECK(h->pt_off.alloc(Np + 1)); HIPCHECK(h->slot.alloc(std::max(Np, 1)));
  HIPCHECK(h->blk_win.alloc(L.win.size())); HIPCHECK(h->long_pts.alloc(std::max(h->n_long, 1)));
  if (!L.mw.woff.empty()) {
    HIPCHECK(h->mw_woff.alloc(L.mw.woff.size()));
    HIPCHECK(h->mw_buf.alloc((size_t)2 * MW_MAX_WG * (MW_MSG + MW_SCAL) + 8));
  }
  if (int rc = alloc_solver_buffers(h)) return rc;
  // every array, in arena order; the observation streams c_pt, c_orig, p_cam come last
  struct Section { void* dst; const void* src; size_t bytes; };
  const size_t ob = (size_t)No * sizeof(int);
  const Section sec[] = {{h->slot.p, L.slot.data(), (size_t)Np * sizeof(int)},       {h->blk_win.p, L.win.data(), L.win.size() * sizeof(int2)},
                         {h->long_pts.p, L.long_pts.data(), L.long_pts.size() * sizeof(int)}, {h->mw_woff.p, L.mw.woff.data(), L.mw.woff.size() * sizeof(int)},
                         {h->offk.p, L.offk.data(), L.offk.size() * sizeof(int)},    {h->pt_off.p, L.pt_off.data(), L.pt_off.size() * sizeof(int)},
                         {h->c_pt.p, L.c_pt.data(), ob}, {h->c_orig.p, L.c_orig.data(), ob}, {h->p_cam.p, L.p_cam.data(), ob}};
  static_assert(sizeof sec / sizeof sec[0] <= UNPACK_MAX_SECTIONS, "k_unpack_problem's section table");
  auto padded = [](size_t bytes) { return (bytes + 63) & ~(size_t)63; };   // sections start 64-byte aligned
  size_t arena = No > 0 ? padded(2 * (size_t)No * sizeof(double)) + padded(ob) : 0;   // (+ the pixels and p_src)
  for (const Section& x : sec) arena += padded(x.bytes);
  if (staged) {
    assert(arena <= up_need);
    HIPCHECK(h->up.reserve(up_need, std::min<size_t>((size_t)4 << 20, std::max<size_t>(2 * up_need, (size_t)256 << 10))));
    HIPCHECK(h->up_dev.alloc(arena));
  } else if (No > 0) {
    HIPCHECK(h->rbuf.alloc(2 * (size_t)No));
  }
  stage("allocations");
  if (staged) {
    UnpackArgs ua;
    memset(&ua, 0, sizeof ua);
    size_t used = 0;
    auto put = [&](const void* src, size_t bytes) { memcpy(h->up.p + used, src, bytes); used += padded(bytes); return used - padded(bytes); };
    for (const Section& x : sec) {
      if (x.bytes == 0) continue;
      ua.off[ua.n_sections] = put(x.src, x.bytes); ua.dst[ua.n_sections] = (int*)x.dst; ua.words[ua.n_sections] = (int)(x.bytes / 4);
      ++ua.n_sections;
    }
    if (No > 0) {              // the pixels (caller's order) and p_src are read from the arena only
      ua.n_obs = No;
      ua.off_uv = put(uv, 2 * (size_t)No * sizeof(double)); ua.off_psrc = put(L.p_src.data(), ob);
      ua.off_cpt = ua.off[ua.n_sections - 3]; ua.off_corig = ua.off[ua.n_sections - 2]; ua.off_pcam = ua.off[ua.n_sections - 1];
      ua.p_uv = h->p_uv.p; ua.c_uv = h->c_uv.p; ua.uv_f32 = h->uv_f32 ? 1 : 0;
      ua.c_ptf0 = h->c_ptf[0].p; ua.c_ptf1 = h->c_ptf[1].p; ua.p_camf0 = h->p_camf[0].p; ua.p_camf1 = h->p_camf[1].p;
    }
    HIPCHECK(hipMemcpyAsync(h->up_dev.p, h->up.p, used, hipMemcpyHostToDevice, h->stream));
    ua.arena = h->up_dev.p;
    BA_LAUNCH(k_unpack_problem, dim3((std::max(No, 4096) + 255) / 256), dim3(256), 0, h->stream, ua);
    // everything the device still reads sits in the pinned arena: no need to wait for the copy and the kernel -- whatever
    // comes next is ordered behind them on the stream; the arena's next use waits for this mark first
    HIPCHECK(h->up.mark(h->stream));
    if (int rc = check_launches(h)) return rc;
  } else {
    for (const Section& x : sec)
      if (x.bytes) HIPCHECK(hipMemcpyAsync(x.dst, x.src, x.bytes, hipMemcpyHostToDevice, h->stream));
    if (No > 0) {
      // pixels: uploaded once in the caller's order, permuted into both orderings on the device (staging: the residual
      // buffer for the pixels, a flagged-index buffer for the point-order permutation)
      HIPCHECK(hipMemcpyAsync(h->rbuf.p, uv, 2 * (size_t)No * sizeof(double), hipMemcpyHostToDevice, h->stream));
      HIPCHECK(hipMemcpyAsync(h->c_ptf[0].p, L.p_src.data(), ob, hipMemcpyHostToDevice, h->stream));
      const dim3 gg((No + 255) / 256), gb(256);
      BA_LAUNCH(k_gather_uv, gg, gb, 0, h->stream, (const double2*)h->rbuf.p, (const int*)h->c_ptf[0].p, No, h->p_uv.p, (int)h->uv_f32);
      BA_LAUNCH(k_gather_uv, gg, gb, 0, h->stream, (const double2*)h->rbuf.p, (const int*)h->c_orig.p, No, h->c_uv.p, (int)h->uv_f32);
      // the flagged copies of the index streams start as the plain streams: a robust linearisation reads them and stores
      // an entry only where its "weights are not (1, 1)" flag changes
      BA_LAUNCH(k_init_flagged, gg, gb, 0, h->stream, (const int*)h->c_pt.p, (const int*)h->p_cam.p, No, h->c_ptf[0].p, h->c_ptf[1].p,
                h->p_camf[0].p, h->p_camf[1].p);
    }
    BA_SYNC(h);                // the host vectors go out of scope
  }
  stage("upload");
  return BA_OK;
}

static int set_problem_host(ba_handle* h, int Nc, int Np, int No, const int32_t* cam_idx, const int32_t* pt_idx, const double* uv,
                            const double K4[4], int fixed_cam, StageClock& stage) {
  // float2 pixel streams (UvArr): only problems the window solvers never take (they read double2), and only when every
  // pixel is a float32 value (branch-free sweep; NaN compares unequal: stays double)
  bool uv_f32 = false;
  if (uv_f32_wanted() && Nc > SMALL_MAX_CAMS && No > 0) {
    int all = 1;
    for (int64_t i = 0; i < 2 * (int64_t)No; ++i) all &= (int)pixel_is_f32(uv[i]);
    uv_f32 = all != 0;
    stage("pixel value sweep");
  }
  HostLayout L;
  L.slot = host_point_numbering(Nc, Np, No, cam_idx, pt_idx);
  std::vector<int> pt(No);
  for (int i = 0; i < No; ++i) pt[i] = L.slot[pt_idx[i]];
  stage("point numbering");
  const PtGrid grid = config_point_grid(h, Nc, Np, No);
  host_sort_by_point(Np, No, cam_idx, pt, L.pt_off, L.p_cam, L.p_src);
  L.long_pts = host_long_tracks(h, grid, Np, L.pt_off);
  if (h->lanes == LPP && grid.table_fits) bank_aware_order(h, Np, L.pt_off, L.p_cam, L.p_src);
  stage("sort by point");
  host_sort_by_camera(Nc, Np, No, cam_idx, L.pt_off, L.p_cam, L.p_src, L.cam_off, L.c_pt, L.c_orig);
  stage("sort by camera");
  const bool cam_band = host_partitions(Nc, Np, L.cam_off, L.c_pt, L.offk);
  stage("partitions + XCD statistic");
  if (!h->banded_known) {      // (decided already by a device build that handed the problem back)
    double span_sum, tracks;
    host_band_statistic(Nc, Np, L.pt_off, L.p_cam, span_sum, tracks);
    if (int rc = decide_banded(h, span_sum, tracks, Nc)) return rc;
  }
  stage("band statistic");
  L.win = host_windows(h, Nc, Np, L.pt_off, L.p_cam, L.long_pts);
  stage("long tracks + windows");
  L.mw = host_window_solver_plan(h, Nc, Np, No, L.pt_off, L.p_cam, L.cam_off, L.c_pt);
  set_dimensions(h, Nc, Np, No, K4, fixed_cam);
  set_window_lds(h, L.win.data(), L.win.size());
  h->cam_band = cam_band; h->uv_f32 = uv_f32;
  h->mw_ok = L.mw.ok; h->mw_G = L.mw.G;
  if (stage.on)
    fprintf(stderr, "ba_set_problem point passes: %d lanes/point, %d range workgroups x %d points + %d long-track workgroups x %d points "
            "(%d points over %d observations), LDS window %zu / %zu bytes, every window in LDS %d / %d\n", h->lanes, h->nblkP, h->ppb,
            h->nblkL, h->long_spb, h->n_long, h->long_thr, h->lds_bytes_m[0], h->lds_bytes_m[1], (int)h->all_lds_m[0], (int)h->all_lds_m[1]);
  return upload_host_layout(h, L, uv, stage);
}

static void clear_priors(ba_handle* h) {
  h->any_cam_prior = h->any_pt_prior = false;
  h->prior_nb = 0;
  h->prior_blocks = 0;
}
static void clear_shared(ba_handle* h) {
  h->n_shared = h->n_shared_chunks = 0;
  h->shared_on = false;
  h->h_cam_gl.clear(); h->h_grp_off.clear(); h->h_grp_mem.clear(); h->h_chunk_rng.clear(); h->h_grp_chunk.clear();
}
static void clear_held(ba_handle* h) {
  h->any_cam_held = h->any_pt_held = false;
  h->cam_held_or = 0;
  h->h_cam_held.clear();
  h->h_pt_held.clear();
  h->held_x2 = 0.0;
}
// sum of the held points' |X|^2 (caller's point order), summed in point order
static double held_points_x2(const ba_handle* h, const double* pts) {
  double s = 0.0;
  if (!h->any_pt_held) return s;
  for (int p = 0; p < h->Np; ++p)
    if (h->h_pt_held[p]) s += pts[3 * (size_t)p] * pts[3 * (size_t)p] + pts[3 * (size_t)p + 1] * pts[3 * (size_t)p + 1] +
                              pts[3 * (size_t)p + 2] * pts[3 * (size_t)p + 2];
  return s;
}
extern "C" int ba_set_problem(ba_handle* h, int32_t n_cams, int32_t n_pts, int64_t n_obs, const int32_t* cam_idx,
                              const int32_t* pt_idx, const double* uv, const double K4[4], int32_t fixed_cam) {
  StageClock stage;            // (host sorts are the bulk of this call at C3)
  if (!h) return fail(BA_ERR_INVALID, "null handle");
  if (n_cams <= 0 || n_pts < 0 || n_obs < 0 || n_obs > 0x7fffffffLL) return fail(BA_ERR_INVALID, "bad sizes");
  if (n_obs > 0 && (!cam_idx || !pt_idx || !uv)) return fail(BA_ERR_INVALID, "null observation arrays");
  if (!K4) return fail(BA_ERR_INVALID, "null intrinsics");
  if (fixed_cam < -1 || fixed_cam >= n_cams) return fail(BA_ERR_INVALID, "fixed_cam %d out of range", fixed_cam);
  clear_held(h);                     // a new problem starts with nothing held beyond its fixed camera
  clear_priors(h);                   // ... and without priors
  clear_shared(h);                   // ... and every camera with its own intrinsics
  h->trk_valid = false;
  h->rs.valid = false;
  h->rn.valid = false;
  {   // index ranges, before anything is touched (a rejected call keeps the previous problem): branch-free sweep first
    int ok = 1;
    for (int64_t i = 0; i < n_obs; ++i)
      ok &= (int)((unsigned)cam_idx[i] < (unsigned)n_cams) & (int)((unsigned)pt_idx[i] < (unsigned)n_pts);
    if (!ok)
      for (int64_t i = 0; i < n_obs; ++i) {
        if (cam_idx[i] < 0 || cam_idx[i] >= n_cams) return fail(BA_ERR_INVALID, "cam_idx[%lld]=%d out of range", (long long)i, cam_idx[i]);
        if (pt_idx[i] < 0 || pt_idx[i] >= n_pts) return fail(BA_ERR_INVALID, "pt_idx[%lld]=%d out of range", (long long)i, pt_idx[i]);
      }
  }
  if ((n_cams + VEC_CAMS - 1) / VEC_CAMS > 16384) return fail(BA_ERR_INVALID, "more than %d cameras are not supported", 16384 * VEC_CAMS);
  stage("validate");
  if (set_device(h)) return BA_ERR_HIP;
  // From here on the previous problem is gone: should anything below fail (allocation, copy), the handle is left
  // WITHOUT a problem rather than with new sizes over old buffers.
  h->have_problem = h->have_params = h->linearized = false;
  h->setup_path = 0;
  h->banded_known = false;
  h->uv_f32 = false;
  // the window solver keeps V = W L resident and only ever writes the columns of points that exist: a new problem on
  // the same handle (fewer landmarks inside the same 16-column padding, or other cameras per point) must not inherit
  // columns of the previous one -> V is cleared again before its next use
  h->small_np_pad = -1;
  // Large problems whose camera table fits in LDS are laid out ON THE DEVICE (set_problem_device, ba_setup.hpp: one upload
  // of the caller's arrays, no host sorts; bit-equal result) from SETUP_DEVICE_MIN_OBS observations on (the measured
  // crossover is near 40 000 -- 0.23 against 0.27 ms at 48 k, 0.40 against 1.05 ms at 160 k).  BA_SETUP=host / device
  // forces a path (device: whenever the problem qualifies at all).
  const char* mode = getenv("BA_SETUP");
  bool try_dev = n_obs > 0 && n_pts > 0 && n_cams > MW_MAX_CAMS && (size_t)n_cams * TA * sizeof(double) <= (size_t)LDS_TAB_BYTES;
  if (mode && strcmp(mode, "host") == 0) try_dev = false;
  else if (!(mode && strcmp(mode, "device") == 0) && n_obs < SETUP_DEVICE_MIN_OBS) try_dev = false;
  int rc = 1;
  if (try_dev) {
    rc = set_problem_device(h, n_cams, n_pts, (int)n_obs, cam_idx, pt_idx, uv, K4, fixed_cam);
    if (rc < 0) { const std::string msg = g_err; (void)hipStreamSynchronize(h->stream); h->launch_err = hipSuccess; g_err = msg; return rc; }
    if (rc == BA_OK) {
      stage("device build (total)");
    } else {                   // rc == 1: this problem is for the host build
      (void)hipStreamSynchronize(h->stream);
      h->launch_err = hipSuccess;
    }
  }
  if (rc != BA_OK)
    if ((rc = set_problem_host(h, n_cams, n_pts, (int)n_obs, cam_idx, pt_idx, uv, K4, fixed_cam, stage))) return rc;
  h->have_problem = true;
  return BA_OK;
}

// block sizes of the running camera model
static int nb_of(const ba_handle* h) { return kModel[h->model].nb; }
// partitions a consumer of the camera passes' partial sums adds up: all of them on one rank; in a multi-rank job the
// arrays arrive folded into partition 0 and all-reduced (fold_and_reduce), the other partitions are stale
static int nparts_of(const ba_handle* h) { return h->multi ? 1 : NPART; }
// the camera half's running sums a consumer reads: all partitions on one rank; the folded, all-reduced message otherwise
static const double* partL_of(const ba_handle* h, int buf) { return h->multi ? h->linmsg[buf].p + 8 : h->partL[buf].p; }
static int nbv(const ba_handle* h) { return h->nblkVm[h->model]; }      // camera-vector workgroups of the active model
static int nh_of(const ba_handle* h) { return kModel[h->model].nh; }
static int nl_of(const ba_handle* h) { return kModel[h->model].nl; }
static size_t lds_of(const ba_handle* h) { return h->lds_bytes_m[h->model]; }
static bool all_lds_of(const ba_handle* h) { return h->all_lds_m[h->model]; }
static double* bc_ptr(ba_handle* h) { return h->HccBc.p + nh_of(h) * (size_t)h->Nc; }
static int cam_grid(ba_handle* h, int segl = 64) { const int cpb = 64 * WPB / segl; return ((h->Nc + cpb - 1) / cpb) * NPART; }
static int row_grid(ba_handle* h) { return ((h->Nc + ROWS - 1) / ROWS) * NPART; }

// pinned bounce buffer for parameter transfers of at most 1 MB (grow-only); false: copy from / to the caller's memory
static bool par_bounce(ba_handle* h, size_t bytes) {
  if (bytes == 0 || bytes > ((size_t)1 << 20)) return false;
  if (h->par.reserve(bytes, std::max<size_t>(2 * bytes, (size_t)64 << 10), h->stream) != hipSuccess) { (void)hipGetLastError(); return false; }
  return true;
}
extern "C" int ba_set_params(ba_handle* h, const double* cams, const double* pts) {
  if (!h || !cams || (!pts && h->Np > 0)) return fail(BA_ERR_INVALID, "null argument");
  if (!h->have_problem) return fail(BA_ERR_STATE, "ba_set_problem has not been called");
  if (set_device(h)) return BA_ERR_HIP;
  h->cur = 0;
  // a window's worth of parameters goes through a pinned bounce buffer: copies from pageable memory are staged by the
  // runtime one blocking transfer at a time (~10 us each), more than the kernels behind them take
  const size_t cb = 6 * (size_t)h->Nc * sizeof(double), pb = 3 * (size_t)h->Np * sizeof(double);
  const double *cams_src = cams, *pts_src = pts;
  if (par_bounce(h, cb + pb)) {
    memcpy(h->par.p, cams, cb);
    if (pb) memcpy(h->par.p + cb, pts, pb);
    cams_src = (const double*)h->par.p; pts_src = (const double*)(h->par.p + cb);
  }
  h->held_x2 = held_points_x2(h, pts);
  HIPCHECK(hipMemcpyAsync(h->cams[0].p, cams_src, cb, hipMemcpyHostToDevice, h->stream));
  if (h->Np > 0) {
    HIPCHECK(hipMemcpyAsync(h->stage.p, pts_src, pb, hipMemcpyHostToDevice, h->stream));
    BA_LAUNCH(k_pack_points, dim3((h->Np + 255) / 256), dim3(256), 0, h->stream, h->stage.p, h->slot.p, h->Np, h->ptab[0].p);
  }
  BA_LAUNCH(k_cam_prepare<Pinhole>, dim3((h->Nc + 63) / 64), dim3(64), 0, h->stream, h->cams[0].p, (const double*)h->intr[0].p,
            h->cs[0].p, h->camA[0].p, h->Nc);
  if (cams_src != cams) {
    // the caller's arrays are no longer referenced: no need to wait for the two kernels (whatever comes next is ordered
    // behind them on the stream; a launch failure surfaces at the next synchronisation)
    HIPCHECK(h->par.mark(h->stream));
    if (int rc = check_launches(h)) return rc;
  } else {
    BA_SYNC(h);
  }
  h->have_params = true;
  h->linearized = false;
  return BA_OK;
}

extern "C" int ba_get_params(ba_handle* h, double* cams, double* pts) {
  if (!h) return fail(BA_ERR_INVALID, "null handle");
  if (!h->have_params) return fail(BA_ERR_STATE, "no parameters set");
  if (set_device(h)) return BA_ERR_HIP;
  const size_t cb = cams ? 6 * (size_t)h->Nc * sizeof(double) : 0, pb = (pts && h->Np > 0) ? 3 * (size_t)h->Np * sizeof(double) : 0;
  const bool bounce = par_bounce(h, cb + pb);
  if (cams) HIPCHECK(hipMemcpyAsync(bounce ? (void*)h->par.p : (void*)cams, h->cams[h->cur].p, cb, hipMemcpyDeviceToHost, h->stream));
  if (pts && h->Np > 0) {
    BA_LAUNCH(k_unpack_points, dim3((h->Np + 255) / 256), dim3(256), 0, h->stream, h->ptab[h->cur].p, h->slot.p, h->Np, h->stage.p);
    HIPCHECK(hipMemcpyAsync(bounce ? (void*)(h->par.p + cb) : (void*)pts, h->stage.p, pb, hipMemcpyDeviceToHost, h->stream));
  }
  BA_SYNC(h);
  if (bounce) {
    if (cb) memcpy(cams, h->par.p, cb);
    if (pb) memcpy(pts, h->par.p + cb, pb);
  }
  return BA_OK;
}

// Held parameters: validated, kept on the host (caller's orders) and uploaded in the problem's orders (point flags through
// the point -> slot permutation of ba_set_problem).  NULL / all-zero arrays hold nothing.
extern "C" int ba_set_held(ba_handle* h, const uint16_t* cam_held, const uint8_t* pt_held) {
  if (!h) return fail(BA_ERR_INVALID, "null handle");
  if (!h->have_problem) return fail(BA_ERR_STATE, "ba_set_problem has not been called");
  unsigned bits = 0;
  bool any_c = false, any_p = false;
  if (cam_held)
    for (int c = 0; c < h->Nc; ++c) { bits |= cam_held[c]; any_c |= cam_held[c] != 0; }
  if (bits & ~0x1ffu) return fail(BA_ERR_INVALID, "camera mask bits beyond bit 8 (the 9-parameter BAL block)");
  if (pt_held)
    for (int p = 0; p < h->Np; ++p) any_p |= pt_held[p] != 0;
  if (set_device(h)) return BA_ERR_HIP;
  clear_held(h);
  if (any_c) {
    h->h_cam_held.assign(cam_held, cam_held + h->Nc);
    HIPCHECK(h->cam_held.alloc((size_t)h->Nc));
    HIPCHECK(hipMemcpyAsync(h->cam_held.p, h->h_cam_held.data(), (size_t)h->Nc * sizeof(unsigned short), hipMemcpyHostToDevice, h->stream));
    h->cam_held_or = bits;
    h->any_cam_held = true;
  }
  if (any_p) {
    h->h_pt_held.resize((size_t)h->Np);
    for (int p = 0; p < h->Np; ++p) h->h_pt_held[p] = pt_held[p] ? 1 : 0;
    HIPCHECK(h->pt_held.alloc((size_t)h->Np));
    HIPCHECK(h->pt_held_in.alloc((size_t)h->Np));
    HIPCHECK(hipMemcpyAsync(h->pt_held_in.p, h->h_pt_held.data(), (size_t)h->Np, hipMemcpyHostToDevice, h->stream));
    BA_LAUNCH(k_scatter_flags, dim3((h->Np + 255) / 256), dim3(256), 0, h->stream, (const unsigned char*)h->pt_held_in.p, h->slot.p,
              h->Np, h->pt_held.p);
    h->any_pt_held = true;
  }
  BA_SYNC(h);
  if (any_p && h->have_params) {                 // the held share of |x| at the current points
    std::vector<double> pts(3 * (size_t)h->Np);
    if (int rc = ba_get_params(h, nullptr, pts.data())) { clear_held(h); return rc; }
    h->held_x2 = held_points_x2(h, pts.data());
  }
  h->linearized = false;
  return BA_OK;
}

// Shared intrinsics: labels -> groups of two or more members (a group of one is an ungrouped camera), numbered by their
// lowest member; the member lists are built here once and uploaded.
extern "C" int ba_set_shared_intrinsics(ba_handle* h, const int32_t* cam_group) {
  if (!h) return fail(BA_ERR_INVALID, "null handle");
  if (!h->have_problem) return fail(BA_ERR_STATE, "ba_set_problem has not been called");
  const int Nc = h->Nc;
  if (cam_group)
    for (int c = 0; c < Nc; ++c)
      if (cam_group[c] < -1) return fail(BA_ERR_INVALID, "ba_set_shared_intrinsics: camera %d: label %d (labels are -1 or non-negative)", c, cam_group[c]);
  clear_shared(h);
  h->linearized = false;
  if (!cam_group) return BA_OK;
  std::vector<std::pair<int32_t, int>> by_label;          // (label, camera), sorted: members ascending within a label
  for (int c = 0; c < Nc; ++c) if (cam_group[c] >= 0) by_label.emplace_back(cam_group[c], c);
  std::sort(by_label.begin(), by_label.end());
  std::vector<std::pair<int, int>> runs;                  // (leader, first index in by_label) of labels with >= 2 members
  for (size_t i = 0; i < by_label.size();) {
    size_t j = i;
    while (j < by_label.size() && by_label[j].first == by_label[i].first) ++j;
    if (j - i >= 2) runs.emplace_back(by_label[i].second, (int)i);
    i = j;
  }
  if (runs.empty()) return BA_OK;
  std::sort(runs.begin(), runs.end());                    // groups in the order of their leaders
  h->h_cam_gl.assign((size_t)Nc, -1);
  h->h_grp_off.assign(1, 0);
  for (size_t g = 0; g < runs.size(); ++g) {
    const int32_t label = by_label[(size_t)runs[g].second].first;
    for (size_t i = (size_t)runs[g].second; i < by_label.size() && by_label[i].first == label; ++i) {
      const int c = by_label[i].second;
      h->h_cam_gl[(size_t)c] = 2 * (int)g + (c == runs[g].first ? 1 : 0);
      h->h_grp_mem.push_back(c);
    }
    h->h_grp_off.push_back((int)h->h_grp_mem.size());
  }
  const int G = (int)runs.size();
  h->h_grp_chunk.assign(1, 0);
  for (int g = 0; g < G; ++g) {
    for (int b = h->h_grp_off[g]; b < h->h_grp_off[g + 1]; b += SHARED_BLOCK) {
      h->h_chunk_rng.push_back(b);
      h->h_chunk_rng.push_back(std::min(b + SHARED_BLOCK, h->h_grp_off[g + 1]));
    }
    h->h_grp_chunk.push_back((int)(h->h_chunk_rng.size() / 2));
  }
  const int n_chunks = h->h_grp_chunk.back();
  if (set_device(h)) { clear_shared(h); return BA_ERR_HIP; }
  auto up = [&](DBuf<int>& d, const std::vector<int>& v) -> hipError_t {
    hipError_t e = d.alloc(v.size());
    return e != hipSuccess ? e : hipMemcpyAsync(d.p, v.data(), v.size() * sizeof(int), hipMemcpyHostToDevice, h->stream);
  };
  hipError_t e = up(h->cam_gl, h->h_cam_gl);
  if (e == hipSuccess) e = up(h->grp_off, h->h_grp_off);
  if (e == hipSuccess) e = up(h->grp_mem, h->h_grp_mem);
  if (e == hipSuccess) e = up(h->chunk_rng, h->h_chunk_rng);
  if (e == hipSuccess) e = up(h->grp_chunk, h->h_grp_chunk);
  if (e == hipSuccess) e = h->grp_rec.alloc((size_t)SHARED_REC * G);
  if (e == hipSuccess) e = h->grp_w.alloc(3 * (size_t)n_chunks);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) { clear_shared(h); return fail(BA_ERR_HIP, "ba_set_shared_intrinsics: %s", hipGetErrorString(e)); }
  h->n_shared = G;
  h->n_shared_chunks = n_chunks;
  return BA_OK;
}
static const int* cam_gl_ptr(const ba_handle* h) { return h->shared_on ? h->cam_gl.p : nullptr; }

// ------------------------------------------------------------------------------------------------------ priors
// eigenvalues of a packed symmetric n x n block (n <= 9) by cyclic Jacobi rotations: smallest and largest
static void sym_eig_range(const double* packed, int n, double* lo, double* hi) {
  double A[9][9];
  for (int i = 0; i < n; ++i) for (int j = 0; j < n; ++j) A[i][j] = packed[ST(n, i, j)];
  for (int sweep = 0; sweep < 64; ++sweep) {
    double off = 0.0, diag = 0.0;
    for (int i = 0; i < n; ++i) { diag += A[i][i] * A[i][i]; for (int j = i + 1; j < n; ++j) off += A[i][j] * A[i][j]; }
    if (off <= 1e-60 || off <= 1e-34 * diag) break;
    for (int p = 0; p < n; ++p)
      for (int q = p + 1; q < n; ++q) {
        if (A[p][q] == 0.0) continue;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), sn = t * c;
        for (int k = 0; k < n; ++k) { const double akp = A[k][p], akq = A[k][q]; A[k][p] = c * akp - sn * akq; A[k][q] = sn * akp + c * akq; }
        for (int k = 0; k < n; ++k) { const double apk = A[p][k], aqk = A[q][k]; A[p][k] = c * apk - sn * aqk; A[q][k] = sn * apk + c * aqk; }
      }
  }
  *lo = *hi = A[0][0];
  for (int i = 1; i < n; ++i) { *lo = std::min(*lo, A[i][i]); *hi = std::max(*hi, A[i][i]); }
}
// one block of a prior: 0 = zero block (no prior), 1 = fine, < 0 = refused (the message is set)
static int check_prior_block(const char* what, int idx, const double* info, const double* mean, int n) {
  const int nh = n * (n + 1) / 2;
  bool any = false;
  for (int q = 0; q < nh; ++q) {
    if (!std::isfinite(info[q])) return fail(BA_ERR_INVALID, "ba_set_priors: %s %d: non-finite entry in the information block", what, idx);
    any |= info[q] != 0.0;
  }
  if (!any) return 0;
  for (int q = 0; q < n; ++q)
    if (!std::isfinite(mean[q])) return fail(BA_ERR_INVALID, "ba_set_priors: %s %d: non-finite mean under a non-zero information block", what, idx);
  double lo, hi;
  sym_eig_range(info, n, &lo, &hi);
  if (lo < -1e-12 * hi || !(hi > 0.0))
    return fail(BA_ERR_INVALID, "ba_set_priors: %s %d: the information block is not positive semidefinite (eigenvalues %g .. %g)", what, idx, lo, hi);
  return 1;
}
// Gaussian priors: validated on the host (caller's orders), uploaded in the problem's orders (point blocks through the
// point -> slot permutation of ba_set_problem).  NULL pairs / all-zero blocks set nothing.
extern "C" int ba_set_priors(ba_handle* h, int32_t nb, const double* cam_mean, const double* cam_info, const double* pt_mean,
                             const double* pt_info) {
  if (!h) return fail(BA_ERR_INVALID, "null handle");
  if (!h->have_problem) return fail(BA_ERR_STATE, "ba_set_problem has not been called");
  if ((cam_mean == nullptr) != (cam_info == nullptr) || (pt_mean == nullptr) != (pt_info == nullptr))
    return fail(BA_ERR_INVALID, "ba_set_priors: a mean and its information array come together (both or neither NULL)");
  if (cam_info && nb != 6 && nb != 9) return fail(BA_ERR_INVALID, "ba_set_priors: nb must be 6 (rvec | t) or 9 (rvec | t | f k1 k2), not %d", nb);
  const int Nc = h->Nc, Np = h->Np;
  const int nh = nb * (nb + 1) / 2;
  long long nc_blocks = 0, np_blocks = 0;
  std::vector<double> cm, pm;
  if (cam_info) {
    cm.assign(cam_mean, cam_mean + (size_t)nb * Nc);
    for (int c = 0; c < Nc; ++c) {
      const int k = check_prior_block("camera", c, cam_info + (size_t)nh * c, cam_mean + (size_t)nb * c, nb);
      if (k < 0) return k;
      if (k) ++nc_blocks;
      else for (int q = 0; q < nb; ++q) cm[(size_t)nb * c + q] = 0.0;
    }
  }
  if (pt_info) {
    pm.assign(pt_mean, pt_mean + 3 * (size_t)Np);
    for (int p = 0; p < Np; ++p) {
      const int k = check_prior_block("point", p, pt_info + 6 * (size_t)p, pt_mean + 3 * (size_t)p, 3);
      if (k < 0) return k;
      if (k) ++np_blocks;
      else for (int q = 0; q < 3; ++q) pm[3 * (size_t)p + q] = 0.0;
    }
  }
  if (set_device(h)) return BA_ERR_HIP;
  clear_priors(h);
  h->linearized = false;
  if (nc_blocks) {
    HIPCHECK(h->cam_info.alloc((size_t)nh * Nc)); HIPCHECK(h->cam_mean.alloc((size_t)nb * Nc));
    HIPCHECK(hipMemcpyAsync(h->cam_info.p, cam_info, (size_t)nh * Nc * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipMemcpyAsync(h->cam_mean.p, cm.data(), (size_t)nb * Nc * sizeof(double), hipMemcpyHostToDevice, h->stream));
  }
  if (np_blocks) {
    HIPCHECK(h->pt_info.alloc(6 * (size_t)Np)); HIPCHECK(h->pt_mean.alloc(3 * (size_t)Np)); HIPCHECK(h->prior_in.alloc(9 * (size_t)Np));
    HIPCHECK(hipMemcpyAsync(h->prior_in.p, pt_info, 6 * (size_t)Np * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipMemcpyAsync(h->prior_in.p + 6 * (size_t)Np, pm.data(), 3 * (size_t)Np * sizeof(double), hipMemcpyHostToDevice, h->stream));
    BA_LAUNCH(k_scatter_rows, dim3((Np + 255) / 256), dim3(256), 0, h->stream, (const double*)h->prior_in.p, h->slot.p, Np, 6, h->pt_info.p);
    BA_LAUNCH(k_scatter_rows, dim3((Np + 255) / 256), dim3(256), 0, h->stream, (const double*)(h->prior_in.p + 6 * (size_t)Np), h->slot.p, Np, 3,
              h->pt_mean.p);
  }
  BA_SYNC(h);                       // (the host copies above go out of scope)
  h->any_cam_prior = nc_blocks > 0;
  h->any_pt_prior = np_blocks > 0;
  h->prior_nb = nc_blocks ? nb : 0;
  h->prior_blocks = nc_blocks + np_blocks;
  return BA_OK;
}
static bool any_prior(const ba_handle* h) { return h->any_cam_prior || h->any_pt_prior; }
// camera priors at parameter set `which` (info == null: none set, or `with_cams` false)
static CamPriors cam_priors(const ba_handle* h, int which, bool with_cams = true) {
  CamPriors pr;
  const bool on = with_cams && h->any_cam_prior;
  pr.info = on ? h->cam_info.p : nullptr; pr.mean = on ? h->cam_mean.p : nullptr;
  pr.cams = h->cams[which].p; pr.intr = h->intr[which].p; pr.nb = h->prior_nb;
  return pr;
}
// the prior rows behind partR at parameter set `which` (a solve with priors: the next scalar fold adds them to the cost);
// the camera sum counts once per job: rank 0's
static void launch_prior_cost(ba_handle* h, int which) {
  if (!h->fold_prior_rows) return;
  BA_LAUNCH(k_prior_cost, dim3(PRIOR_ROWS), dim3(256), 0, h->stream, cam_priors(h, which, h->rank == 0), h->Nc,
            h->any_pt_prior ? (const double*)h->pt_info.p : (const double*)nullptr, (const double*)h->pt_mean.p, (const double*)h->ptab[which].p,
            h->Np, h->partR.p + 2 * (size_t)NPART * h->Nc);
}
static const char* kSharedNeedsBal = "shared intrinsics (ba_set_shared_intrinsics) need the BAL camera model: clear them with a NULL argument";
static const char* kPriorNeedsBal = "camera priors with nb = 9 (f, k1, k2) need the BAL camera model";
extern "C" int ba_prior_cost(ba_handle* h, const double* intr, double* cam_cost, double* pt_cost) {
  if (!h) return fail(BA_ERR_INVALID, "null handle");
  if (!h->have_params) return fail(BA_ERR_STATE, "ba_set_problem / ba_set_params first");
  if (!intr && h->prior_nb == 9) return fail(BA_ERR_INVALID, "%s", kPriorNeedsBal);
  if (set_device(h)) return BA_ERR_HIP;
  double sums[2] = {0.0, 0.0};
  if (any_prior(h)) {
    if (intr) {
      HIPCHECK(h->tri.alloc(3 * (size_t)h->Nc + 8));
      HIPCHECK(hipMemcpyAsync(h->tri.p, intr, 3 * (size_t)h->Nc * sizeof(double), hipMemcpyHostToDevice, h->stream));
    }
    HIPCHECK(h->prior_rows.alloc(4 * PRIOR_ROWS));
    CamPriors pr = cam_priors(h, h->cur);
    pr.intr = intr ? h->tri.p : nullptr;
    CamPriors none = pr;
    none.info = nullptr;
    BA_LAUNCH(k_prior_cost, dim3(PRIOR_ROWS), dim3(256), 0, h->stream, pr, h->Nc, (const double*)nullptr, (const double*)nullptr,
              (const double*)h->ptab[h->cur].p, 0, h->prior_rows.p);
    BA_LAUNCH(k_prior_cost, dim3(PRIOR_ROWS), dim3(256), 0, h->stream, none, h->Nc,
              h->any_pt_prior ? (const double*)h->pt_info.p : (const double*)nullptr, (const double*)h->pt_mean.p, (const double*)h->ptab[h->cur].p,
              h->Np, h->prior_rows.p + 2 * PRIOR_ROWS);
    double rows[4 * PRIOR_ROWS];
    HIPCHECK(hipMemcpyAsync(rows, h->prior_rows.p, sizeof rows, hipMemcpyDeviceToHost, h->stream));
    BA_SYNC(h);
    for (int k = 0; k < 2; ++k)
      for (int b = 0; b < PRIOR_ROWS; ++b) sums[k] += rows[2 * (k * PRIOR_ROWS + b) + 1];
  }
  if (cam_cost) *cam_cost = 0.5 * sums[0];
  if (pt_cost) *pt_cost = 0.5 * sums[1];
  return BA_OK;
}

// multi-rank: every rank ends up with the points of all shards (its own at [p_begin, p_begin + Np)):
// zero-filled buffer + own slice, summed over the ranks with the solver's all-reduce
extern "C" int ba_allgather_points(ba_handle* h, int64_t p_begin, int64_t n_total, double* pts_all) {
  if (!h || !pts_all) return fail(BA_ERR_INVALID, "null argument");
  if (!h->have_params) return fail(BA_ERR_STATE, "no parameters set");
  if (p_begin < 0 || n_total < 0 || p_begin + (int64_t)h->Np > n_total)
    return fail(BA_ERR_INVALID, "shard [%lld, %lld) does not fit in %lld points", (long long)p_begin,
                (long long)(p_begin + h->Np), (long long)n_total);
  if (n_total == 0) return BA_OK;
  if (set_device(h)) return BA_ERR_HIP;
  HIPCHECK(h->gather.alloc(3 * (size_t)n_total));
  HIPCHECK(hipMemsetAsync(h->gather.p, 0, 3 * (size_t)n_total * sizeof(double), h->stream));
  if (h->Np > 0)
    BA_LAUNCH(k_unpack_points, dim3((h->Np + 255) / 256), dim3(256), 0, h->stream, h->ptab[h->cur].p, h->slot.p, h->Np,
                       h->gather.p + 3 * (size_t)p_begin);
  if (int rc = allreduce(h, h->gather.p, 3 * (size_t)n_total)) return rc;
  HIPCHECK(hipMemcpyAsync(pts_all, h->gather.p, 3 * (size_t)n_total * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  BA_SYNC(h);
  return BA_OK;
}

extern "C" int ba_get_rotations(ba_handle* h, double* R) {
  if (!h || !R) return fail(BA_ERR_INVALID, "null argument");
  if (!h->have_params) return fail(BA_ERR_STATE, "no parameters set");
  if (set_device(h)) return BA_ERR_HIP;
  HIPCHECK(hipMemcpy2DAsync(R, 9 * sizeof(double), h->cs[h->cur].p, CS * sizeof(double), 9 * sizeof(double), h->Nc,
                            hipMemcpyDeviceToHost, h->stream));
  BA_SYNC(h);
  return BA_OK;
}

// ---------------------------------------------------------------------- launch helpers
// Every helper dispatches on the camera model of the running call (BA_BY_MODEL(h->model, ..)): the same kernel
// templates, instantiated for the reference's pinhole and for the BAL camera (ba_models.hpp).
// intr: the BAL camera on the pinhole state with these device (f, k1, k2) (ba_residuals_bal stages them in h->tri
// without switching the model); null: the model of the running call with the intrinsics of parameter set `which`
static void launch_residual(ba_handle* h, int which, ba_loss loss, double fscale, double* r_out, const double* intr = nullptr) {
  Scope sc(h, BA_K_RESIDUAL);
  const bool robust = loss != BA_LOSS_LINEAR;
  if (h->model || intr) {                // (the two residual kernels predate the models and are no template of CM: no BA_BY_MODEL)
    auto kern = robust ? k_cam_residual_bal<true> : k_cam_residual_bal<false>;
    BA_LAUNCH(kern, dim3(cam_grid(h)), dim3(64 * WPB), 0, h->stream, h->cs[which].p, intr ? intr : (const double*)h->intr[which].p,
              h->ptab[which].p, h->offk.p, h->c_pt.p, uv_arr(h, h->c_uv), h->c_orig.p, fscale, (int)loss, h->Nc, h->cam_band, r_out, h->partR.p);
    return;
  }
  auto kern = robust ? k_cam_residual<true> : k_cam_residual<false>;
  BA_LAUNCH(kern, dim3(cam_grid(h)), dim3(64 * WPB), 0, h->stream, h->cs[which].p, h->ptab[which].p, h->offk.p,
                     h->c_pt.p, uv_arr(h, h->c_uv), h->c_orig.p, h->K4[0], h->K4[1], h->K4[2], h->K4[3], fscale, (int)loss, h->Nc, h->cam_band, r_out,
                     h->partR.p);
}
// fold the partial arrays of a step into `scal` (residual always; point / camera parts optional)
// with_step: also the step partials and the PCG verdict for iteration k; on a single rank the
// results go straight to the host-mapped mirror (no copy kernel)
// decide (single rank): the same kernel also computes the gain ratio and the next damping (lm_decide)
static ScalarsArgs scalars_args(ba_handle* h, bool with_step, int k, double tol2, int min_iters, long long seq, double cost_cur,
                                double lambda, double lam_floor = 0.0) {
  const bool direct = with_step && !h->multi;         // results straight into host-mapped memory + sequence word
  ScalarsArgs a;
  a.partR = h->partR.p; a.nR = NPART * h->Nc + h->fold_prior_rows;   // (+ the prior rows right behind: a solve with priors)
  a.partB = h->partB.p; a.nB = (with_step && h->Np > 0) ? h->nblkP + h->nblkL : 0;
  a.partC = h->partC.p; a.nC = with_step ? nbv(h) : 0;
  a.kit = k;
  a.st = with_step ? (const PcgState*)h->st.p : (const PcgState*)nullptr;
  a.partV = h->partV.p; a.nblkV = nbv(h);
  a.tol2 = tol2; a.min_iters = min_iters;
  a.scal = h->scal.p; a.scal_host = direct ? h->d_scal_host : (double*)nullptr;
  a.host_flag = direct ? h->d_flags + 2 : (long long*)nullptr; a.seq = seq;
  a.decide = direct ? 1 : 0; a.cost_cur = cost_cur; a.lambda = lambda; a.lam_floor = lam_floor;
  a.lam_slot = nullptr; a.err_flag = nullptr; a.on = 0;
  return a;
}
static void launch_scalars(ba_handle* h, bool with_step, int k = 0, double tol2 = 0.0, int min_iters = 0, long long seq = 0,
                           double cost_cur = 0.0, double lambda = 0.0, double lam_floor = 0.0) {
  Scope sc(h, BA_K_MISC);
  BA_LAUNCH(k_scalars, dim3(1), dim3(1024), 0, h->stream, scalars_args(h, with_step, k, tol2, min_iters, seq, cost_cur, lambda, lam_floor));
}
// spin on a host-mapped sequence word until it reaches `target` (the device publishes with a
// system-scope release); a wall-clock limit turns a wedged GPU into an error instead of a hang
static int wait_flag(ba_handle* h, int idx, long long target) {
  // a kernel the runtime refused to launch will never publish: say so instead of spinning into the time-out
  if (int rc = check_launches(h)) return rc;
  volatile long long* f = h->h_flags + idx;
  const auto t0 = std::chrono::steady_clock::now();
  double next_query = 2e-3;         // seconds of waiting before the stream is first asked for an error state
  unsigned spins = 0;
  while (*f < target) {
    if ((++spins & 0xfff) != 0) continue;
    const double waited = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (waited > next_query) {      // a faulted kernel puts the stream into a sticky error state: report that, not a time-out
      next_query = waited * 2;
      const hipError_t q = hipStreamQuery(h->stream);
      if (q != hipSuccess && q != hipErrorNotReady)
        return fail(BA_ERR_HIP, "the stream reports '%s' while waiting for flag %d", hipGetErrorString(q), idx);
      if (q == hipSuccess && *f < target)          // stream drained and the word was never written
        return fail(BA_ERR_HIP, "the stream drained without publishing flag %d (%lld < %lld)", idx, (long long)*f, target);
    }
    if (waited > 20.0)
      return fail(BA_ERR_HIP, "timed out waiting for the device (flag %d: %lld < %lld)", idx, (long long)*f, target);
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  return BA_OK;
}
static const unsigned short* cam_held_ptr(const ba_handle* h) { return h->any_cam_held ? h->cam_held.p : nullptr; }
static const unsigned char* pt_held_ptr(const ba_handle* h) { return h->any_pt_held ? h->pt_held.p : nullptr; }
// camera half of the linearisation at parameter set `which`, into buffer set `buf`
// cost: also the cost partials at that parameter set (partR) -- the pass then doubles as the trial-cost evaluation
template <class CM>
static void launch_lin_cam_t(ba_handle* h, int which, int buf, ba_loss loss, double fscale, bool cost) {
  const bool robust = loss != BA_LOSS_LINEAR;
  auto kern = robust ? (cost ? k_camrow_linearize<CM, true, true> : k_camrow_linearize<CM, true, false>)
                     : (cost ? k_camrow_linearize<CM, false, true> : k_camrow_linearize<CM, false, false>);
  BA_LAUNCH(kern, dim3(row_grid(h)), dim3(ROW_LANES * ROWS), 0, h->stream, h->cs[which].p, (const double*)h->intr[which].p,
                     h->ptab[which].p, h->offk.p, h->c_pt.p, uv_arr(h, h->c_uv), h->K4[0], h->K4[1], h->K4[2], h->K4[3], fscale, (int)loss,
                     h->Nc, h->cam_band, h->c_w[buf].p, h->c_ptf[buf].p, h->partL[buf].p, h->partR.p);
}
static void launch_lin_cam(ba_handle* h, int which, int buf, ba_loss loss, double fscale, bool cost = false) {
  Scope sc(h, BA_K_LINEARIZE_CAM);
  BA_BY_MODEL(h->model, launch_lin_cam_t<CM>(h, which, buf, loss, fscale, cost));
}
static void launch_lin_finalize(ba_handle* h) {
  Scope sc(h, BA_K_MISC);
  // (VEC_CAMS cameras per workgroup for either model: nblkVm[0])
  BA_BY_MODEL(h->model, BA_LAUNCH(k_lin_finalize<CM::NB>, dim3(h->nblkVm[0]), dim3(VEC_BLOCK), 0, h->stream, partL_of(h, h->lb), nparts_of(h),
                                  h->cs[h->cur].p, h->Nc, h->fixed, h->HccBc.p, bc_ptr(h), cam_held_ptr(h), cam_priors(h, h->cur)));
}
static PtWork pt_work(ba_handle* h) {        // every point; long tracks skipped when they have a launch of their own
  return PtWork{nullptr, h->Np, h->nblkL ? h->long_thr : 0x7fffffff, 0, h->ppb, /*xcd_ranges=*/1};
}
static PtWork pt_work_long(ba_handle* h) { return PtWork{h->long_pts.p, h->n_long, 0x7fffffff, h->nblkP, h->long_spb, 0}; }
// point half at parameter set `w` into point-buffer set `pbuf`, with the damped inverse / y0 at `lambda` fused in
// (lam_dev != null: the damping is read from that device word instead -- a speculated pass, see ba_solve)
template <class CM>
static void launch_lin_pt_t(ba_handle* h, int w, int pbuf, ba_loss loss, double fscale, double lambda, const double* lam_dev,
                            const ScalarsArgs& sa) {
  const bool robust = loss != BA_LOSS_LINEAR;
  const int ride = sa.on * NPART;                      // the step's scalar fold + verdict as workgroup 0 of this launch (+ NPART - 1 idle ones)
#define LP_HEAD h->camA[w].p, h->ptab[w].p, h->pt_off.p, h->p_cam.p, uv_arr(h, h->p_uv), h->blk_win.p
#define LP_TAIL h->K4[0], h->K4[1], h->K4[2], h->K4[3], fscale, (int)loss, lambda, lam_dev, h->Hpp[pbuf].p, h->bp[pbuf].p, h->p_w[pbuf].p,      \
                h->p_camf[pbuf].p, h->Hppinv[pbuf].p, h->y0[pbuf].p, h->partG[pbuf].p, sa
#define LP_LAUNCH(R, L, LN, G, WK) BA_LAUNCH((k_pt_linearize<CM, R, L, LN>), dim3((G) + ride), dim3(PT_THREADS), lds_of(h), h->stream, LP_HEAD, WK, LP_TAIL)
#define LP_BOTH(R, L) BA_LAUNCH((k_pt_linearize_both<CM, R, L>), dim3(h->nblkP + h->nblkL + ride), dim3(PT_THREADS), lds_of(h), h->stream, \
                                         LP_HEAD, wk, h->nblkP, wl, LP_TAIL)
  const PtWork wk = pt_work(h), wl = pt_work_long(h);
  if (h->nblkL) {          // short and long tracks in one launch
    if (all_lds_of(h)) { if (robust) LP_BOTH(true, true); else LP_BOTH(false, true); }
    else               { if (robust) LP_BOTH(true, false); else LP_BOTH(false, false); }
  } else {
#define LP_ONE(R, L)                                             \
  do {                                                           \
    switch (h->lanes) {                                          \
      case 4: LP_LAUNCH(R, L, 4, h->nblkP, wk); break;           \
      case 8: LP_LAUNCH(R, L, 8, h->nblkP, wk); break;           \
      case 16: LP_LAUNCH(R, L, 16, h->nblkP, wk); break;         \
      default: LP_LAUNCH(R, L, 2, h->nblkP, wk); break;          \
    }                                                            \
  } while (0)
    if (all_lds_of(h)) { if (robust) LP_ONE(true, true); else LP_ONE(false, true); }
    else               { if (robust) LP_ONE(true, false); else LP_ONE(false, false); }
#undef LP_ONE
  }
#undef LP_BOTH
#undef LP_LAUNCH
#undef LP_HEAD
#undef LP_TAIL
}
static void launch_lin_pt(ba_handle* h, int w, int pbuf, ba_loss loss, double fscale, double lambda, const double* lam_dev = nullptr,
                          const ScalarsArgs* rider = nullptr) {
  if (h->Np == 0) return;
  Scope sc(h, BA_K_LINEARIZE_PT);
  ScalarsArgs sa;
  if (rider) sa = *rider;
  else { memset(&sa, 0, sizeof sa); }
  BA_BY_MODEL(h->model, launch_lin_pt_t<CM>(h, w, pbuf, loss, fscale, lambda, lam_dev, sa));
  // point priors: L_p into Hpp | bp, the damped inverse, y0 and the gtol maxima redone (at the damping the pass used)
  if (h->any_pt_prior)
    BA_LAUNCH(k_prior_points, dim3(h->nblkP + h->nblkL), dim3(256), 0, h->stream, (const double*)h->pt_info.p, (const double*)h->pt_mean.p,
              h->Np, lambda, lam_dev, h->Hpp[pbuf].p, h->bp[pbuf].p, h->Hppinv[pbuf].p, h->y0[pbuf].p, h->ptab[w].p, h->partG[pbuf].p);
  // held points: their blocks and inverses zeroed, the gtol maxima redone without them (the point pass itself is not
  // told about held points: its observation loop and registers stay those of an unmasked solve)
  if (h->any_pt_held)
    BA_LAUNCH(k_held_points, dim3(h->nblkP + h->nblkL), dim3(256), 0, h->stream, (const unsigned char*)h->pt_held.p, h->Np,
              h->Hpp[pbuf].p, h->bp[pbuf].p, h->Hppinv[pbuf].p, h->y0[pbuf].p, h->ptab[w].p, h->partG[pbuf].p);
}
static void launch_point_invert(ba_handle* h, double lambda) {
  if (h->Np == 0) return;
  Scope sc(h, BA_K_POINT_INVERT);
  BA_LAUNCH(k_point_invert, dim3((h->Np + 255) / 256), dim3(256), 0, h->stream, h->Hpp[h->pb].p, h->bp[h->pb].p, lambda,
                     h->Np, h->Hppinv[h->pb].p, h->y0[h->pb].p, h->ptab[h->cur].p, pt_held_ptr(h));
}
// part6 buffer: [u.y word, pad | NPART x Nc x NB partial sums]; the u.y word sits in FRONT of partition 0 so that a
// multi-rank job all-reduces it together with the folded partition (one contiguous message)
constexpr int GMAX_HOST_SLOT = 40;   // word of the host-mapped scalar block that receives max |gradient| (k_scalars uses [0, S_COUNT))
static double* uy_ptr(ba_handle* h) { return h->part6.p; }
static double* p6_ptr(ba_handle* h) { return h->part6.p + 2; }
// (multi-rank: the damped system's sums are read from the all-reduced message of exchange_system)
static double* sys_p6(ba_handle* h) { return h->multi ? h->sysmsg.p + 2 : p6_ptr(h); }
static double* sys_E(ba_handle* h) { return h->multi ? h->sysmsg.p + 2 + nb_of(h) * (size_t)h->Nc : h->partE.p; }
static size_t sys_nE(ba_handle* h) { return h->sys_diag ? nh_of(h) * (size_t)h->Nc : 0; }
static const double* gmax_parts(ba_handle* h) {   // per-workgroup (single rank) / per-rank (multi-rank) maxima of |bp|
  return h->multi ? h->sysmsg.p + 2 + nb_of(h) * (size_t)h->Nc + sys_nE(h) : h->partG[h->pb].p;
}
static int gmax_count(ba_handle* h) { return h->multi ? h->world : (h->Np > 0 ? h->nblkP + h->nblkL : 0); }
// camera pass of the Schur product on the y slot of the current point table
//   diag: also the Schur-Jacobi blocks; pcg: iteration k with early exit
template <class CM>
static void launch_cam_schur_t(ba_handle* h, bool robust, bool diag, bool pcg, int k) {
  const int w = h->cur;
#define CS_ARGS h->cs[w].p, (const double*)h->intr[w].p, h->ptab[w].p, h->offk.p, (robust ? h->c_ptf[h->lb].p : h->c_pt.p), h->c_w[h->lb].p,  \
                h->K4[0], h->K4[1], h->Nc, h->cam_band, h->fixed,                                                                 \
                p6_ptr(h), k, (const double*)h->verdict.p, h->partA.p, (h->Np > 0 ? h->nblkP + h->nblkL : 0), uy_ptr(h)
  const int segl = pcg ? h->cam_segl : 64;
  const dim3 g(cam_grid(h, segl) + (pcg ? 1 : 0)), b(64 * WPB);
#define CS_PCG(R, JT)                                                                                       \
  do {                                                                                                      \
    if (segl == 16) BA_LAUNCH((k_cam_schur<CM, R, true, JT, 16>), g, b, 0, h->stream, CS_ARGS);        \
    else BA_LAUNCH((k_cam_schur<CM, R, true, JT, 64>), g, b, 0, h->stream, CS_ARGS);                   \
  } while (0)
  if (diag) {
    auto kern = robust ? k_camrow_schur_diag<CM, true> : k_camrow_schur_diag<CM, false>;
    BA_LAUNCH(kern, dim3(row_grid(h)), dim3(ROW_LANES * ROWS), 0, h->stream, h->cs[w].p, (const double*)h->intr[w].p, h->ptab[w].p,
                       h->offk.p, (robust ? h->c_ptf[h->lb].p : h->c_pt.p), h->c_w[h->lb].p, h->Hppinv[h->pb].p, h->K4[0],
                       h->K4[1], h->Nc, h->cam_band, h->fixed, p6_ptr(h), h->partE.p);
  } else if (pcg) {
    if (h->jac_f32) { if (robust) CS_PCG(true, float); else CS_PCG(false, float); }
    else            { if (robust) CS_PCG(true, double); else CS_PCG(false, double); }
  } else {
    if (robust) BA_LAUNCH((k_cam_schur<CM, true, false, double, 64>), g, b, 0, h->stream, CS_ARGS);
    else        BA_LAUNCH((k_cam_schur<CM, false, false, double, 64>), g, b, 0, h->stream, CS_ARGS);
  }
#undef CS_PCG
#undef CS_ARGS
}
static void launch_cam_schur(ba_handle* h, bool robust, bool diag, bool pcg, int k) {
  Scope sc(h, diag ? BA_K_PRECOND : BA_K_SCHUR_CAM);
  BA_BY_MODEL(h->model, launch_cam_schur_t<CM>(h, robust, diag, pcg, k));
}
// point pass with the camera vector in vtil; mode 0 = PCG iteration k, mode 1 = back substitution
// gmax_out (first PCG probe behind a fresh linearisation): host-mapped word that receives max |gradient|
// f32: the fp32-Jacobian instantiation (jacobian_precision = 1; mode 0 only -- the back substitution is always fp64)
template <class CM>
static void launch_pt_schur_t(ba_handle* h, bool robust, int mode, int k, double tol2, int min_iters, long long flag_base,
                              double* gmax_out, const CamUpdateArgs& cu, bool f32) {
  const int w = h->cur;
  const int ride = (mode == 1 || cu.fuse) ? cu.n_blocks : 0;      // the camera update as extra workgroups of the back substitution
                                                                  // (or of the PCG point pass that may turn into it: cu.fuse)
#define PS_HEAD h->camA[w].p, h->ptab[w].p, h->pt_off.p, (robust ? h->p_camf[h->pb].p : h->p_cam.p), h->p_w[h->pb].p,                 \
                h->Hppinv[h->pb].p, h->blk_win.p
#define PS_TAIL h->K4[0], h->K4[1], h->fixed, h->partA.p, k, h->st.p, h->partV.p, nbv(h), tol2, min_iters, h->y0[h->pb].p,     \
                h->Hpp[h->pb].p, h->bp[h->pb].p, h->ptab[1 - w].p, h->partB.p, flag, flag_base, h->verdict.p,                      \
                gmax_parts(h), gmax_count(h), (const double*)h->partGc.p, nbv(h), gmax_out, cu
  const size_t lds = std::max(lds_of(h), ride ? cu.groups * cam_update_lds_doubles<CM>() * sizeof(double) : (size_t)0) + (size_t)h->debug_lds_extra;
  long long* flag = (mode == 0 && flag_base > 0) ? h->d_flags : (long long*)nullptr;
  // data with long tracks: short and long tracks in one launch (workgroup 0 publishes the verdict)
#define PS_ONE(R, M, L, LN, JT) \
  BA_LAUNCH((k_pt_schur<CM, R, M, L, LN, JT>), dim3(h->nblkP + ride), dim3(PT_THREADS), lds, h->stream, PS_HEAD, wk, PS_TAIL)
#define PS_LAUNCH(R, M, L, JT)                                                                                              \
  do {                                                                                                                      \
    if (h->nblkL) BA_LAUNCH((k_pt_schur_both<CM, R, M, L, JT>), dim3(h->nblkP + h->nblkL + ride), dim3(PT_THREADS), lds,  \
                                     h->stream, PS_HEAD, wk, h->nblkP, wl, PS_TAIL);                                        \
    else {                                                                                                                  \
      switch (h->lanes) {                                                                                                   \
        case 4: PS_ONE(R, M, L, 4, JT); break;                                                                              \
        case 8: PS_ONE(R, M, L, 8, JT); break;                                                                              \
        case 16: PS_ONE(R, M, L, 16, JT); break;                                                                            \
        default: PS_ONE(R, M, L, 2, JT); break;                                                                             \
      }                                                                                                                     \
    }                                                                                                                       \
  } while (0)
#define PS_MODE(R, L)                                                                 \
  do {                                                                                \
    if (mode != 0) PS_LAUNCH(R, 1, L, double);                                        \
    else if (f32) PS_LAUNCH(R, 0, L, float);                                          \
    else PS_LAUNCH(R, 0, L, double);                                                  \
  } while (0)
  const PtWork wk = pt_work(h), wl = pt_work_long(h);
  if (all_lds_of(h)) { if (robust) PS_MODE(true, true); else PS_MODE(false, true); }
  else               { if (robust) PS_MODE(true, false); else PS_MODE(false, false); }
#undef PS_MODE
#undef PS_LAUNCH
#undef PS_ONE
#undef PS_HEAD
#undef PS_TAIL
}
static void launch_pt_schur(ba_handle* h, bool robust, int mode, int k, double tol2, int min_iters, long long flag_base = 0,
                            double* gmax_out = nullptr, const CamUpdateArgs* rider = nullptr, bool f32 = false) {
  if (h->Np == 0) {
    // an empty landmark shard (multi-rank): no point pass, but the PCG probe's verdict is still owed
    if (mode == 0 && flag_base > 0) {
      Scope sc(h, BA_K_SCHUR_PT);
      BA_LAUNCH(k_pcg_probe, dim3(1), dim3(64), 0, h->stream, k, h->st.p, h->partV.p, nbv(h), tol2, min_iters, h->d_flags,
                flag_base, h->verdict.p, gmax_parts(h), gmax_count(h), (const double*)h->partGc.p, nbv(h), gmax_out);
    }
    return;
  }
  Scope sc(h, mode == 0 ? BA_K_SCHUR_PT : BA_K_BACKSUB);
  CamUpdateArgs cu;
  if (rider) cu = *rider;
  else memset(&cu, 0, sizeof cu);
  BA_BY_MODEL(h->model, launch_pt_schur_t<CM>(h, robust, mode, k, tol2, min_iters, flag_base, gmax_out, cu, f32));
}

// multi-rank: a buffer of NPART per-partition partial sums is folded in place (partition 0 <- the sum
// in partition order, the others <- 0) and only partition 0 is all-reduced; the consumers, which add
// the NPART partitions, then read "total + 0 + ... + 0" and stay the kernels they are on one rank.
// An eighth of the bytes on the wire for two launch-floor kernels.  Single rank: nothing.
static int fold_and_reduce(ba_handle* h, double* parts, size_t n_per_part, double* msg, size_t msg_count) {
  if (!h->multi) return BA_OK;
  {
    Scope sc(h, BA_K_MISC);
    BA_LAUNCH(k_fold_parts, dim3((unsigned)((n_per_part + 255) / 256)), dim3(256), 0, h->stream, parts, n_per_part, NPART);
  }
  return allreduce(h, msg, msg_count);
}
// with_scalars: the step's six local sums (h->scal, written by k_scalars just before) ride in the message's header
static int exchange_partL(ba_handle* h, int buf, bool with_scalars = false) {
  if (!h->multi) return BA_OK;
  const size_t n = nl_of(h) * (size_t)h->Nc;
  HIPCHECK(h->linmsg[buf].alloc(8 + n));           // (sized in ba_set_problem; a communicator that joined after it: here)
  {
    Scope sc(h, BA_K_MISC);
    BA_LAUNCH(k_fold_lin, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, with_scalars ? (const double*)h->scal.p : (const double*)nullptr,
              (const double*)h->partL[buf].p, n, NPART, h->linmsg[buf].p);
  }
  return allreduce(h, h->linmsg[buf].p, 8 + n);
}
static int exchange_schur(ba_handle* h) {
  if (!h->multi) return BA_OK;
  // the message starts at the u.y word in front of partition 0
  return fold_and_reduce(h, p6_ptr(h), nb_of(h) * (size_t)h->Nc, uy_ptr(h), 2 + nb_of(h) * (size_t)h->Nc);
}
// The damped system's sums of a multi-rank job: W y0 (part6), the Schur-Jacobi blocks (partE, with_diag) and every rank's
// max |bp| travel in ONE message (k_fold_msg gathers and folds them, one all-reduce); k_pcg_setup and the first PCG probe
// read them from there.
static int exchange_system(ba_handle* h, bool with_diag) {
  if (!h->multi) return BA_OK;
  h->sys_diag = with_diag;
  const size_t n6 = nb_of(h) * (size_t)h->Nc, nE = sys_nE(h);
  HIPCHECK(h->sysmsg.alloc(2 + n6 + nE + (size_t)h->world + 8));
  {
    Scope sc(h, BA_K_MISC);
    BA_LAUNCH(k_fold_msg, dim3((unsigned)((n6 + nE + 255) / 256)), dim3(256), 0, h->stream, (const double*)uy_ptr(h),
              (const double*)p6_ptr(h), n6, (const double*)h->partE.p, nE, NPART,
              (const double*)h->partG[h->pb].p, h->Np > 0 ? h->nblkP + h->nblkL : 0, h->rank, h->world, h->sysmsg.p);
  }
  return allreduce(h, h->sysmsg.p, 2 + n6 + nE + (size_t)h->world);
}
// finalize = true: fold the fresh camera-half partials into Hcc | bc inside the same kernel
// precond: 0 = Jacobi blocks, 1 = Schur-Jacobi blocks from partE, 2 = keep the blocks already in Minv (k_pcg_setup)
static void launch_pcg_setup(ba_handle* h, double lambda, int precond, bool finalize) {
  Scope sc(h, BA_K_PCG_UPDATE);
#define SU_ARGS partL_of(h, h->lb), h->HccBc.p, bc_ptr(h), sys_p6(h), sys_E(h), nparts_of(h), h->cs[h->cur].p, lambda,           \
                precond, h->Nc, h->fixed, h->Hccd.p, h->Minv.p, h->gvec.p, h->x.p, h->r.p, h->p.p, h->s.p,     \
                h->z.p, h->camA[h->cur].p, h->partV.p, h->st.p, h->partGc.p, h->vx.p, \
                cam_held_ptr(h), cam_priors(h, h->cur, finalize), cam_gl_ptr(h)
  if (finalize) BA_BY_MODEL(h->model, BA_LAUNCH((k_pcg_setup<CM, true>), dim3(nbv(h)), dim3(VEC_BLOCK), 0, h->stream, SU_ARGS));
  else          BA_BY_MODEL(h->model, BA_LAUNCH((k_pcg_setup<CM, false>), dim3(nbv(h)), dim3(VEC_BLOCK), 0, h->stream, SU_ARGS));
#undef SU_ARGS
  // shared intrinsics: the group sums of the preconditioner's 3 x 3 blocks, of g and of bc, then the members' rows 6-8
  // and the workgroups' partials with the leader rule (ba_kernels.hpp, "shared intrinsics")
  if (h->shared_on) {
    const int keep = precond == 2 ? 1 : 0;
    BA_LAUNCH(k_shared_sum<BalCam>, dim3(h->n_shared), dim3(SHARED_BLOCK), 0, h->stream, (const int*)h->grp_off.p, (const int*)h->grp_mem.p,
              keep, (const double*)h->Minv.p, (const double*)h->gvec.p, (const double*)bc_ptr(h), h->grp_rec.p);
    BA_LAUNCH(k_shared_finish<BalCam>, dim3(nbv(h)), dim3(VEC_BLOCK), 0, h->stream, (const int*)h->cam_gl.p, (const double*)h->grp_rec.p,
              keep, h->Nc, (const double*)h->Hccd.p, (const double*)bc_ptr(h), h->Minv.p, h->gvec.p, h->r.p, h->z.p, h->camA[h->cur].p,
              h->partV.p, h->partGc.p);
  }
}

// ------------------------------------------------------------------------------------------------------------------
// bal_enter / bal_leave: the two ends of with_model() below, the scope in which every entry point that takes `intr` runs
// its body with the BAL 9-parameter camera [rvec | t | f k1 k2] (BASELINE config 5 is stated
// on a BAL problem; the reference's only camera is cv2.projectPoints(..., distCoeffs=None), src/bundle_adjuster.py:67).
// Cameras (rvec, t) and points are the handle's (ba_set_params / ba_get_params); the per-camera (f, k1, k2) travel with the call.  K4 of
// ba_set_problem is not used.  The entry points switch the handle to the BalCam instantiation of every kernel
// (ba_models.hpp) for the duration of the call: same LM / Schur / PCG loop, same device-side verdicts and speculation,
// same multi-rank exchange, 9x9 camera blocks.
static int bal_enter(ba_handle* h, const double* intr) {
  HIPCHECK(hipMemcpyAsync(h->intr[h->cur].p, intr, 3 * (size_t)h->Nc * sizeof(double), hipMemcpyHostToDevice, h->stream));
  h->model = 1;
  h->linearized = false;
  BA_LAUNCH(k_cam_prepare<BalCam>, dim3((h->Nc + 63) / 64), dim3(64), 0, h->stream, h->cams[h->cur].p, (const double*)h->intr[h->cur].p,
            h->cs[h->cur].p, h->camA[h->cur].p, h->Nc);
  return BA_OK;
}
// back to the pinhole layout of the camera table (what every other entry point reads), at the current parameters
static void bal_leave(ba_handle* h) {
  h->model = 0;
  h->linearized = false;                      // the linearisation buffers hold 9-parameter blocks
  BA_LAUNCH(k_cam_prepare<Pinhole>, dim3((h->Nc + 63) / 64), dim3(64), 0, h->stream, h->cams[h->cur].p, (const double*)h->intr[h->cur].p,
            h->cs[h->cur].p, h->camA[h->cur].p, h->Nc);
}
// The model scope: body() with the BAL camera of `intr` (null: the pinhole, no switch).  Whatever way body() ends, the
// handle is the pinhole's again and idle: after a failure the stream is drained and a refused launch forgotten (the
// failure that is reported is the first one, whose text is kept), then the pinhole camera state is rebuilt at the current
// parameters -- a failure in the middle of a solve may have left it behind them -- and the stream drained.
template <class Body>
static int with_model(ba_handle* h, const double* intr, Body body) {
  if (intr) if (int rc = bal_enter(h, intr)) { h->model = 0; return rc; }
  int rc = body();
  const std::string msg = g_err;
  if (rc != BA_OK) { (void)hipStreamSynchronize(h->stream); h->launch_err = hipSuccess; }
  if (intr) {
    bal_leave(h);
    if (hipStreamSynchronize(h->stream) != hipSuccess && rc == BA_OK) return fail(BA_ERR_HIP, "stream synchronise failed");
  }
  g_err = msg;
  return rc;
}

// What the evaluating entry points (ba_residuals*, ba_linearize*, ba_schur_system, ba_covariance) check alike, behind their
// own null-argument test.  pinhole_refuses: what a call with the pinhole camera cannot honour -- CK_BAL_BITS: held f, k1, k2
// and 9-parameter priors, CK_SHARED: shared intrinsics; 0 for a BAL call and for the residual, which reads neither.
enum { CK_BAL_BITS = 1, CK_SHARED = 2 };
static int check_eval(const ba_handle* h, int32_t loss, double f_scale, int pinhole_refuses) {
  if (!h->have_params) return fail(BA_ERR_STATE, "ba_set_problem / ba_set_params first");
  if ((pinhole_refuses & CK_BAL_BITS) && (h->cam_held_or & ~0x3fu))
    return fail(BA_ERR_INVALID, "camera mask bits 6-8 (f, k1, k2) need the BAL camera model");
  if ((pinhole_refuses & CK_SHARED) && h->n_shared) return fail(BA_ERR_INVALID, "%s", kSharedNeedsBal);
  if ((pinhole_refuses & CK_BAL_BITS) && h->prior_nb == 9) return fail(BA_ERR_INVALID, "%s", kPriorNeedsBal);
  if (!loss_valid(loss)) return fail(BA_ERR_INVALID, "unknown loss %d", loss);
  if (!(f_scale > 0)) return fail(BA_ERR_INVALID, "f_scale must be positive");
  return BA_OK;
}

// --------------------------------------------------------------------- K1 entry points
// intr != NULL: the BAL 9-parameter camera (row f2) on the same problem upload and row order, the cameras' (f, k1, k2)
// handed over per call and staged in h->tri; the handle's K4 is then not used.
static int residuals_impl(ba_handle* h, const double* intr, int32_t loss, double f_scale, double* r, double* sse, double* cost) {
  if (int rc = check_eval(h, loss, f_scale, 0)) return rc;
  if (set_device(h)) return BA_ERR_HIP;
  if (intr) {
    HIPCHECK(h->tri.alloc(3 * (size_t)h->Nc + 8));
    HIPCHECK(hipMemcpyAsync(h->tri.p, intr, 3 * (size_t)h->Nc * sizeof(double), hipMemcpyHostToDevice, h->stream));
  }
  double* rdev = nullptr;
  if (r && h->Nobs > 0) {
    HIPCHECK(h->rbuf.alloc(2 * (size_t)h->Nobs));
    rdev = h->rbuf.p;
  }
  launch_residual(h, h->cur, (ba_loss)loss, f_scale, rdev, intr ? h->tri.p : nullptr);
  launch_scalars(h, false);
  if (int rc = allreduce(h, h->scal.p, 2)) return rc;
  HIPCHECK(hipMemcpyAsync(h->h_scal, h->scal.p, 2 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (rdev) HIPCHECK(hipMemcpyAsync(r, rdev, 2 * (size_t)h->Nobs * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  BA_SYNC(h);
  if (sse) *sse = h->h_scal[0];
  if (cost) *cost = 0.5 * h->h_scal[1];
  return BA_OK;
}
extern "C" int ba_residuals(ba_handle* h, int32_t loss, double f_scale, double* r, double* sse, double* cost) {
  if (!h) return fail(BA_ERR_INVALID, "null handle");
  return residuals_impl(h, nullptr, loss, f_scale, r, sse, cost);
}
extern "C" int ba_residuals_bal(ba_handle* h, const double* intr, int32_t loss, double f_scale, double* r, double* sse,
                                double* cost) {
  if (!h || !intr) return fail(BA_ERR_INVALID, "null argument");
  return residuals_impl(h, intr, loss, f_scale, r, sse, cost);
}

// --------------------------------------------------------------------- K2 entry points
// per-point blocks back in the caller's point order: `width` doubles per point of src, through `tmp`, to the host
static int copy_point_rows(ba_handle* h, const double* src, int width, double* tmp, double* host) {
  if (!host || !h->Np) return BA_OK;
  BA_LAUNCH(k_unpermute_rows, dim3((h->Np + 255) / 256), dim3(256), 0, h->stream, src, h->slot.p, h->Np, width, tmp);
  HIPCHECK(hipMemcpyAsync(host, tmp, width * (size_t)h->Np * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  return BA_OK;
}
// intr != NULL: the BAL camera, 45 + 9 doubles per camera in Hcc | bc
static int linearize_impl(ba_handle* h, const double* intr, int32_t loss, double f_scale, double* Hcc, double* bc, double* Hpp, double* bp) {
  if (int rc = check_eval(h, loss, f_scale, intr ? 0 : CK_BAL_BITS | CK_SHARED)) return rc;
  if (set_device(h)) return BA_ERR_HIP;
  return with_model(h, intr, [&]() -> int {
    launch_lin_cam(h, h->cur, h->lb, (ba_loss)loss, f_scale);
    if (int rc = exchange_partL(h, h->lb)) return rc;
    launch_lin_finalize(h);
    launch_lin_pt(h, h->cur, h->pb, (ba_loss)loss, f_scale, 1.0);
    if (!intr) {                  // (a BAL linearisation does not outlive its scope)
      h->linearized = true;
      h->lin_loss = (ba_loss)loss;
      h->lin_fscale = f_scale;
    }
    if (Hcc) HIPCHECK(hipMemcpyAsync(Hcc, h->HccBc.p, nh_of(h) * (size_t)h->Nc * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (bc) HIPCHECK(hipMemcpyAsync(bc, bc_ptr(h), nb_of(h) * (size_t)h->Nc * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if ((Hpp || bp) && h->Np) HIPCHECK(h->rbuf.alloc(6 * (size_t)h->Np));
    if (int rc = copy_point_rows(h, h->Hpp[h->pb].p, 6, h->rbuf.p, Hpp)) return rc;
    if (int rc = copy_point_rows(h, h->bp[h->pb].p, 3, h->stage.p, bp)) return rc;
    BA_SYNC(h);
    return BA_OK;
  });
}
extern "C" int ba_linearize(ba_handle* h, int32_t loss, double f_scale, double* Hcc, double* bc, double* Hpp, double* bp) {
  if (!h) return fail(BA_ERR_INVALID, "null handle");
  return linearize_impl(h, nullptr, loss, f_scale, Hcc, bc, Hpp, bp);
}
extern "C" int ba_linearize_bal(ba_handle* h, const double* intr, int32_t loss, double f_scale, double* Hcc, double* bc,
                                double* Hpp, double* bp) {
  if (!h || !intr) return fail(BA_ERR_INVALID, "null argument");
  return linearize_impl(h, intr, loss, f_scale, Hcc, bc, Hpp, bp);
}

// --------------------------------------------------------------------- K4 test hooks
// invert: (re)compute the damped point inverses (not needed right after launch_lin_pt at the
// same lambda); finalize: Hcc | bc still have to be folded from the camera-half partials
// keep = true (Schur-Jacobi only, ba_options.precond_lag): the preconditioner blocks in Minv stay as they are -- the
// right-hand side W y0 then comes from the 6-sum camera pass (k_cam_schur) instead of the 27-sum one that also builds
// the blocks' Schur terms, and k_pcg_setup neither folds them nor inverts anything
static int damped_system(ba_handle* h, double lambda, bool schur_diag, bool invert = true, bool finalize = false, bool keep = false) {
  if (invert) launch_point_invert(h, lambda);
  const bool diag_pass = schur_diag && !keep;
  launch_cam_schur(h, h->lin_loss != BA_LOSS_LINEAR, diag_pass, false, 0);
  if (int rc = exchange_system(h, diag_pass)) return rc;
  launch_pcg_setup(h, lambda, schur_diag ? (keep ? 2 : 1) : 0, finalize);
  if (schur_diag) h->stats[keep ? BA_STAT_PRECOND_REUSES : BA_STAT_PRECOND_BUILDS]++;
  return BA_OK;
}

// The reduced camera system exactly as one LM iteration of ba_solve forms and uses it: linearisation at the current
// parameters (camera half, point half with the damped inverses at lambda), then damped_system() for the right-hand side g
// and the preconditioner blocks Minv, then S v for each of n_vec vectors in the PCG loop's launch form -- the point pass
// mode 0 (fp32 Jacobian blocks when jacobian_precision = 1), the camera pass k_cam_schur<.., PCG = true, .., cam_segl>
// behind a "go on" verdict for iteration 0 -- with Hccd v - W y folded per camera by k_schur_combine.
// precond 2: the blocks are built at lambda_prev and kept for the system at lambda (ba_options.precond_lag: g then comes
// from the 6-sum camera pass).  intr != NULL: the BAL camera (with_model).
extern "C" int ba_schur_system(ba_handle* h, const double* intr, int32_t loss, double f_scale, double lambda, int32_t precond,
                               double lambda_prev, int32_t jacobian_precision, int32_t n_vec, const double* v, double* sv,
                               double* g, double* minv) {
  if (!h) return fail(BA_ERR_INVALID, "null handle");
  if (n_vec < 0 || (n_vec > 0 && (!v || !sv))) return fail(BA_ERR_INVALID, "n_vec vectors need v and sv");
  if (int rc = check_eval(h, loss, f_scale, intr ? 0 : CK_BAL_BITS)) return rc;
  if (precond < 0 || precond > 2) return fail(BA_ERR_INVALID, "precond must be 0 (Jacobi), 1 (Schur-Jacobi) or 2 (Schur-Jacobi kept)");
  if (jacobian_precision != 0 && jacobian_precision != 1)
    return fail(BA_ERR_INVALID, "jacobian_precision must be 0 (f64) or 1 (f32 blocks, f64 accumulation)");
  if (set_device(h)) return BA_ERR_HIP;
  const bool jac_f32_was = h->jac_f32;
  const int rc = with_model(h, intr, [&]() -> int {
    const ba_loss ls = (ba_loss)loss;
    const bool robust = ls != BA_LOSS_LINEAR;
    const int nb = nb_of(h), nh = nh_of(h);
    launch_lin_cam(h, h->cur, h->lb, ls, f_scale);
    if (int rc = exchange_partL(h, h->lb)) return rc;
    h->lin_loss = ls; h->lin_fscale = f_scale;
    if (precond == 2) {            // blocks built at lambda_prev (a fresh system), then the same linearisation damped again
      launch_lin_pt(h, h->cur, h->pb, ls, f_scale, lambda_prev);
      if (int rc = damped_system(h, lambda_prev, true, false, true, false)) return rc;
      if (int rc = damped_system(h, lambda, true, true, false, true)) return rc;
    } else {
      launch_lin_pt(h, h->cur, h->pb, ls, f_scale, lambda);
      if (int rc = damped_system(h, lambda, precond == 1, false, true, false)) return rc;
    }
    h->linearized = true;
    if (g) HIPCHECK(hipMemcpyAsync(g, h->gvec.p, nb * (size_t)h->Nc * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (minv) HIPCHECK(hipMemcpyAsync(minv, h->Minv.p, nh * (size_t)h->Nc * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    h->jac_f32 = jacobian_precision == 1;
    for (int i = 0; i < n_vec; ++i) {
      const size_t n = nb * (size_t)h->Nc;
      HIPCHECK(hipMemcpyAsync(h->vin.p, v + i * n, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
      {
        Scope sc(h, BA_K_MISC);
        BA_BY_MODEL(h->model, BA_LAUNCH(k_vtil<CM>, dim3((h->Nc + 63) / 64), dim3(64), 0, h->stream, h->vin.p, h->cs[h->cur].p, h->Nc, h->fixed,
                                        h->camA[h->cur].p, cam_held_ptr(h)));
        // a not-converged PCG state, so that the probe of iteration 0 finds "go on" (tol2 < 0), and the same verdict word
        // written here for the camera pass (no point pass on an empty landmark shard)
        BA_LAUNCH(k_pcg_reset, dim3(1), dim3(64), 0, h->stream, h->st.p, h->partV.p, nbv(h));
        HIPCHECK(hipMemsetAsync(h->verdict.p, 0, 4 * sizeof(double), h->stream));
      }
      // flag_base 0: no probe word for the host; y = Hppinv W^T v into the point table, then the camera pass
      launch_pt_schur(h, robust, 0, 0, -1.0, 1 << 30, 0, nullptr, nullptr, h->jac_f32);
      launch_cam_schur(h, robust, false, true, 0);
      if (int rc = exchange_schur(h)) return rc;
      {
        Scope sc(h, BA_K_MISC);
        BA_BY_MODEL(h->model, BA_LAUNCH(k_schur_combine<CM>, dim3((h->Nc + 63) / 64), dim3(64), 0, h->stream, h->Hccd.p, h->vin.p, p6_ptr(h),
                                        nparts_of(h), h->cs[h->cur].p, h->Nc, h->fixed, h->z.p, cam_held_ptr(h)));
      }
      HIPCHECK(hipMemcpyAsync(sv + i * n, h->z.p, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    }
    BA_SYNC(h);
    return BA_OK;
  });
  h->jac_f32 = jac_f32_was;
  return rc;
}

// ----------------------------------------------------------------------------- solve
extern "C" int ba_default_options(ba_options* o) {
  if (!o) return fail(BA_ERR_INVALID, "null options");
  memset(o, 0, sizeof *o);
  o->loss = BA_LOSS_HUBER;          // src/bundle_adjuster.py:171
  o->max_iters = 50;                // max_nfev=50, :173
  o->f_scale = 1.0;
  o->ftol = 1e-5;                   // :173
  o->xtol = 1e-5;                   // :173
  o->gtol = 1e-8;                   // scipy default (least_squares.py:241-245)
  o->initial_lambda = 1e-4;
  o->pcg_tol = 0.1;
  o->pcg_max_iters = 200;
  o->pcg_min_iters = 1;
  o->preconditioner = BA_PRECOND_SCHUR_JACOBI;
  o->jacobian_precision = 0;
  o->reserved0 = 0;
  o->profile = 0;
  o->verbose = 0;
  o->pcg_model_tol = -1.0;          // Nash & Sofer's truncated-Newton test on the quadratic model: automatic -- 0.5 (their value) on
                                    // band-structured problems, off otherwise (ba_hip.h)
  o->pcg_model_min_iters = 5;
  o->precond_lag = 3;
  return BA_OK;
}

static double now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

static int eval_cost(ba_handle* h, int which, ba_loss loss, double fscale, double* sse, double* cost) {
  launch_residual(h, which, loss, fscale, nullptr);
  launch_prior_cost(h, which);
  launch_scalars(h, false);
  if (int rc = allreduce(h, h->scal.p, 2)) return rc;
  HIPCHECK(hipMemcpyAsync(h->h_scal, h->scal.p, 2 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  BA_SYNC(h);
  *sse = h->h_scal[0];
  *cost = 0.5 * h->h_scal[1];
  return BA_OK;
}

static int solve_impl(ba_handle* h, const ba_options* opts, ba_summary* sum);
extern "C" int ba_solve(ba_handle* h, const ba_options* opts, ba_summary* sum) {
  if (!h || !opts || !sum) return fail(BA_ERR_INVALID, "null argument");
  const int rc = solve_impl(h, opts, sum);
  if (rc != BA_OK) {             // leave the handle usable: nothing queued, no launch remembered as refused
    const std::string msg = g_err;
    (void)hipStreamSynchronize(h->stream);
    h->launch_err = hipSuccess;
    h->linearized = false;
    g_err = msg;
  }
  // the per-solve modes (solve_impl sets them in one place), off again behind every exit, successful or not
  if (h->profile) flush_profile(h);
  h->profile = false;
  h->jac_f32 = false;
  h->fold_prior_rows = 0;        // (ba_residuals* and the test hooks fold the reprojection rows only)
  h->shared_on = false;          // (... and report per-camera quantities)
  return rc;
}
// Sliding-window-sized problems (ba_small.hpp): the whole LM loop in one kernel launch, dense Cholesky of the reduced
// system instead of PCG.  Same options, summary and trace as the multi-kernel path.
static bool small_mw_wanted(const ba_handle* h) {          // BA_SMALL_MW=0: always the one-workgroup kernel
  const char* mw_env = getenv("BA_SMALL_MW");
  return h->mw_ok && (!mw_env || atoi(mw_env) != 0);
}
// diagnostic stamps of LM iteration 2 (BA_SMALL_STAMPS), as either window kernel left them
static int report_small_stamps(const long long* stamps, bool used_mw) {
  long long st[16];
  HIPCHECK(hipMemcpy(st, stamps, sizeof st, hipMemcpyDeviceToHost));
  if (used_mw) {
    static const char* names[] = {"C1 camera half (slices)", "P1 point half + V (8 lanes / landmark)", "G  [V;z][V;z]^T (MFMA, LDS) + message",
                                  "exchange 1 (barrier + gather)", "S, g", "elimination + back substitution", "camera update + P2", "C3 trial cost (slices)", "exchange 2"};
    for (int k = 0; k < 9; ++k) fprintf(stderr, "[k_small_mw, LM iteration 2, workgroup 0] %-40s %7.2f us\n", names[k], (st[k + 1] - st[k]) * 0.01);
    fprintf(stderr, "[k_small_mw] elimination %.2f us, back substitution %.2f us\n", (st[13] - st[12]) * 0.01, (st[6] - st[13]) * 0.01);
  } else {
    static const char* names[] = {"C1 camera half", "P1 point half + V", "G  [V;z][V;z]^T (MFMA)", "S, g from the tiles", "Cholesky + solves (1 wave)",
                                  "camera update", "P2 back substitution", "C3 trial cost"};
    for (int k = 0; k < 8; ++k) fprintf(stderr, "[k_small_lm, LM iteration 2] %-28s %7.2f us\n", names[k], (st[k + 1] - st[k]) * 0.01);
    fprintf(stderr, "[k_small_lm] wave 0: factor %.2f us, forward %.2f us, backward %.2f us\n", (st[13] - st[4]) * 0.01, (st[14] - st[13]) * 0.01, (st[5] - st[14]) * 0.01);
    fprintf(stderr, "[k_small_lm] shader clock over the iteration: %.2f GHz\n", (double)(st[10] - st[9]) / ((st[8] - st[0]) * 10.0));
  }
  return BA_OK;
}
static bool small_applies(const ba_handle* h, const ba_options* opts) {
  // (the observation limit is the measured crossover of the ONE-workgroup kernel with the multi-kernel path; a window that
  // fits the multi-workgroup kernel -- five cameras, 2048 landmarks: at most 10 k observations -- is far below its own)
  const bool mw = small_mw_wanted(h);
  if (any_prior(h)) return false;      // priors: the multi-kernel path (the window kernels do not know them; ba_hip.h)
  return opts->small_solver == 0 && !h->multi && h->Nc <= SMALL_MAX_CAMS && h->Np > 0 && h->Nobs > 0 && (h->Nobs <= SMALL_MAX_OBS || mw) &&
         opts->max_iters >= 1;
}
static int small_solve(ba_handle* h, const ba_options* opts, ba_summary* sum) {
  const double t_begin = now_s();
  const size_t off_cur = sizeof(ba_summary), off_trace = 256;
  const size_t bytes = off_trace + sizeof(ba_iter_record) * (size_t)opts->max_iters;
  if (h->h_small_bytes < bytes) {
    if (h->h_small) { BA_SYNC(h); (void)hipHostFree(h->h_small); h->h_small = nullptr; h->h_small_bytes = 0; }
    HIPCHECK(hipHostMalloc((void**)&h->h_small, bytes, hipHostMallocMapped | hipHostMallocCoherent));
    HIPCHECK(hipHostGetDevicePointer((void**)&h->d_small_host, h->h_small, 0));
    h->h_small_bytes = bytes;
  }
  SmallArgs A;
  for (int k = 0; k < 2; ++k) { A.cams[k] = h->cams[k].p; A.cs[k] = h->cs[k].p; A.ptab[k] = h->ptab[k].p; A.camA[k] = h->camA[k].p; }
  A.offk = h->offk.p; A.c_pt = h->c_pt.p; A.c_uv = h->c_uv.p;
  A.pt_off = h->pt_off.p; A.p_cam = h->p_cam.p; A.p_uv = h->p_uv.p;
  A.Hpp = h->Hpp[h->pb].p; A.bp = h->bp[h->pb].p; A.Lf = h->Hppinv[h->pb].p; A.y0 = h->y0[h->pb].p;
  A.Np_pad = (h->Np + 15) & ~15;
  A.Kp = 3 * A.Np_pad;
  bool used_mw = small_mw_wanted(h);
  HIPCHECK(h->small_gS.alloc((size_t)SMALL_WAVES * SMALL_TILES * 256 + 16));        // + 16 words of diagnostic stamps
  A.gS = h->small_gS.p;
  A.n_cams = h->Nc; A.n_pts = h->Np; A.fixed_cam = h->fixed; A.loss = opts->loss;
  for (int c = 0; c < 8; ++c) A.cam_held[c] = (h->any_cam_held && c < h->Nc) ? h->h_cam_held[c] : 0;
  A.pt_held = pt_held_ptr(h);
  A.fx = h->K4[0]; A.fy = h->K4[1]; A.cx = h->K4[2]; A.cy = h->K4[3]; A.hub_c = opts->f_scale;
  A.max_iters = opts->max_iters; A.ftol = opts->ftol; A.xtol = opts->xtol; A.gtol = opts->gtol; A.lambda0 = opts->initial_lambda;
  A.cur = h->cur;
  A.summary = (ba_summary*)h->d_small_host;
  A.cur_out = (int*)(h->d_small_host + off_cur);
  A.trace = (ba_iter_record*)(h->d_small_host + off_trace);
  A.host_flag = h->d_flags + 4;
  A.stamps = getenv("BA_SMALL_STAMPS") ? (long long*)(h->small_gS.p + (size_t)SMALL_WAVES * SMALL_TILES * 256) : nullptr;   // device memory: a host store would stall the wave
  // one launch of either kernel and the wait for its result word: the kernel's last act is a system-scope release of the
  // sequence word -- summary, parameter set and trace are in host memory by then, and whatever the caller queues next on
  // the stream is ordered behind the kernel as usual
  auto run_once = [&](bool mw) -> int {
    if (!mw && h->small_np_pad != A.Np_pad) {             // columns of padding points and rows past 6 Nc stay zero for good
      const size_t nv = (size_t)SMALL_VROWS * A.Kp;       // (k_small_mw keeps its columns of V in LDS: nothing to clear)
      HIPCHECK(h->small_V.alloc(nv));
      HIPCHECK(hipMemsetAsync(h->small_V.p, 0, nv * sizeof(double), h->stream));
      h->small_np_pad = A.Np_pad;
    }
    A.V = h->small_V.p;
    memset(h->h_small, 0, off_trace);
    A.seq = ++h->small_seq;
    if (mw) {           // several workgroups: 64 landmarks each, two exchanges per LM iteration (ba_small_mw.hpp)
      MwArgs M;
      M.A = A; M.woff = h->mw_woff.p; M.G = h->mw_G;
      // (test hook BA_DEBUG_MW_EXTRA_WG: every barrier waits for one workgroup more than the launch has -- the time-out path)
      M.G_barrier = h->mw_G + (getenv("BA_DEBUG_MW_EXTRA_WG") ? 1 : 0);
      M.slots = h->mw_buf.p; M.sslots = h->mw_buf.p + (size_t)2 * MW_MAX_WG * MW_MSG;
      M.ctr = (unsigned long long*)(h->mw_buf.p + (size_t)2 * MW_MAX_WG * (MW_MSG + MW_SCAL));
      Scope sc(h, BA_K_MISC);
      // instantiated per number of 16-row tiles of [V; z]: 6 Nc + 1 rows
      if (h->Nc <= 5)      BA_LAUNCH(k_small_mw<2>, dim3(h->mw_G), dim3(MW_THREADS), 0, h->stream, M);
      else if (h->Nc <= 7) BA_LAUNCH(k_small_mw<3>, dim3(h->mw_G), dim3(MW_THREADS), 0, h->stream, M);
      else                 BA_LAUNCH(k_small_mw<4>, dim3(h->mw_G), dim3(MW_THREADS), 0, h->stream, M);
      h->stats[BA_STAT_WINDOW_MW_LAUNCHES]++;
    } else {
      Scope sc(h, BA_K_MISC);
      BA_LAUNCH(k_small_lm, dim3(1), dim3(SMALL_THREADS), 0, h->stream, A);
      h->stats[BA_STAT_WINDOW_LM_LAUNCHES]++;
    }
    if (int rc = wait_flag(h, 4, A.seq)) return rc;
    memcpy(sum, h->h_small, sizeof(ba_summary));
    return BA_OK;
  };
  if (int rc = run_once(used_mw)) return rc;
  if (used_mw && sum->status == BA_ERR_HIP) {
    // A workgroup of k_small_mw was not served at a barrier within MW_SPIN_TICKS: its G workgroups were not resident
    // together (another stream, handle or tool holds compute units).  The window is solved again, in this process, by the
    // one-workgroup kernel from the SAME start point: the cameras of the start set were never written (only the final block
    // of a successful solve stores them), the landmarks' start positions are restored from the y slots every workgroup
    // parked them in.  Workgroups of the failed launch that were still queued run (and give up) first: stream order.
    if (h->Np > 0)
      BA_LAUNCH(k_small_restore, dim3((h->Np + 255) / 256), dim3(256), 0, h->stream, h->ptab[A.cur].p, h->Np);
    h->stats[BA_STAT_WINDOW_FALLBACKS]++;
    used_mw = false;
    if (int rc = run_once(false)) return rc;
  }
  if (sum->status == BA_ERR_HIP) return fail(BA_ERR_HIP, "the window solver reported a device-side failure");
  if (sum->status == BA_ERR_NUMERIC)
    return fail(BA_ERR_NUMERIC, sum->iterations == 0 ? "non-finite cost at the initial parameters"
                                                     : "non-finite cost / gradient during the solve (LM iteration %d)", sum->iterations);
  if (sum->iterations > 0) {
    h->trace.resize((size_t)sum->iterations);
    memcpy(h->trace.data(), h->h_small + off_trace, sizeof(ba_iter_record) * (size_t)sum->iterations);
  }
  memcpy(&h->cur, h->h_small + off_cur, sizeof(int));
  if (A.stamps)
    if (int rc = report_small_stamps(A.stamps, used_mw)) return rc;
  h->linearized = false;
  sum->seconds_total = now_s() - t_begin;
  const double per = sum->iterations ? sum->seconds_total / sum->iterations : 0.0;
  for (auto& r : h->trace) r.seconds = per;
  return BA_OK;
}

// ------------------------------------------------------------------------------------------------- covariances
// Marginal covariances at the current parameters (csrc/ba_cov.hpp): the camera half and the point half of a linearisation
// (Hcc, Hpp; the damped point inverses it also writes are not used), S assembled densely from them and the per-observation
// W blocks, factorised and inverted in place, the points' blocks from the inverse.  One drain in the middle (the pair
// scan of the point-ordered observations is formed on the host from pt_off), one at the end, where the failure words of
// the rank tests are read; outputs are copied only when nothing failed.
static const char* cov_param_name(int q) {
  static const char* names[9] = {"rvec[0]", "rvec[1]", "rvec[2]", "t[0]", "t[1]", "t[2]", "f", "k1", "k2"};
  return names[q];
}
template <class CM>
static int cov_impl(ba_handle* h, ba_loss loss, double f_scale, double rcond, double* cam_cov, double* pt_cov, double* cam_full) {
  constexpr int NB = CM::NB, NH = CM::NH;
  const int Nc = h->Nc, Np = h->Np, n = NB * Nc;
  const int npad = ((n + COV_T - 1) / COV_T) * COV_T, nt = npad / COV_T;
  launch_lin_cam(h, h->cur, h->lb, loss, f_scale);
  if (int rc = exchange_partL(h, h->lb)) return rc;
  launch_lin_finalize(h);
  launch_lin_pt(h, h->cur, h->pb, loss, f_scale, 1.0);
  h->linearized = true;
  h->lin_loss = loss;
  h->lin_fscale = f_scale;
  // pair numbering: exclusive scan of L_p (L_p + 1) / 2 over the point slots, in 64 bits
  std::vector<int> off((size_t)Np + 1, 0);
  std::vector<long long> poff((size_t)Np + 1, 0);
  if (Np) HIPCHECK(hipMemcpyAsync(off.data(), h->pt_off.p, ((size_t)Np + 1) * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  BA_SYNC(h);
  for (int s = 0; s < Np; ++s) {
    const long long L = off[s + 1] - off[s];
    poff[s + 1] = poff[s] + L * (L + 1) / 2;
  }
  const long long n_pairs = poff[Np];
  DBuf<double> A, dS, tinv, P, D, Vinv, Wbuf, ptc, blk;
  DBuf<long long> dpoff;
  DBuf<unsigned char> status;
  DBuf<int> failw;
  HIPCHECK(A.alloc((size_t)npad * npad));
  HIPCHECK(dS.alloc(npad)); HIPCHECK(tinv.alloc(COV_T * COV_T)); HIPCHECK(P.alloc((size_t)npad * COV_T)); HIPCHECK(D.alloc(COV_T * COV_T));
  HIPCHECK(Vinv.alloc(6 * (size_t)std::max(Np, 1))); HIPCHECK(status.alloc(std::max(Np, 1)));
  HIPCHECK(Wbuf.alloc((size_t)NB * 3 * std::max(h->Nobs, 1))); HIPCHECK(dpoff.alloc((size_t)Np + 1)); HIPCHECK(failw.alloc(2));
  HIPCHECK(hipMemsetAsync(failw.p, 0x7f, 2 * sizeof(int), h->stream));
  HIPCHECK(hipMemcpyAsync(dpoff.p, poff.data(), ((size_t)Np + 1) * sizeof(long long), hipMemcpyHostToDevice, h->stream));
  // S = U - W V^-1 W^T, held rows identity
  if (Np) BA_LAUNCH(k_cov_points, dim3((Np + 255) / 256), dim3(256), 0, h->stream, h->slot.p, h->pt_off.p, h->p_cam.p,
                    h->Hpp[h->pb].p, pt_held_ptr(h), Np, rcond, status.p, Vinv.p, failw.p,
                    h->any_pt_prior ? (const double*)h->pt_info.p : (const double*)nullptr);
  BA_LAUNCH(k_cov_diag<NB>, dim3((NH * Nc + (npad - n) + 255) / 256), dim3(256), 0, h->stream, h->HccBc.p, Nc, npad, A.p);
  if (Np) {
    BA_LAUNCH(k_cov_w<CM>, dim3((Np + 3) / 4), dim3(256), 0, h->stream, h->cs[h->cur].p, (const double*)h->intr[h->cur].p,
              h->ptab[h->cur].p, h->pt_off.p, h->p_cam.p, uv_arr(h, h->p_uv), status.p, Np, h->K4[0], h->K4[1], h->K4[2], h->K4[3],
              f_scale, (int)loss, Wbuf.p, A.p, npad);
    if (n_pairs > 0) {
      const long long g = std::min<long long>((n_pairs + 255) / 256, 64ll * h->n_cu);
      BA_LAUNCH(k_cov_pairs<NB>, dim3((unsigned)g), dim3(256), 0, h->stream, dpoff.p, Np, h->pt_off.p, h->p_cam.p, status.p, Vinv.p,
                Wbuf.p, A.p, npad);
    }
  }
  const bool any_held = h->fixed >= 0 || h->any_cam_held;
  if (any_held) BA_LAUNCH(k_cov_held, dim3(1, n), dim3(256), 0, h->stream, cam_held_ptr(h), h->fixed, NB, n, npad, 1.0, A.p);
  BA_LAUNCH(k_cov_save_diag, dim3((npad + 255) / 256), dim3(256), 0, h->stream, A.p, npad, dS.p);
  // potrf
  for (int kt = 0; kt < nt; ++kt) {
    const int m = nt - kt - 1;
    BA_LAUNCH(k_cov_potrf_diag, dim3(1), dim3(256), 0, h->stream, A.p, npad, kt, dS.p, n, rcond, failw.p, tinv.p);
    if (m == 0) continue;
    BA_LAUNCH(k_cov_potrf_panel, dim3(m), dim3(256), 0, h->stream, A.p, npad, kt, tinv.p);
    BA_LAUNCH(k_cov_potrf_update, dim3(m * (m + 1) / 2), dim3(256), 0, h->stream, A.p, npad, kt);
  }
  // trtri: L^-1, tile columns last to first
  for (int jt = nt - 1; jt >= 0; --jt) {
    const int m = nt - jt - 1;
    BA_LAUNCH(k_cov_trtri_diag, dim3(1), dim3(256), 0, h->stream, A.p, npad, jt, tinv.p);
    if (m == 0) continue;
    BA_LAUNCH(k_cov_trtri_panel, dim3(m), dim3(256), 0, h->stream, (const double*)A.p, npad, jt, (const double*)tinv.p, P.p);
    BA_LAUNCH(k_cov_trtri_update, dim3(m), dim3(256), 0, h->stream, A.p, npad, jt, (const double*)P.p);
  }
  // lauum: L^-T L^-1, tile rows first to last
  for (int it = 0; it < nt; ++it) {
    BA_LAUNCH(k_cov_lauum, dim3(it + 1), dim3(256), 0, h->stream, A.p, npad, it, D.p);
    BA_LAUNCH(k_cov_lauum_copy, dim3(1), dim3(256), 0, h->stream, A.p, npad, it, (const double*)D.p);
  }
  if (any_held) BA_LAUNCH(k_cov_held, dim3(1, n), dim3(256), 0, h->stream, cam_held_ptr(h), h->fixed, NB, n, npad, 0.0, A.p);
  if (pt_cov && Np) {
    HIPCHECK(ptc.alloc(6 * (size_t)Np));
    BA_LAUNCH(k_cov_point_cov<NB>, dim3((Np + 3) / 4), dim3(256), 0, h->stream, (const double*)A.p, npad, h->pt_off.p, h->p_cam.p,
              status.p, Vinv.p, Wbuf.p, Np, ptc.p);
    HIPCHECK(h->rbuf.alloc(6 * (size_t)Np));
    BA_LAUNCH(k_unpermute_rows, dim3((Np + 255) / 256), dim3(256), 0, h->stream, ptc.p, h->slot.p, Np, 6, h->rbuf.p);
  }
  if (cam_cov) {
    HIPCHECK(blk.alloc((size_t)NH * Nc));
    BA_LAUNCH(k_cov_cam_blocks<NB>, dim3((NH * Nc + 255) / 256), dim3(256), 0, h->stream, (const double*)A.p, npad, Nc, blk.p);
  }
  if (cam_full) BA_LAUNCH(k_cov_symmetrize, dim3(1, n), dim3(256), 0, h->stream, A.p, npad, n);
  int fw[2] = {COV_FAIL_NONE, COV_FAIL_NONE};
  HIPCHECK(hipMemcpyAsync(fw, failw.p, sizeof fw, hipMemcpyDeviceToHost, h->stream));
  BA_SYNC(h);
  if (fw[1] >= 0 && fw[1] < Np)
    return fail(BA_ERR_NUMERIC, "ba_covariance: point %d is not determined by its observations (3x3 block fails the rank test at "
                "rcond %g: zero parallax?); hold it or remove it", fw[1], rcond);
  if (fw[0] >= 0 && fw[0] < n)
    return fail(BA_ERR_NUMERIC, "ba_covariance: the reduced camera matrix is singular at camera %d, parameter %s (Cholesky pivot "
                "fails the rank test at rcond %g): the gauge must be fixed -- 6 pose dof + scale for the pinhole with fixed_cam "
                "(hold one more coordinate), 7 dof for a BAL problem with nothing held", fw[0] / NB, cov_param_name(fw[0] % NB), rcond);
  if (cam_cov) HIPCHECK(hipMemcpyAsync(cam_cov, blk.p, (size_t)NH * Nc * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (pt_cov && Np) HIPCHECK(hipMemcpyAsync(pt_cov, h->rbuf.p, 6 * (size_t)Np * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (cam_full)
    HIPCHECK(hipMemcpy2DAsync(cam_full, (size_t)n * sizeof(double), A.p, (size_t)npad * sizeof(double), (size_t)n * sizeof(double), n,
                              hipMemcpyDeviceToHost, h->stream));
  BA_SYNC(h);
  return BA_OK;
}
extern "C" int ba_covariance(ba_handle* h, const double* intr, int32_t loss, double f_scale, double rcond, double* cam_cov,
                             double* pt_cov, double* cam_full) {
  if (!h) return fail(BA_ERR_INVALID, "null handle");
  if (int rc = check_eval(h, loss, f_scale, intr ? 0 : CK_BAL_BITS)) return rc;
  if (h->multi) return fail(BA_ERR_INVALID, "ba_covariance: multi-rank jobs are not supported");
  if (h->n_shared)
    return fail(BA_ERR_INVALID, "ba_covariance: covariances of shared intrinsics are not offered (camera %d shares its f, k1, k2; "
                "clear the groups with ba_set_shared_intrinsics(h, NULL))", h->h_grp_mem[0]);
  const long long n = (long long)kModel[intr ? 1 : 0].nb * h->Nc;
  if (n > COV_MAX_N) return fail(BA_ERR_INVALID, "ba_covariance: %lld camera parameters, more than the %d the dense inverse takes", n, COV_MAX_N);
  if (!(rcond > 0)) rcond = COV_RCOND_DEFAULT;
  if (set_device(h)) return BA_ERR_HIP;
  return with_model(h, intr, [&]() -> int {
    int rc = BA_OK;
    BA_BY_MODEL(h->model, rc = cov_impl<CM>(h, (ba_loss)loss, f_scale, rcond, cam_cov, pt_cov, cam_full));
    return rc;
  });
}

static int solve_impl(ba_handle* h, const ba_options* opts, ba_summary* sum);
extern "C" int ba_solve_bal(ba_handle* h, double* intr, const ba_options* opts, ba_summary* sum) {
  if (!h || !intr || !opts || !sum) return fail(BA_ERR_INVALID, "null argument");
  if (!h->have_params) return fail(BA_ERR_STATE, "ba_set_problem / ba_set_params first");
  if (set_device(h)) return BA_ERR_HIP;
  // shared intrinsics: the members start from ONE f, k1, k2, hold the same of them, and none is the fixed camera
  for (int g = 0; g < h->n_shared; ++g) {
    const int lead = h->h_grp_mem[(size_t)h->h_grp_off[g]];
    for (int i = h->h_grp_off[g]; i < h->h_grp_off[g + 1]; ++i) {
      const int c = h->h_grp_mem[(size_t)i];
      if (c == h->fixed)
        return fail(BA_ERR_INVALID, "ba_solve_bal: camera %d is fixed_cam and shares its intrinsics with camera %d: fixed_cam holds the "
                    "whole 9-parameter block; hold the camera's pose with ba_set_held bits 0-5 instead", c, c == lead ? h->h_grp_mem[(size_t)h->h_grp_off[g] + 1] : lead);
      if (memcmp(intr + 3 * (size_t)c, intr + 3 * (size_t)lead, 3 * sizeof(double)) != 0)
        return fail(BA_ERR_INVALID, "ba_solve_bal: camera %d does not start with the f, k1, k2 of camera %d, whose intrinsics it shares", c, lead);
      const unsigned hc = h->any_cam_held ? (h->h_cam_held[(size_t)c] & 0x1c0u) : 0u, hl = h->any_cam_held ? (h->h_cam_held[(size_t)lead] & 0x1c0u) : 0u;
      if (hc != hl)
        return fail(BA_ERR_INVALID, "ba_solve_bal: camera %d holds other intrinsics (mask bits 6-8: 0x%x) than camera %d (0x%x), whose intrinsics it shares", c, hc, lead, hl);
    }
  }
  return with_model(h, intr, [&]() -> int {
    int rc = ba_solve(h, opts, sum);          // (ba_solve drains the stream and clears the per-solve modes on failure)
    // the adjusted (f, k1, k2) of the accepted parameter set -- also after a failed solve: the last accepted step stands
    // (k_cam_update writes parameters and camera state for the TRIAL set; the current set is always complete)
    if (hipMemcpyAsync(intr, h->intr[h->cur].p, 3 * (size_t)h->Nc * sizeof(double), hipMemcpyDeviceToHost, h->stream) != hipSuccess && rc == BA_OK)
      rc = fail(BA_ERR_HIP, "copying the intrinsics back failed");
    return rc;
  });
}

static int64_t held_params(const ba_handle* h, int nb) {       // held scalar parameters, the fixed camera's whole block included
  const unsigned full = (1u << nb) - 1;
  int64_t n = 0;
  for (int c = 0; c < h->Nc; ++c) {
    const unsigned m = ((h->any_cam_held ? h->h_cam_held[c] : 0u) | (c == h->fixed ? full : 0u)) & full;
    n += __builtin_popcount(m);
  }
  if (h->any_pt_held)
    for (int p = 0; p < h->Np; ++p) n += 3 * h->h_pt_held[p];
  return n;
}
static bool all_held(const ba_handle* h) {
  const int nb = nb_of(h);
  return held_params(h, nb) == (int64_t)nb * h->Nc + 3 * (int64_t)h->Np;
}
// The LM driver.  solve_impl is the skeleton; what is fixed for one solve sits in SolvePlan, what the iterations change in
// LmState and PrecondLag, and the stages of one iteration are functions of their own: linearize, run_pcg (the inner solve),
// queue_step_and_verdict (everything queued behind it) and apply_verdict (the host's half of accepting or rejecting the step).
static int check_solve_options(const ba_handle* h, const ba_options* opts) {
  if (!h->have_params) return fail(BA_ERR_STATE, "ba_set_problem / ba_set_params first");
  if (!loss_valid(opts->loss)) return fail(BA_ERR_INVALID, "unknown loss %d", opts->loss);
  if (!(opts->f_scale > 0) || opts->max_iters < 0 || opts->pcg_max_iters < 1 || !(opts->initial_lambda > 0))
    return fail(BA_ERR_INVALID, "bad options");
  if (opts->jacobian_precision != 0 && opts->jacobian_precision != 1)
    return fail(BA_ERR_INVALID, "jacobian_precision must be 0 (f64) or 1 (f32 blocks, f64 accumulation)");
  if (opts->preconditioner < BA_PRECOND_JACOBI || opts->preconditioner > BA_PRECOND_SCHUR_JACOBI) return fail(BA_ERR_INVALID, "unknown preconditioner");
  if (!(opts->pcg_model_tol >= 0.0 || opts->pcg_model_tol == -1.0) || opts->pcg_model_min_iters < 0)
    return fail(BA_ERR_INVALID, "bad pcg_model_tol (>= 0, or -1 = automatic) / pcg_model_min_iters");
  if (opts->precond_lag < 0) return fail(BA_ERR_INVALID, "precond_lag must not be negative");
  if (h->model == 0 && (h->cam_held_or & ~0x3fu))
    return fail(BA_ERR_INVALID, "camera mask bits 6-8 (f, k1, k2) need the BAL camera model");
  if (h->model == 0 && h->prior_nb == 9) return fail(BA_ERR_INVALID, "%s", kPriorNeedsBal);
  if (h->model == 0 && h->n_shared) return fail(BA_ERR_INVALID, "%s", kSharedNeedsBal);
  return BA_OK;
}
struct SolvePlan {               // fixed for one solve: read from the options, the environment and the handle once
  const ba_options* opts;
  ba_loss loss;
  bool robust, schur_diag;       // (robust: the Schur passes only read the weights -- the same for every non-linear loss)
  double fs, tol2, model_tol;
  int lag, riders;               // precond_lag, 0 where there are no Schur-Jacobi blocks to keep; BA_RIDERS
  bool debug_poison, use_ipc;    // (debug_poison, tests: every trial cost comes out NaN)
};
static SolvePlan solve_plan(const ba_handle* h, const ba_options* opts) {
  SolvePlan P;
  P.opts = opts;
  P.loss = (ba_loss)opts->loss; P.robust = P.loss != BA_LOSS_LINEAR; P.fs = opts->f_scale;
  P.schur_diag = opts->preconditioner != BA_PRECOND_JACOBI; P.lag = P.schur_diag ? opts->precond_lag : 0;
  P.tol2 = opts->pcg_tol * opts->pcg_tol;
  // (automatic: the model test trades inner accuracy for outer iterations -- on band-structured problems a large gain at
  // loose outer tolerances like the reference's ftol = 1e-5, a loss where the caller asks for tight convergence)
  P.model_tol = opts->pcg_model_tol >= 0.0 ? opts->pcg_model_tol : ((h->banded && opts->ftol >= 1e-6) ? 0.5 : 0.0);
  // BA_RIDERS: bit 0 = the camera update rides along the back substitution, bit 1 = the scalar fold + verdict rides along
  // the speculated point half (ba_kernels.hpp, "riders"), bit 2 = the PCG probe that finds PCG finished goes on as the back
  // substitution in the same launch (needs bit 0); BA_RIDERS=0: launches of their own (tests)
  P.riders = getenv("BA_RIDERS") ? atoi(getenv("BA_RIDERS")) : 7;
  P.debug_poison = getenv("BA_DEBUG_POISON_TRIAL") != nullptr;
  // BA_IPC: the exchange of the Schur product happens inside k_pcg_step, workgroup by workgroup (ba_kernels.hpp,
  // "device-side all-reduce"); every workgroup's record has to fit its slot of the receive buffers
  // (shared intrinsics: the group fold runs on the all-reduced product, between the exchange and k_pcg_step -- base transport)
  P.use_ipc = h->ipc && h->multi && !h->shared_on && nbv(h) <= IPC_MAX_BLOCKS &&
              (size_t)nbv(h) * (2 + (size_t)nb_of(h) * kModel[h->model].vc) <= IpcComm::STRIDE;
  return P;
}
struct LmState {                 // what the LM iterations change
  double lambda, nu = 2.0, lam_floor = 0.0, cost = 0.0, sse = 0.0;
  int it = 0, status = 0;
  bool stop = false;
  explicit LmState(double lambda0) : lambda(lambda0) {}
  bool need_linearize = true;    // a linearisation at the current parameters is needed before the next damped system
  bool have_lin = false;         // ... and buffer sets [lb] / [pb] already hold it (speculated at the trial point that was accepted)
};
// Schur-Jacobi blocks kept over consecutive damped systems (ba_options.precond_lag): when they were built, how often they
// have been kept since, and what the inner solves cost with them.  Host-side and deterministic: the rule reads options,
// dampings and PCG iteration counts only (identical on every rank of a multi-rank job).
struct PrecondLag {
  int lag, kept = 0, pcg_at_build = -1, pcg_last = -1;
  bool have = false;
  double lam_built = 0.0, last_decrease = 1.0;      // (last_decrease: relative cost decrease of the last accepted step)
  explicit PrecondLag(int lag_) : lag(lag_) {}
  // (!fresh: the same linearisation damped again after a rejected step; else the point the blocks were built at has moved by
  // a step that lowered the cost by no more than 1 % -- early, large steps always rebuild: there a stale preconditioner
  // costs more PCG iterations, at three passes each, than the one 27-sum pass it saves)
  bool keep(double lambda, bool fresh) const {
    return lag > 0 && have && kept < lag && lambda <= 10.0 * lam_built && lambda >= 0.1 * lam_built &&
           (pcg_at_build < 0 || pcg_last <= pcg_at_build + pcg_at_build / 2 + 2) && (!fresh || last_decrease <= 1e-2);
  }
  void built(double lambda) { have = true; lam_built = lambda; kept = 0; pcg_at_build = -1; }
  void kept_once() { ++kept; }
  void inner_solve_done(int n) { pcg_last = n; if (pcg_at_build < 0) pcg_at_build = n; }      // (< 0: the first with freshly built blocks)
  void accepted(double rel_decrease) { last_decrease = rel_decrease; }
};
static int initial_cost(ba_handle* h, const SolvePlan& P, LmState* st, ba_summary* sum) {
  if (int rc = eval_cost(h, h->cur, P.loss, P.fs, &st->sse, &st->cost)) return rc;
  sum->initial_sse = st->sse; sum->initial_cost = st->cost;
  return BA_OK;
}
static int finish_solve(ba_summary* sum, const LmState& st, double t_begin) {      // every successful way out of solve_impl
  sum->seconds_total = now_s() - t_begin;
  sum->iterations = st.it; sum->status = st.status;
  sum->final_sse = st.sse; sum->final_cost = st.cost; sum->final_lambda = st.lambda;
  return BA_OK;
}
// the held parameters' share of |x|^2 (xtol test): the held points' over every shard of a multi-rank job, the held camera
// parameters' read from the current cameras (the camera update adds their zero step and keeps their share in its sum)
static int held_norms(ba_handle* h, double* held_x2, double* held_cam_x2) {
  *held_x2 = h->held_x2;
  *held_cam_x2 = 0.0;
  if (h->any_cam_held) {
    const int nb = nb_of(h), Nc = h->Nc;
    std::vector<double> cams(6 * (size_t)Nc), intr(nb > 6 ? 3 * (size_t)Nc : 0);
    HIPCHECK(hipMemcpyAsync(cams.data(), h->cams[h->cur].p, cams.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (nb > 6) HIPCHECK(hipMemcpyAsync(intr.data(), h->intr[h->cur].p, intr.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    BA_SYNC(h);
    for (int c = 0; c < Nc; ++c)
      for (int q = 0; q < nb; ++q)
        if (((h->h_cam_held[c] >> q) & 1u) && !(q >= 6 && h->shared_on && h->h_cam_gl[c] >= 0 && !(h->h_cam_gl[c] & 1))) {   // (a shared entry once)
          const double v = q < 6 ? cams[6 * (size_t)c + q] : intr[3 * (size_t)c + q - 6];
          *held_cam_x2 += v * v;
        }
  }
  if (h->multi) {
    HIPCHECK(h->held_red.alloc(1));
    HIPCHECK(hipMemcpyAsync(h->held_red.p, held_x2, sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (int rc = allreduce(h, h->held_red.p, 1)) return rc;
    HIPCHECK(hipMemcpyAsync(held_x2, h->held_red.p, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    BA_SYNC(h);
  }
  return BA_OK;
}
static int linearize(ba_handle* h, const SolvePlan& P, LmState* st) {
  Range r_lin("linearize");
  if (!st->have_lin) {
    launch_lin_cam(h, h->cur, h->lb, P.loss, P.fs);
    launch_lin_pt(h, h->cur, h->pb, P.loss, P.fs, st->lambda);          // also Hpp^-1, y0 at this lambda
    // multi-rank: the camera-half partials of a pass launched here still have to be all-reduced
    // (a speculated pass was reduced right behind its launch)
    if (int rc = exchange_partL(h, h->lb)) return rc;
  }
  h->lin_loss = P.loss; h->lin_fscale = P.fs;
  st->need_linearize = false;
  st->have_lin = false;
  return BA_OK;
}
// K7a + K6 arguments.  The camera update does not feed the back substitution except through the step's vt, which the point
// workgroups drop into the rows of their LDS windows themselves (vx): it rides along the same launch as extra
// workgroups (ba_kernels.hpp, "riders") whenever every window is staged in LDS; else it is a launch of its own.
static CamUpdateArgs cam_update_args(ba_handle* h) {
  CamUpdateArgs cu;
  memset(&cu, 0, sizeof cu);
  cu.cams = h->cams[h->cur].p; cu.intr = h->intr[h->cur].p; cu.dc = h->x.p; cu.rpcg = h->r.p; cu.Hcc = h->HccBc.p; cu.bc = bc_ptr(h);
  cu.cs = h->cs[h->cur].p; cu.cams_trial = h->cams[1 - h->cur].p; cu.intr_trial = h->intr[1 - h->cur].p; cu.cs_trial = h->cs[1 - h->cur].p;
  cu.vtil = h->camA[h->cur].p; cu.camA_trial = h->camA[1 - h->cur].p; cu.partC = h->partC.p;
  cu.vx = h->vx.p;
  cu.cam_gl = cam_gl_ptr(h);
  cu.lam_slot = h->dev_lam.p;
  // (riding workgroups: a multiple of NPART, so that the point workgroups behind them keep their XCD = index mod NPART)
  cu.n_cams = h->Nc; cu.fixed_cam = h->fixed; cu.groups = CU_GROUPS;
  cu.n_blocks = (((nbv(h) + cu.groups - 1) / cu.groups + NPART - 1) / NPART) * NPART;
  return cu;
}
struct RiderPlan { bool ride, fuse; };        // of one LM iteration: the camera update rides / the finishing probe goes on as back substitution
static RiderPlan rider_plan(const ba_handle* h, const SolvePlan& P, const CamUpdateArgs& cu, int pcg_last) {
  RiderPlan rp;
  rp.ride = (P.riders & 1) && all_lds_of(h) && h->Np > 0;
  // The probe that finds PCG finished goes on as the back substitution (pt_schur_body, cu.fuse): the camera-update riders
  // then sit behind the point workgroups of EVERY PCG point pass (they only run in the launch that finds PCG finished), so
  // only where they do not add a round of workgroups to those launches -- a point-pass workgroup has a compute unit to
  // itself (config 5: 256 workgroups, one round; 16 more would be a second one in each of ~100 launches per LM iteration);
  // fp64 blocks only (the back substitution is never computed with the PCG passes' fp32 blocks).  Nothing in the launch
  // waits for a rider, so residency is a matter of speed, not of correctness.
  const int pt_wgs = h->nblkP + h->nblkL;
  // ... and where the inner solves are short: every PCG point pass carries the riders (0.6 us each at C3), the launch they
  // save comes once per LM iteration (5 - 8 us) -- beyond ~16 PCG iterations per LM iteration the separate launch is cheaper
  // (decided from the last inner solve's count: host-side, deterministic, identical on every rank; the bits do not depend on it)
  rp.fuse = rp.ride && (P.riders & 4) && !h->jac_f32 && (pcg_last < 0 || pcg_last <= 16) &&
            (pt_wgs + cu.n_blocks + h->n_cu - 1) / h->n_cu == (pt_wgs + h->n_cu - 1) / h->n_cu;
  return rp;
}
// the vector kernel of PCG iteration kk (behind the shared intrinsics' group fold, where there is one)
static void launch_pcg_step(ba_handle* h, const SolvePlan& P, int kk, long long base, const IpcStep& ipc) {
  Scope sc(h, BA_K_PCG_UPDATE);
  // (device-side exchange: k_cam_schur's raw partitions, folded inside the kernel; else partition 0 holds the all-reduced sums)
  const int step_parts = P.use_ipc ? NPART : nparts_of(h);
  if (h->shared_on)                 // rows 6-8 of w summed over the members, a workgroup per chunk of a group
    BA_LAUNCH(k_shared_fold<BalCam>, dim3(h->n_shared_chunks), dim3(SHARED_BLOCK), 0, h->stream, (const int*)h->chunk_rng.p, (const int*)h->grp_mem.p,
              (const double*)h->Hccd.p, (const double*)h->z.p, (const double*)p6_ptr(h), step_parts, h->Nc, h->grp_w.p);
#define STEP_ARGS kk, (const double*)p6_ptr(h), step_parts, (const double*)uy_ptr(h), h->Hccd.p, h->Minv.p, h->cs[h->cur].p, h->Nc, h->fixed, P.tol2,  \
                  P.opts->pcg_min_iters, h->x.p, h->r.p, h->p.p, h->s.p, h->z.p, h->camA[h->cur].p, h->partV.p, nbv(h), h->st.p, \
                  h->d_flags, base, (const double*)h->verdict.p, h->vx.p, P.model_tol, P.opts->pcg_model_min_iters, ipc, h->d_flags + 6,    \
                  cam_held_ptr(h), cam_gl_ptr(h), (const double*)(h->shared_on ? h->grp_w.p : nullptr),                                 \
                  (const int*)(h->shared_on ? h->grp_chunk.p : nullptr)
  if (h->shared_on) BA_LAUNCH((k_pcg_step<BalCam, true>), dim3(nbv(h)), dim3(VEC_BLOCK), 0, h->stream, STEP_ARGS);
  else BA_BY_MODEL(h->model, BA_LAUNCH((k_pcg_step<CM>), dim3(nbv(h)), dim3(VEC_BLOCK), 0, h->stream, STEP_ARGS));
#undef STEP_ARGS
}
// ---- PCG.  The point pass of iteration k is the probe: it publishes the verdict for k (go on /
// converged after n iterations) in host-mapped memory when it STARTS.  Only after a "go on" are
// the camera pass and the vector kernel of k queued (the point pass is still running then),
// followed at once by the probe of k+1.  Convergence costs one early-exit point pass.  The rule
// only depends on the (deterministic, rank-identical) verdicts, never on timing.
struct PcgOutcome {
  int k = 0;                     // iterations queued
  int done_iters = -1;           // ... and the count a probe reported, where one found PCG finished
  bool gtol_stop = false, backsub_done = false;
};
// gtol_pending (single rank): max |gradient| lands in host-mapped memory, read at the first PCG verdict
static int run_pcg(ba_handle* h, const SolvePlan& P, const RiderPlan& rp, CamUpdateArgs& cu, bool gtol_pending, int it, PcgOutcome* out) {
  const ba_options* opts = P.opts;
  Range r_pcg("pcg");
  const long long base = h->flag_base;
  h->flag_base += opts->pcg_max_iters + 8;
  int& k = out->k;
  while (true) {
    const size_t probe_ev = h->ev_slot.size(), probe_flushes = h->n_flushes;
    launch_pt_schur(h, P.robust, 0, k, P.tol2, opts->pcg_min_iters, base,
                    (k == 0 && gtol_pending) ? h->d_scal_host + GMAX_HOST_SLOT : (double*)nullptr, rp.fuse ? &cu : nullptr, h->jac_f32);
    if (int rc = wait_flag(h, 0, base + k + 1)) return rc;
    if (h->h_flags[6] == 2) { h->h_flags[6] = 0; return fail(BA_ERR_COMM, "LM iteration %d: a peer's share of the reduced camera system's product did not arrive (BA_IPC)", it); }
    // the gradient maximum was written by a kernel ahead of this probe: visible now
    if (gtol_pending) {
      gtol_pending = false;
      const double gmax = h->h_scal[GMAX_HOST_SLOT];
      if (!std::isfinite(gmax)) return fail(BA_ERR_NUMERIC, "non-finite gradient at LM iteration %d", it);
      if (gmax <= opts->gtol) { out->gtol_stop = true; break; }
    }
    const long long payload = h->h_flags[1];
    if (payload > 0) {
      out->done_iters = (int)payload - 1;
      if (rp.fuse) {                // the launch that published this verdict is doing the back substitution
        out->backsub_done = true;
        if (h->profile && probe_flushes == h->n_flushes && probe_ev < h->ev_slot.size()) h->ev_slot[probe_ev] = BA_K_SCHUR_PT_BACKSUB;
      }
      break;
    }
    launch_cam_schur(h, P.robust, false, true, k);
    // the Schur product of the reduced camera system, summed over the ranks: device-side stores into every peer's receive
    // buffer (inside k_pcg_step), or fold + all-reduce on the base transport
    IpcStep ipc;
    memset(&ipc, 0, sizeof ipc);
    if (P.use_ipc) {
      IpcComm* c = h->ipc;
      ipc.P = c->peers; ipc.on = 1; ipc.rank = c->rank; ipc.world = c->world;
      ipc.seq = ++c->seq;
      ipc.parity = (int)(ipc.seq & 1);
      ipc.stride = IpcComm::STRIDE;
      h->stats[BA_STAT_IPC_EXCHANGES]++;
    } else if (int rc = exchange_schur(h)) return rc;
    launch_pcg_step(h, P, k, base, ipc);
    if (++k >= opts->pcg_max_iters) break;
  }
  return BA_OK;
}
// ---- step, trial point, gain-ratio scalars: everything that is queued between the inner solve and the host's wait for the
// step's verdict (flag 2 reaching h->step_seq).  Speculation: unless this is the last iteration, the cost at the trial point
// comes out of the camera half of the NEXT linearisation computed there (one pass instead of two), into the other c_w / partL
// buffers; the step's verdict (gain ratio, next damping) is computed on the device right behind it, and while the host reads
// it the GPU already runs the point half at the trial point with that damping, into the other point buffers.  An accepted
// step finds its linearisation done; a rejected one ignores both.
static int queue_step_and_verdict(ba_handle* h, const SolvePlan& P, const RiderPlan& rp, CamUpdateArgs& cu, const PcgOutcome& pcg,
                                  const LmState& st, bool speculated) {
  const ba_options* opts = P.opts;
  if (!pcg.backsub_done) {          // (PCG ran into its iteration cap, or the fused form is off)
    cu.fuse = 0;
    if (!rp.ride) {
      Scope sc(h, BA_K_MISC);
      BA_BY_MODEL(h->model, BA_LAUNCH(k_cam_update<CM>, dim3(nbv(h)), dim3(VEC_BLOCK), 0, h->stream, cu));
      cu.n_blocks = 0;              // (the arguments still travel: the launch clears the riding verdict's damping word)
    }
    launch_pt_schur(h, P.robust, 1, 0, 0.0, 0, 0, nullptr, &cu);
  }
  if (speculated) launch_lin_cam(h, 1 - h->cur, 1 - h->lb, P.loss, P.fs, true);
  else            launch_residual(h, 1 - h->cur, P.loss, P.fs, nullptr);
  launch_prior_cost(h, 1 - h->cur);          // (priors set: their terms at the trial point, behind the reprojection rows)
  if (P.debug_poison) BA_LAUNCH(k_poison, dim3(1), dim3(64), 0, h->stream, h->partR.p);
  const long long seq = ++h->step_seq;
  // the step's scalar fold + verdict: single rank with a speculated point half behind it -> workgroup 0 of that launch
  // (the point workgroups pick the next damping up through a device word); else a launch of its own
  const bool ride_scalars = (P.riders & 2) && speculated && !h->multi && h->Np > 0;
  if (!ride_scalars) launch_scalars(h, true, pcg.k, P.tol2, opts->pcg_min_iters, seq, st.cost, st.lambda, st.lam_floor);
  if (h->multi) {
    // the six sums over ranks, then the verdict on the all-reduced block (same host-mapped mirror + word).  A speculated
    // camera half has to be all-reduced anyway: the six words travel in the header of that message, one collective
    const double* reduced6 = nullptr;
    if (speculated) {
      if (int rc = exchange_partL(h, 1 - h->lb, true)) return rc;
      reduced6 = h->linmsg[1 - h->lb].p;
    } else if (int rc = allreduce(h, h->scal.p, 6)) return rc;
    Scope sc(h, BA_K_MISC);
    BA_LAUNCH(k_decide, dim3(1), dim3(64), 0, h->stream, h->scal.p, reduced6, st.cost, st.lambda, st.lam_floor, h->d_scal_host, h->d_flags + 2, seq);
  }
  if (speculated) {
    ScalarsArgs sa = scalars_args(h, true, pcg.k, P.tol2, opts->pcg_min_iters, seq, st.cost, st.lambda, st.lam_floor);
    sa.on = 1; sa.lam_slot = h->dev_lam.p; sa.err_flag = h->d_flags + 6;
    launch_lin_pt(h, 1 - h->cur, 1 - h->pb, P.loss, P.fs, 0.0, h->scal.p + S_LAM_NEXT, ride_scalars ? &sa : nullptr);
  }
  return BA_OK;
}
// The host's half of the verdict, pure host code: the scalars of the step are in h->h_scal (gain ratio and next damping were
// decided on the device, lm_decide).  Records the iteration, accepts or rejects the step, tests ftol and xtol.
static int apply_verdict(ba_handle* h, const SolvePlan& P, LmState* st, PrecondLag* lag, ba_summary* sum, int pcg_done_iters,
                         bool speculated, double held_x2, double held_cam_x2, double t0) {
  const ba_options* opts = P.opts;
  const double* S = h->h_scal;
  const double sse_new = S[S_SSE], cost_new = 0.5 * S[S_RHO];
  const double step2 = S[S_PT_DD] + S[S_CAM_DD];
  const double x2 = (held_x2 != 0.0 || held_cam_x2 != 0.0)
                        ? std::max(0.0, S[S_PT_XX] - held_x2) + std::max(0.0, S[S_CAM_XX] - held_cam_x2)
                        : S[S_PT_XX] + S[S_CAM_XX];
  const double rho = S[S_GAIN];
  const bool accept = rho > 0 && std::isfinite(cost_new);
  const int it = ++st->it;
  if (opts->verbose)
    fprintf(stderr, "[ba] it %3d cost %.9e -> %.9e lambda %.3e rho %+.3f pcg %d |step| %.3e\n", it, st->cost, cost_new,
            st->lambda, rho, pcg_done_iters, std::sqrt(step2));
  ba_iter_record rec = {};
  rec.iteration = it; rec.accepted = accept ? 1 : 0; rec.pcg_iterations = pcg_done_iters;
  rec.cost = st->cost; rec.cost_trial = cost_new; rec.sse_trial = sse_new; rec.lambda = st->lambda; rec.gain_ratio = rho;
  rec.step_norm = std::sqrt(step2); rec.seconds = now_s() - t0;
  h->trace.push_back(rec);
  if (accept) {
    const double dcost = st->cost - cost_new;
    lag->accepted(cost_new > 0.0 ? dcost / cost_new : 1.0);
    h->cur = 1 - h->cur;
    if (speculated) { h->lb = 1 - h->lb; h->pb = 1 - h->pb; st->have_lin = true; }
    st->cost = cost_new;
    st->sse = sse_new;
    sum->accepted++;
    st->lambda = S[S_LAM_NEXT];
    st->nu = 2.0;
    st->need_linearize = true;
    if (dcost <= opts->ftol * st->cost) { st->status = 1; st->stop = true; }
  } else {
    // a trial cost that is not finite even at the largest damping the loop allows cannot be stepped away from
    if (!std::isfinite(cost_new) && st->lambda >= 1e12)
      return fail(BA_ERR_NUMERIC, "non-finite cost at the trial point of LM iteration %d with the damping at its cap", it);
    st->lambda = std::min(st->lambda * st->nu, 1e12);
    st->nu *= 2.0;
  }
  if (!st->stop && std::sqrt(step2) <= opts->xtol * (opts->xtol + std::sqrt(x2))) { st->status = 2; st->stop = true; }
  return BA_OK;
}
static int solve_impl(ba_handle* h, const ba_options* opts, ba_summary* sum) {
  if (int rc = check_solve_options(h, opts)) return rc;
  if (set_device(h)) return BA_ERR_HIP;
  memset(sum, 0, sizeof *sum);
  h->trace.clear();
  // the per-solve modes: switched on here, switched off by ba_solve behind every exit of this function
  h->shared_on = h->model != 0 && h->n_shared > 0;
  h->fold_prior_rows = any_prior(h) ? PRIOR_ROWS : 0;      // cost = reprojection + priors in every fold of this solve
  h->profile = opts->profile != 0;
  h->jac_f32 = opts->jacobian_precision == 1;              // (read by the PCG passes only: the window solver has none)
  const SolvePlan P = solve_plan(h, opts);
  LmState st(opts->initial_lambda);
  double t_begin = now_s();
  // single rank, every parameter held: nothing to adjust
  if (!h->multi && all_held(h)) {
    if (int rc = initial_cost(h, P, &st, sum)) return rc;
    return finish_solve(sum, st, t_begin);
  }
  // window-sized problems: one launch, exact reduced solve -- no PCG, so preconditioner / jacobian_precision (validated
  // above) have nothing to act on
  if (h->model == 0 && small_applies(h, opts)) return small_solve(h, opts, sum);
  roctx_load();
  Range r_solve("ba_solve");
  BA_SYNC(h);
  t_begin = now_s();
  if (int rc = initial_cost(h, P, &st, sum)) return rc;
  if (!std::isfinite(st.cost)) return fail(BA_ERR_NUMERIC, "non-finite cost at the initial parameters");
  // nothing to adjust.  Single rank only: a rank of a multi-rank job whose landmark shard is empty still has to
  // join every collective of the loop below (with zero partials), or the other ranks wait for it forever.
  if (!h->multi && (h->Np == 0 || h->Nobs == 0)) return finish_solve(sum, st, t_begin);
  double held_x2 = 0.0, held_cam_x2 = 0.0;
  if (int rc = held_norms(h, &held_x2, &held_cam_x2)) return rc;
  PrecondLag lag(P.lag);
  h->linearized = false;

  while (st.it < opts->max_iters && !st.stop) {
    const double t0 = now_s();
    Range r_iter("lm_iteration");
    const bool fresh = st.need_linearize;
    if (fresh)
      if (int rc = linearize(h, P, &st)) return rc;
    // ---- damped system, right-hand side, preconditioner, first PCG vectors
    const bool keep = lag.keep(st.lambda, fresh);
    { Range r_damp("damped_system"); if (int rc = damped_system(h, st.lambda, P.schur_diag, !fresh, fresh, keep)) return rc; }
    if (keep) lag.kept_once();
    else lag.built(st.lambda);
    // max |gradient| = max(|bc|, |bp|): per-workgroup maxima come out of the point half (partG) and of
    // k_pcg_setup (partGc); single rank: the first PCG probe folds them into host-mapped memory
    // (multi-rank: bc is all-reduced, identical on every rank; bp is shard-local -- every rank's maximum came with the
    // damped system's message, exchange_system, and the probe folds those instead of partG)
    const bool gtol_pending = fresh && opts->gtol > 0;
    const double t1 = now_s();
    sum->seconds_linearize += t1 - t0;
    // ---- the inner solve
    CamUpdateArgs cu = cam_update_args(h);
    const RiderPlan rp = rider_plan(h, P, cu, lag.pcg_last);
    cu.fuse = rp.fuse ? 1 : 0;
    PcgOutcome pcg;
    if (int rc = run_pcg(h, P, rp, cu, gtol_pending, st.it, &pcg)) return rc;
    if (pcg.gtol_stop) { st.status = 3; break; }      // converged by gradient: no step (the queued probe exits on its own)
    // Cap-aware damping.  An inner solve that runs into pcg_max_iters says that at this damping the reduced system is
    // beyond what the preconditioned iteration resolves within its budget (long camera chains at small damping: the drift
    // modes; BASELINE config 5).  The step it leaves is still a descent step (truncated CG), but letting the damping fall
    // further only buys more capped solves: from here on the damping stays at or above three times the value that
    // hit the cap -- one Nielsen step back, where the solve still converged.  The floor travels with the step's verdict
    // (lm_decide): the speculated point half reads the next damping on the device.
    if (pcg.k >= opts->pcg_max_iters) { st.lam_floor = std::max(st.lam_floor, 3.0 * st.lambda); h->stats[BA_STAT_CAP_FLOOR_RAISES]++; }
    Range r_step("step");
    const bool speculated = st.it + 1 < opts->max_iters;      // the next linearisation is computed at the trial point
    if (int rc = queue_step_and_verdict(h, P, rp, cu, pcg, st, speculated)) return rc;
    if (int rc = wait_flag(h, 2, h->step_seq)) return rc;
    if (h->h_flags[6] != 0) {          // a point workgroup of the speculated pass waited RIDER_WAIT_TICKS for the riding verdict
      h->h_flags[6] = 0;
      return fail(BA_ERR_HIP, "LM iteration %d: the point workgroups of the speculated linearisation were not served by the riding scalar fold", st.it);
    }
    if (pcg.done_iters < 0) pcg.done_iters = (h->h_scal[S_PCG_FIN] != 0.0) ? (int)h->h_scal[S_PCG_ITERS] : pcg.k;
    sum->pcg_iterations += pcg.done_iters;
    lag.inner_solve_done(pcg.done_iters);
    const double t2 = now_s();
    sum->seconds_pcg += t2 - t1;
    if (int rc = apply_verdict(h, P, &st, &lag, sum, pcg.done_iters, speculated, held_x2, held_cam_x2, t0)) return rc;
    sum->seconds_update += now_s() - t2;
  }
  BA_SYNC(h);
  return finish_solve(sum, st, t_begin);
}

// ------------------------------------------------------------------ counters, test hooks
extern "C" int ba_get_stat(ba_handle* h, int32_t which, int64_t* value) {
  if (!h || !value || which < 0 || which >= BA_STAT_END) return fail(BA_ERR_INVALID, "bad argument");
  if (which == BA_STAT_PRIOR_BLOCKS) { *value = h->have_problem ? h->prior_blocks : 0; return BA_OK; }
  if (which == BA_STAT_SHARED_GROUPS) { *value = h->have_problem ? h->n_shared : 0; return BA_OK; }
  if (which == BA_STAT_SCRATCH_BYTES) { *value = (int64_t)h->scratch.bytes; return BA_OK; }
  if (which == BA_STAT_SCRATCH_ALLOCS) { *value = h->scratch.allocs; return BA_OK; }
  if (which == BA_STAT_HELD_PARAMS) {
    *value = h->have_problem ? held_params(h, (h->cam_held_or & ~0x3fu) ? BalCam::NB : Pinhole::NB) : 0;
    return BA_OK;
  }
  *value = which == BA_STAT_PIXELS_F32 ? (int64_t)(h->have_problem && h->uv_f32) : (int64_t)h->stats[which];
  return BA_OK;
}
// Test hook: every byte of the scratch arena set to `byte`, so a test sees whether a call reads what it did not write itself
extern "C" int ba_debug_scratch_fill(ba_handle* h, int32_t byte) {
  if (!h) return fail(BA_ERR_INVALID, "null handle");
  if (set_device(h)) return BA_ERR_HIP;
  BA_SYNC(h);
  for (const Scratch::Block& b : h->scratch.blocks) HIPCHECK(hipMemset(b.p, byte & 0xff, b.cap));
  HIPCHECK(hipStreamSynchronize(nullptr));       // (the fill is queued on the null stream, which the handle's stream does not wait for)
  return BA_OK;
}
// Test hook: the layout ba_set_problem built, copied to the host (tests compare the device build with the host build).
// which: 0 pt_off (Np+1 ints), 1 p_cam, 2 c_pt, 3 c_orig (Nobs ints each), 4 offk (Nc x 9 ints), 5 long_pts (n_long ints),
// 6 blk_win ((nblkP + nblkL) x 2 ints), 7 slot (Np ints), 8 scalars (16 ints: lanes, nblkP, ppb, nblkL, long_spb, long_thr,
// n_long, cam_band, banded, cam_segl, all_lds[0], all_lds[1], lds_bytes[0], lds_bytes[1], build path 0 host / 1 device, mw_ok),
// 9 p_uv, 10 c_uv (Nobs x 2 doubles each).  *n = elements (ints, or doubles for 9 / 10) written.
extern "C" int ba_debug_layout(ba_handle* h, int32_t which, void* out, int64_t capacity, int64_t* n) {
  if (!h || !out || !n) return fail(BA_ERR_INVALID, "null argument");
  if (!h->have_problem) return fail(BA_ERR_STATE, "ba_set_problem has not been called");
  if (set_device(h)) return BA_ERR_HIP;
  const void* src = nullptr;
  int64_t cnt = 0;
  size_t esz = sizeof(int);
  int sc[16];
  switch (which) {
    case 0: src = h->pt_off.p; cnt = h->Np + 1; break;
    case 1: src = h->p_cam.p; cnt = h->Nobs; break;
    case 2: src = h->c_pt.p; cnt = h->Nobs; break;
    case 3: src = h->c_orig.p; cnt = h->Nobs; break;
    case 4: src = h->offk.p; cnt = (int64_t)h->Nc * (NPART + 1); break;
    case 5: src = h->long_pts.p; cnt = h->n_long; break;
    case 6: src = h->blk_win.p; cnt = 2 * (int64_t)(h->nblkP + h->nblkL); break;
    case 7: src = h->slot.p; cnt = h->Np; break;
    case 8: {
      const int v[16] = {h->lanes, h->nblkP, h->ppb, h->nblkL, h->long_spb, h->long_thr, h->n_long, h->cam_band, (int)h->banded, h->cam_segl,
                         (int)h->all_lds_m[0], (int)h->all_lds_m[1], (int)h->lds_bytes_m[0], (int)h->lds_bytes_m[1], h->setup_path, (int)h->mw_ok};
      memcpy(sc, v, sizeof sc);
      if (capacity < 16) return fail(BA_ERR_INVALID, "capacity");
      memcpy(out, sc, sizeof sc); *n = 16; return BA_OK;
    }
    case 9: src = h->p_uv.p; cnt = 2 * (int64_t)h->Nobs; esz = sizeof(double); break;
    case 10: src = h->c_uv.p; cnt = 2 * (int64_t)h->Nobs; esz = sizeof(double); break;
    default: return fail(BA_ERR_INVALID, "unknown layout array %d", which);
  }
  if (capacity < cnt) return fail(BA_ERR_INVALID, "capacity %lld < %lld", (long long)capacity, (long long)cnt);
  if ((which == 9 || which == 10) && h->uv_f32) {          // float2 streams: widened here, the caller sees the doubles it gave
    std::vector<float> tmp((size_t)cnt);
    if (cnt > 0) HIPCHECK(hipMemcpyAsync(tmp.data(), src, (size_t)cnt * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    BA_SYNC(h);
    for (int64_t i = 0; i < cnt; ++i) ((double*)out)[i] = (double)tmp[i];
    *n = cnt;
    return BA_OK;
  }
  if (cnt > 0) HIPCHECK(hipMemcpyAsync(out, src, (size_t)cnt * esz, hipMemcpyDeviceToHost, h->stream));
  BA_SYNC(h);
  *n = cnt;
  return BA_OK;
}
// workgroups that hold their compute unit's LDS for a bounded time and do nothing (ba_debug_occupy)
__global__ void __launch_bounds__(256) k_debug_occupy(long long ticks, double* __restrict__ sink) {
  extern __shared__ __align__(16) double hog[];
  if (threadIdx.x == 0) hog[0] = (double)blockIdx.x;
  const long long t0 = (long long)wall_clock64();
  while ((long long)wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(127);
  if (threadIdx.x == 0 && sink && hog[0] < 0.0) sink[0] = hog[0];          // (keeps the LDS word alive; never true)
}
extern "C" int ba_debug_occupy(ba_handle* h, int32_t n_workgroups, int32_t lds_bytes, double milliseconds) {
  if (!h || n_workgroups < 1 || n_workgroups > 4096 || lds_bytes < 8 || lds_bytes > 160 * 1024 || !(milliseconds > 0) || milliseconds > 2000.0)
    return fail(BA_ERR_INVALID, "bad argument");
  if (set_device(h)) return BA_ERR_HIP;
  if (!h->stream2) HIPCHECK(hipStreamCreateWithFlags(&h->stream2, hipStreamNonBlocking));
  HIPCHECK(hipFuncSetAttribute((const void*)k_debug_occupy, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes));
  hipLaunchKernelGGL(k_debug_occupy, dim3(n_workgroups), dim3(256), (size_t)lds_bytes, h->stream2, (long long)(milliseconds * 1e5), (double*)nullptr);
  HIPCHECK(hipGetLastError());
  return BA_OK;
}

// --------------------------------------------------------- two-view triangulation (row f3)
extern "C" int ba_triangulate(ba_handle* h, const double K[9], const double R_rel[9], const double t_rel[3], int64_t n,
                              const double* pts1, const double* pts2, double* xyz, uint8_t* valid) {
  if (!h || !K || !R_rel || !t_rel || n < 0) return fail(BA_ERR_INVALID, "bad argument");
  if (n == 0) return BA_OK;
  if (!pts1 || !pts2 || !xyz || !valid) return fail(BA_ERR_INVALID, "null point arrays");
  if (set_device(h)) return BA_ERR_HIP;
  TriView v;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c) {
      v.P1[4 * r + c] = (c < 3) ? K[3 * r + c] : 0.0;                                   // K [I | 0]
      double s2 = 0.0;
      for (int k = 0; k < 3; ++k) s2 += K[3 * r + k] * ((c < 3) ? R_rel[3 * k + c] : t_rel[k]);
      v.P2[4 * r + c] = s2;                                                             // K [R | t]
    }
  memcpy(v.R, R_rel, sizeof v.R);
  memcpy(v.t, t_rel, sizeof v.t);
  // staging: 2n + 2n doubles in, 3n doubles + n bytes out, in the handle's scratch buffer
  const size_t words = 7 * (size_t)n + ((size_t)n + 7) / 8 + 8;
  HIPCHECK(h->tri.alloc(words));
  double* d1 = h->tri.p;
  double* d2 = d1 + 2 * (size_t)n;
  double* dx = d2 + 2 * (size_t)n;
  uint8_t* dv = (uint8_t*)(dx + 3 * (size_t)n);
  HIPCHECK(hipMemcpyAsync(d1, pts1, 2 * (size_t)n * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHECK(hipMemcpyAsync(d2, pts2, 2 * (size_t)n * sizeof(double), hipMemcpyHostToDevice, h->stream));
  BA_LAUNCH(k_triangulate, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, v, n, (const double2*)d1, (const double2*)d2, dx, dv);
  HIPCHECK(hipMemcpyAsync(xyz, dx, 3 * (size_t)n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(hipMemcpyAsync(valid, dv, (size_t)n, hipMemcpyDeviceToHost, h->stream));
  BA_SYNC(h);
  return BA_OK;
}

extern "C" int ba_get_trace(ba_handle* h, ba_iter_record* out, int32_t capacity, int32_t* n) {
  if (!h || !n || capacity < 0) return fail(BA_ERR_INVALID, "bad argument");
  *n = (int32_t)h->trace.size();
  if (out) memcpy(out, h->trace.data(), sizeof(ba_iter_record) * (size_t)std::min<int32_t>(capacity, *n));
  return BA_OK;
}

// The end of every write_* / apply: parameter set 0, which the caller has just filled (cameras rvec | t and the point table),
// becomes what ba_set_params would have left behind -- current, its camera state recomputed (prepared: already done, by
// k_sim_cam_prepare), the linearisation forgotten
static void adopt_set0(ba_handle* h, bool prepared = false) {
  h->cur = 0;
  if (!prepared)
    BA_LAUNCH(k_cam_prepare<Pinhole>, dim3((h->Nc + 63) / 64), dim3(64), 0, h->stream, h->cams[0].p, (const double*)h->intr[0].p,
              h->cs[0].p, h->camA[0].p, h->Nc);
  h->linearized = false;
}

// ------------------------------------------------------------------------------------------------- tracks
// ba_triangulate_tracks (csrc/ba_tracks.hpp): camera centres, the short-track launch over every point slot, the long-track
// launch over long_pts, results back in the caller's point order.  Local to the rank: no collective.
static void launch_tracks(ba_handle* h) {
  h->trk_args.cs = h->cs[h->cur].p;
  const TrackArgs& a = h->trk_args;
  BA_LAUNCH(k_track_centres, dim3((h->Nc + 255) / 256), dim3(256), 0, h->stream, a.cs, h->Nc, h->trk_ctr.p);
  if (h->Np == 0) return;
  const int tpb = TRK_THREADS / TRK_G;
  BA_BY_MODEL(h->trk_bal, BA_LAUNCH(k_tracks_short<CM>, dim3((h->Np + tpb - 1) / tpb), dim3(TRK_THREADS), 0, h->stream, a));
  if (h->n_long > 0) {
    TrackArgs b = a;
    b.list = h->long_pts.p; b.n_items = h->n_long;
    BA_BY_MODEL(h->trk_bal, BA_LAUNCH(k_tracks_long<CM>, dim3(h->n_long), dim3(64), 0, h->stream, b));
  }
}
extern "C" int ba_default_track_options(ba_track_options* o) {
  if (!o) return fail(BA_ERR_INVALID, "null argument");
  memset(o, 0, sizeof *o);
  o->loss = BA_LOSS_LINEAR;
  o->refine_iters = 20;
  o->f_scale = 1.0;
  return BA_OK;
}
extern "C" int ba_triangulate_tracks(ba_handle* h, const double* intr, const ba_track_options* opts, double* xyz, uint8_t* status,
                                     double* angle_deg, double* rms_px, double* max_px) {
  if (!h || !opts) return fail(BA_ERR_INVALID, "null argument");
  if (!h->have_problem || !h->have_params) return fail(BA_ERR_STATE, "ba_triangulate_tracks: ba_set_problem / ba_set_params first");
  if (!loss_valid(opts->loss)) return fail(BA_ERR_INVALID, "ba_triangulate_tracks: unknown loss %d", opts->loss);
  if (!(opts->f_scale > 0)) return fail(BA_ERR_INVALID, "ba_triangulate_tracks: f_scale must be positive");
  if (opts->refine_iters < 0) return fail(BA_ERR_INVALID, "ba_triangulate_tracks: refine_iters must not be negative");
  if (opts->reserved0 != 0) return fail(BA_ERR_INVALID, "ba_triangulate_tracks: reserved0 must be 0");
  if (set_device(h)) return BA_ERR_HIP;
  const int Nc = h->Nc, Np = h->Np;
  const size_t np1 = (size_t)std::max(Np, 1);
  HIPCHECK(h->trk_out.alloc(TRK_OUT * np1)); HIPCHECK(h->trk_ctr.alloc(4 * (size_t)Nc)); HIPCHECK(h->trk_res.alloc(6 * np1));
  HIPCHECK(h->trk_status.alloc(np1));
  if (intr) {
    HIPCHECK(h->trk_intr.alloc(3 * (size_t)Nc));
    HIPCHECK(hipMemcpyAsync(h->trk_intr.p, intr, 3 * (size_t)Nc * sizeof(double), hipMemcpyHostToDevice, h->stream));
  }
  TrackArgs& a = h->trk_args;
  a.cs = h->cs[h->cur].p; a.intr = intr ? h->trk_intr.p : nullptr; a.ctr = h->trk_ctr.p;
  a.pt_off = h->pt_off.p; a.p_cam = h->p_cam.p; a.uv = uv_arr(h, h->p_uv);
  a.list = nullptr; a.n_items = Np; a.thr = h->n_long > 0 ? h->long_thr : 0x7fffffff;
  a.fx = h->K4[0]; a.fy = h->K4[1]; a.cx = h->K4[2]; a.cy = h->K4[3];
  a.loss = opts->loss; a.iters = opts->refine_iters;
  a.fscale = opts->f_scale; a.min_angle = opts->min_angle_deg; a.max_px = opts->max_reproj_px; a.min_depth = opts->min_depth;
  a.out = h->trk_out.p;
  h->trk_bal = intr != nullptr;
  h->trk_valid = true;
  launch_tracks(h);
  if (Np > 0) {
    BA_LAUNCH(k_tracks_unpermute, dim3((Np + 255) / 256), dim3(256), 0, h->stream, (const double*)h->trk_out.p, (const int*)h->slot.p, Np,
              h->trk_res.p, h->trk_res.p + 3 * (size_t)Np, h->trk_status.p);
    if (xyz) HIPCHECK(hipMemcpyAsync(xyz, h->trk_res.p, 3 * (size_t)Np * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    double* const meas[3] = {angle_deg, rms_px, max_px};
    for (int q = 0; q < 3; ++q)
      if (meas[q]) HIPCHECK(hipMemcpyAsync(meas[q], h->trk_res.p + (3 + q) * (size_t)Np, (size_t)Np * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (status) HIPCHECK(hipMemcpyAsync(status, h->trk_status.p, (size_t)Np, hipMemcpyDeviceToHost, h->stream));
  }
  if (opts->write_points) {
    // what ba_set_params(cameras as they are, merged points) leaves behind: the point table rebuilt, then adopt_set0
    if (Np > 0)
      BA_LAUNCH(k_tracks_merge, dim3((Np + 255) / 256), dim3(256), 0, h->stream, (const double*)h->trk_out.p, pt_held_ptr(h),
                (const double*)h->ptab[h->cur].p, Np, h->ptab[0].p);
    if (h->cur != 0)
      HIPCHECK(hipMemcpyAsync(h->cams[0].p, h->cams[h->cur].p, 6 * (size_t)Nc * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    adopt_set0(h);
  }
  BA_SYNC(h);
  return BA_OK;
}

// ------------------------------------------------------------------------------------------------- resection
// ba_resect (csrc/ba_resect.hpp): one workgroup per camera over the camera-ordered list.  Local to the rank: no collective.
static void launch_resect(ba_handle* h) {
  ResectArgs& a = h->rs.args;
  a.t.cs = h->cs[h->cur].p; a.cams = h->cams[h->cur].p; a.ptab = h->ptab[h->cur].p;
  if (h->Nc == 0) return;
  BA_BY_MODEL(h->rs.bal, BA_LAUNCH(k_resect<CM>, dim3(h->Nc), dim3(RS_THREADS), 0, h->stream, a));
}
// What ba_resect and ba_resect_ransac (`who` in the messages) do alike before their launches: the checks of the options they
// share -- o is ba_resect's struct for both; ba_resect_ransac fills one from its own, init = CURRENT --, the uploads of intr,
// cam_sel and pt_known into the caller's set s, and its ResectArgs
static int resect_begin(ba_handle* h, const char* who, const double* intr, const uint8_t* cam_sel, const uint8_t* pt_known,
                        const ba_resect_options& o, ba_handle::ResectSet& s) {
  if (!loss_valid(o.loss)) return fail(BA_ERR_INVALID, "%s: unknown loss %d", who, o.loss);
  if (!(o.f_scale > 0)) return fail(BA_ERR_INVALID, "%s: f_scale must be positive", who);
  if (o.refine_iters < 0) return fail(BA_ERR_INVALID, "%s: refine_iters must not be negative", who);
  if (o.min_inliers < 0) return fail(BA_ERR_INVALID, "%s: min_inliers must not be negative", who);
  // the cameras of a multi-rank job are replicated and ba_solve relies on every rank holding the same bits: a pose
  // resected from this rank's shard alone would split them (a forced communicator of one rank has nobody to differ from)
  if (o.write_cams && h->world > 1)
    return fail(BA_ERR_INVALID, "%s: write_cams = 1 on a multi-rank handle (world %d): every rank would store poses from its own "
                                "shard's observations and the replicated cameras would differ; resect with write_cams = 0 and "
                                "hand every rank the same poses (ba_set_params)", who, h->world);
  if (o.write_cams && any_prior(h))
    return fail(BA_ERR_STATE, "%s with write_cams = 1: priors are set (ba_set_priors) and their means were set for the old poses: "
                              "resect first, set the priors afterwards", who);
  if (set_device(h)) return BA_ERR_HIP;
  const int Nc = h->Nc, Np = h->Np;
  const size_t nc1 = (size_t)std::max(Nc, 1), np1 = (size_t)std::max(Np, 1);
  HIPCHECK(s.out.alloc(RS_OUT * nc1));
  if (intr) {
    HIPCHECK(s.intr.alloc(3 * nc1));
    HIPCHECK(hipMemcpyAsync(s.intr.p, intr, 3 * (size_t)Nc * sizeof(double), hipMemcpyHostToDevice, h->stream));
  }
  if (cam_sel) {
    HIPCHECK(s.sel.alloc(nc1));
    HIPCHECK(hipMemcpyAsync(s.sel.p, cam_sel, (size_t)Nc, hipMemcpyHostToDevice, h->stream));
  }
  if (pt_known && Np > 0) {
    HIPCHECK(h->rs_known_in.alloc(np1)); HIPCHECK(s.known.alloc(np1));
    HIPCHECK(hipMemcpyAsync(h->rs_known_in.p, pt_known, (size_t)Np, hipMemcpyHostToDevice, h->stream));
    BA_LAUNCH(k_resect_known, dim3((Np + 255) / 256), dim3(256), 0, h->stream, (const unsigned char*)h->rs_known_in.p, (const int*)h->slot.p, Np,
              s.known.p);
  }
  ResectArgs& a = s.args;
  a = ResectArgs{};
  a.t.intr = intr ? s.intr.p : nullptr;
  a.t.uv = uv_arr(h, h->c_uv);
  a.t.fx = h->K4[0]; a.t.fy = h->K4[1]; a.t.cx = h->K4[2]; a.t.cy = h->K4[3];
  a.t.loss = o.loss; a.t.iters = o.refine_iters;
  a.t.fscale = o.f_scale; a.t.max_px = o.max_reproj_px; a.t.min_depth = o.min_depth;
  a.offk = h->offk.p; a.c_pt = h->c_pt.p;
  a.known = (pt_known && Np > 0) ? s.known.p : nullptr;
  a.sel = cam_sel ? s.sel.p : nullptr;
  a.init = o.init; a.min_inliers = o.min_inliers; a.max_rms = o.max_rms_px;
  a.out = s.out.p;
  s.bal = intr != nullptr;
  s.valid = true;
  return BA_OK;
}
// ... and behind them: the rows of s.out back, write_cams, the sync, the rows into the caller's arrays
static int resect_end(ba_handle* h, ba_handle::ResectSet& s, int write_cams, double* poses, uint8_t* status, int32_t* n_inliers,
                      double* rms_px, double* max_px) {
  const int Nc = h->Nc, Np = h->Np;
  std::vector<double> res(RS_OUT * (size_t)Nc);
  if (Nc > 0) HIPCHECK(hipMemcpyAsync(res.data(), s.out.p, res.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (write_cams) {
    // what ba_set_params(merged cameras, points as they are) leaves behind: the cameras merged and the point table rebuilt,
    // then adopt_set0 (held_x2 stays: no point moves)
    const int nmax = std::max(Nc, Np);
    if (nmax > 0)
      BA_LAUNCH(k_resect_merge, dim3((nmax + 255) / 256), dim3(256), 0, h->stream, (const double*)s.out.p, s.args.sel, cam_held_ptr(h), h->fixed,
                (const double*)h->cams[h->cur].p, Nc, h->cams[0].p, (const double*)h->ptab[h->cur].p, Np, h->ptab[0].p);
    adopt_set0(h);
  }
  BA_SYNC(h);
  for (int c = 0; c < Nc; ++c) {
    const double* r = res.data() + RS_OUT * (size_t)c;
    if (poses) memcpy(poses + 6 * (size_t)c, r, 6 * sizeof(double));
    if (status) status[c] = (uint8_t)(int)r[6];
    if (n_inliers) n_inliers[c] = (int32_t)r[7];
    if (rms_px) rms_px[c] = r[8];
    if (max_px) max_px[c] = r[9];
  }
  return BA_OK;
}
extern "C" int ba_default_resect_options(ba_resect_options* o) {
  if (!o) return fail(BA_ERR_INVALID, "null argument");
  memset(o, 0, sizeof *o);
  o->loss = BA_LOSS_LINEAR;
  o->refine_iters = 20;
  o->f_scale = 1.0;
  o->init = BA_RESECT_INIT_DLT;
  o->min_inliers = 6;
  return BA_OK;
}
extern "C" int ba_resect(ba_handle* h, const double* intr, const ba_resect_options* opts, const uint8_t* cam_sel, const uint8_t* pt_known,
                         double* poses, uint8_t* status, int32_t* n_inliers, double* rms_px, double* max_px) {
  if (!h || !opts) return fail(BA_ERR_INVALID, "null argument");
  if (!h->have_problem || !h->have_params) return fail(BA_ERR_STATE, "ba_resect: ba_set_problem / ba_set_params first");
  if (opts->init != BA_RESECT_INIT_DLT && opts->init != BA_RESECT_INIT_CURRENT) return fail(BA_ERR_INVALID, "ba_resect: unknown init %d", opts->init);
  if (opts->reserved0 != 0) return fail(BA_ERR_INVALID, "ba_resect: reserved0 must be 0");
  if (int rc = resect_begin(h, "ba_resect", intr, cam_sel, pt_known, *opts, h->rs)) return rc;
  launch_resect(h);
  return resect_end(h, h->rs, opts->write_cams, poses, status, n_inliers, rms_px, max_px);
}

// ------------------------------------------------------------------------------------------------- RANSAC resection
// ba_resect_ransac (csrc/ba_ransac.hpp): usable observations, hypotheses and scores, local optimisation.  Local to the rank.
static int launch_ransac(ba_handle* h) {
  RansacArgs& a = h->rn_args;
  a.r.t.cs = h->cs[h->cur].p; a.r.cams = h->cams[h->cur].p; a.r.ptab = h->ptab[h->cur].p;
  if (h->Nc == 0) return BA_OK;
  if (a.inl && h->Nobs > 0) HIPCHECK(hipMemsetAsync(a.inl, 0, (size_t)h->Nobs, h->stream));
  const dim3 gc(h->Nc), gs(h->Nc, a.n_blk), b(RN_THREADS);
  BA_BY_MODEL(h->rn.bal, BA_LAUNCH(k_ransac_prep<CM>, gc, b, 0, h->stream, a));
  BA_BY_MODEL(h->rn.bal, BA_LAUNCH(k_ransac_score<CM>, gs, b, 0, h->stream, a));
  BA_BY_MODEL(h->rn.bal, BA_LAUNCH(k_ransac_lo<CM>, gc, b, 0, h->stream, a));
  return BA_OK;
}
extern "C" int ba_default_ransac_options(ba_ransac_options* o) {
  if (!o) return fail(BA_ERR_INVALID, "null argument");
  memset(o, 0, sizeof *o);
  o->n_hyp = 256;
  o->lo_rounds = 2;
  o->max_reproj_px = 4.0;
  o->loss = BA_LOSS_LINEAR;
  o->refine_iters = 20;
  o->f_scale = 1.0;
  o->min_inliers = 6;
  return BA_OK;
}
extern "C" int ba_resect_ransac(ba_handle* h, const double* intr, const ba_ransac_options* opts, const uint8_t* cam_sel, const uint8_t* pt_known,
                                double* poses, uint8_t* status, int32_t* n_inliers, double* rms_px, double* max_px, uint8_t* obs_inlier) {
  if (!h || !opts) return fail(BA_ERR_INVALID, "null argument");
  if (!h->have_problem || !h->have_params) return fail(BA_ERR_STATE, "ba_resect_ransac: ba_set_problem / ba_set_params first");
  if (opts->n_hyp < 1 || opts->n_hyp > HY_MAX_HYP) return fail(BA_ERR_INVALID, "ba_resect_ransac: n_hyp %d is outside 1 .. %d", opts->n_hyp, HY_MAX_HYP);
  if (opts->lo_rounds < 0) return fail(BA_ERR_INVALID, "ba_resect_ransac: lo_rounds must not be negative");
  if (!(opts->max_reproj_px > 0)) return fail(BA_ERR_INVALID, "ba_resect_ransac: max_reproj_px must be positive");
  ba_resect_options common = {};
  common.loss = opts->loss; common.refine_iters = opts->refine_iters; common.f_scale = opts->f_scale;
  common.init = BA_RESECT_INIT_CURRENT; common.min_inliers = opts->min_inliers; common.write_cams = opts->write_cams;
  common.max_reproj_px = opts->max_reproj_px; common.max_rms_px = opts->max_rms_px; common.min_depth = opts->min_depth;
  if (int rc = resect_begin(h, "ba_resect_ransac", intr, cam_sel, pt_known, common, h->rn)) return rc;
  const size_t nc1 = (size_t)std::max(h->Nc, 1), no1 = (size_t)std::max<long long>(h->Nobs, 1);
  const int n_blk = (opts->n_hyp + RN_THREADS - 1) / RN_THREADS;
  HIPCHECK(h->rn_rec.alloc(RN_REC * no1)); HIPCHECK(h->rn_cnt.alloc(nc1)); HIPCHECK(h->rn_best.alloc(RN_BEST * nc1 * n_blk));
  HIPCHECK(h->rn_cons.alloc(no1)); HIPCHECK(h->rn_inl.alloc(no1));
  RansacArgs& a = h->rn_args;
  a = RansacArgs{};
  a.r = h->rn.args;
  a.n_hyp = opts->n_hyp; a.lo_rounds = opts->lo_rounds; a.n_blk = n_blk; a.seed = opts->seed;
  a.rec = h->rn_rec.p; a.cnt = h->rn_cnt.p; a.best = h->rn_best.p; a.cons = h->rn_cons.p;
  a.c_orig = h->c_orig.p; a.inl = h->rn_inl.p;
  if (int rc = launch_ransac(h)) return rc;
  if (obs_inlier && h->Nobs > 0) {
    if (h->Nc > 0) HIPCHECK(hipMemcpyAsync(obs_inlier, h->rn_inl.p, (size_t)h->Nobs, hipMemcpyDeviceToHost, h->stream));
    else memset(obs_inlier, 0, (size_t)h->Nobs);
  }
  return resect_end(h, h->rn, opts->write_cams, poses, status, n_inliers, rms_px, max_px);
}

// ------------------------------------------------------------------------------------------------- the pair-shaped calls' plumbing
// What ba_relative_pose, ba_homography, ba_sim3 and ba_fundamental refuse alike; `who` is the call the message names.  K null: the
// call has none.
static int pairs_check(const char* who, const double* K, int32_t n_pairs, const int64_t* pair_off, const double* pts1, const double* pts2,
                       int32_t n_hyp, int32_t lo_rounds, int32_t refine_iters, int32_t min_inliers) {
  if (n_pairs < 0 || n_pairs > 65535) return fail(BA_ERR_INVALID, "%s: n_pairs %d is outside 0 .. 65535", who, n_pairs);
  if (n_hyp < 1 || n_hyp > HY_MAX_HYP) return fail(BA_ERR_INVALID, "%s: n_hyp %d is outside 1 .. %d", who, n_hyp, HY_MAX_HYP);
  if (lo_rounds < 0) return fail(BA_ERR_INVALID, "%s: lo_rounds must not be negative", who);
  if (refine_iters < 0) return fail(BA_ERR_INVALID, "%s: refine_iters must not be negative", who);
  if (min_inliers < 0) return fail(BA_ERR_INVALID, "%s: min_inliers must not be negative", who);
  if (K && (!(K[0] > 0 && K[4] > 0 && std::isfinite(K[0]) && std::isfinite(K[4]) && std::isfinite(K[2]) && std::isfinite(K[5])) || K[1] != 0 ||
            K[3] != 0 || K[6] != 0 || K[7] != 0 || K[8] != 1))
    return fail(BA_ERR_INVALID, "%s: K must be the pinhole matrix [fx 0 cx; 0 fy cy; 0 0 1] with fx, fy > 0", who);
  if (n_pairs == 0) return BA_OK;
  if (!pair_off) return fail(BA_ERR_INVALID, "%s: null pair_off", who);
  if (pair_off[0] != 0) return fail(BA_ERR_INVALID, "%s: pair_off[0] must be 0", who);
  for (int32_t p = 0; p < n_pairs; ++p) {
    if (pair_off[p + 1] < pair_off[p]) return fail(BA_ERR_INVALID, "%s: pair_off decreases at pair %d", who, p);
    if (pair_off[p + 1] - pair_off[p] > 0x7fffffffLL) return fail(BA_ERR_INVALID, "%s: pair_off: pair %d has too many matches", who, p);
  }
  if (pair_off[n_pairs] > 0 && (!pts1 || !pts2)) return fail(BA_ERR_INVALID, "%s: null point arrays", who);
  return BA_OK;
}
// What the calls' options hold alike, each under its own names; max_px: the call's threshold in pixels
struct PairOpts { int32_t n_hyp, lo_rounds, refine_iters, min_inliers; uint64_t seed; double max_px; };
// A call (n_pairs > 0) begun: its arrays taken from the scratch arena and uploaded, and the shared head of its arguments.  K null:
// fbar = 1.  width: doubles per point (2, or ba_sim3's 3); best_per / out_per: the call's doubles per score block / per pair.
// d1 | d2: the two point arrays on the device.
static int pairs_upload(ba_handle* h, const double* K, int32_t n_pairs, const int64_t* pair_off, int width, const double* pts1,
                        const double* pts2, const PairOpts& o, int n_blk, int best_per, int out_per, HypArgs& a, const double*& d1,
                        const double*& d2) {
  if (set_device(h)) return BA_ERR_HIP;
  Scratch& sc = h->scratch;
  HIPCHECK(sc.begin(h->stream));
  const size_t nm = (size_t)pair_off[n_pairs], np = (size_t)n_pairs;
  static_assert(sizeof(long long) == sizeof(int64_t), "pair_off is uploaded as it is");
  HIPCHECK(sc.put(h->stream, width * nm, pts1, &d1)); HIPCHECK(sc.put(h->stream, width * nm, pts2, &d2)); HIPCHECK(sc.put(h->stream, np + 1, pair_off, &a.off));
  HIPCHECK(sc.take((size_t)best_per * np * n_blk, &a.best)); HIPCHECK(sc.take((size_t)out_per * np, &a.out)); HIPCHECK(sc.take(nm, &a.cons, &a.inl));
  a.fbar = K ? 0.5 * (K[0] + K[4]) : 1.0; a.thr = o.max_px / a.fbar;
  a.n_hyp = o.n_hyp; a.lo_rounds = o.lo_rounds; a.iters = o.refine_iters; a.min_inliers = o.min_inliers;
  a.n_blk = n_blk; a.seed = o.seed;
  if (nm > 0) HIPCHECK(hipMemsetAsync(a.inl, 0, nm, h->stream));
  return BA_OK;
}
// The same for the calls on pixels, with their K (null: fx = fy = 1, cx = cy = 0) and the two views; max_depth is the caller's
static int pairs_upload(ba_handle* h, const double* K, int32_t n_pairs, const int64_t* pair_off, const double* pts1, const double* pts2,
                        const PairOpts& o, int n_blk, int best_per, int out_per, PairArgs& a) {
  const double *d1, *d2;
  if (int rc = pairs_upload(h, K, n_pairs, pair_off, 2, pts1, pts2, o, n_blk, best_per, out_per, a, d1, d2)) return rc;
  a.fx = K ? K[0] : 1.0; a.fy = K ? K[4] : 1.0; a.cx = K ? K[2] : 0.0; a.cy = K ? K[5] : 0.0;
  a.p1 = (const double2*)d1; a.p2 = (const double2*)d2;
  return BA_OK;
}
// The pairs' rows of out_per doubles into res (want: the call returns any of them) and match_inlier, and the stream drained
static int pairs_download(ba_handle* h, const HypArgs& a, bool want, int out_per, int32_t n_pairs, const int64_t* pair_off,
                          uint8_t* match_inlier, std::vector<double>& res) {
  const size_t nm = (size_t)pair_off[n_pairs];
  res.resize(want ? (size_t)out_per * n_pairs : 0);
  if (want) HIPCHECK(hipMemcpyAsync(res.data(), a.out, res.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (match_inlier && nm > 0) HIPCHECK(hipMemcpyAsync(match_inlier, a.inl, nm, hipMemcpyDeviceToHost, h->stream));
  BA_SYNC(h);
  return BA_OK;
}

// ------------------------------------------------------------------------------------------------- two-view relative pose
// ba_relative_pose (csrc/ba_relpose.hpp): five-point hypotheses, scores, decomposition and local optimisation.  Needs no problem.
static_assert(RP_OK == BA_RELPOSE_OK && RP_FEW_MATCHES == BA_RELPOSE_FEW_MATCHES && RP_DEGENERATE == BA_RELPOSE_DEGENERATE &&
              RP_BEHIND == BA_RELPOSE_BEHIND && RP_FEW_INLIERS == BA_RELPOSE_FEW_INLIERS && RP_LOW_PARALLAX == BA_RELPOSE_LOW_PARALLAX &&
              sizeof(ba_relpose_options) == 48, "device status codes (ba_relpose.hpp)");
extern "C" int ba_default_relpose_options(ba_relpose_options* o) {
  if (!o) return fail(BA_ERR_INVALID, "null argument");
  memset(o, 0, sizeof *o);
  o->n_hyp = 256;
  o->lo_rounds = 2;
  o->max_epi_px = 3.0;
  o->refine_iters = 20;
  o->min_inliers = 8;
  o->max_depth = 50.0;
  return BA_OK;
}
extern "C" int ba_relative_pose(ba_handle* h, const double K[9], int32_t n_pairs, const int64_t* pair_off, const double* pts1, const double* pts2,
                                const ba_relpose_options* opts, double* R, double* t, uint8_t* status, int32_t* n_inliers, double* rms_px,
                                double* parallax_deg, int32_t* best_hyp, uint8_t* match_inlier) {
  if (!h || !K || !opts) return fail(BA_ERR_INVALID, "null argument");
  if (int rc = pairs_check("ba_relative_pose", K, n_pairs, pair_off, pts1, pts2, opts->n_hyp, opts->lo_rounds, opts->refine_iters, opts->min_inliers))
    return rc;
  if (!(opts->max_epi_px > 0)) return fail(BA_ERR_INVALID, "ba_relative_pose: max_epi_px must be positive");
  if (n_pairs == 0) return BA_OK;
  const size_t np = (size_t)n_pairs;
  const int n_blk = (RP_SLOTS * opts->n_hyp + RP_THREADS - 1) / RP_THREADS;
  RelposeArgs a = {};
  const PairOpts o = {opts->n_hyp, opts->lo_rounds, opts->refine_iters, opts->min_inliers, opts->seed, opts->max_epi_px};
  if (int rc = pairs_upload(h, K, n_pairs, pair_off, pts1, pts2, o, n_blk, RP_BEST, RP_OUT, a)) return rc;
  HIPCHECK(h->scratch.take(9 * (size_t)RP_SLOTS * np * opts->n_hyp, &a.E)); HIPCHECK(h->scratch.take(np * opts->n_hyp, &a.mask));
  a.max_depth = opts->max_depth; a.min_parallax = opts->min_parallax_deg;
  const dim3 b(RP_THREADS);
  BA_LAUNCH(k_relpose_solve, dim3(n_pairs, (opts->n_hyp + RP_TEAMS - 1) / RP_TEAMS), b, 0, h->stream, a);
  BA_LAUNCH(k_relpose_score, dim3(n_pairs, n_blk), b, 0, h->stream, a);
  BA_LAUNCH(k_relpose_lo, dim3(n_pairs), b, 0, h->stream, a);
  const bool want = R || t || status || n_inliers || rms_px || parallax_deg || best_hyp;
  std::vector<double> res;
  if (int rc = pairs_download(h, a, want, RP_OUT, n_pairs, pair_off, match_inlier, res)) return rc;
  if (want)
    for (size_t p = 0; p < np; ++p) {
      const double* r = res.data() + RP_OUT * p;
      if (R) memcpy(R + 9 * p, r, 9 * sizeof(double));
      if (t) memcpy(t + 3 * p, r + 9, 3 * sizeof(double));
      if (status) status[p] = (uint8_t)r[12];
      if (n_inliers) n_inliers[p] = (int32_t)r[13];
      if (rms_px) rms_px[p] = r[14];
      if (parallax_deg) parallax_deg[p] = r[15];
      if (best_hyp) best_hyp[p] = (int32_t)r[16];
    }
  return BA_OK;
}

// ------------------------------------------------------------------------------------------------- two-view homography
// ba_homography (csrc/ba_homography.hpp): four-point hypotheses and scores, local optimisation, decomposition.  Needs no problem.
static_assert(HG_OK == BA_HOMOGRAPHY_OK && HG_FEW_MATCHES == BA_HOMOGRAPHY_FEW_MATCHES && HG_DEGENERATE == BA_HOMOGRAPHY_DEGENERATE &&
              HG_FEW_INLIERS == BA_HOMOGRAPHY_FEW_INLIERS && HG_ROTATION == BA_HOMOGRAPHY_ROTATION && HG_AMBIGUOUS == BA_HOMOGRAPHY_AMBIGUOUS &&
              sizeof(ba_homography_options) == 56, "device status codes (ba_homography.hpp)");
extern "C" int ba_default_homography_options(ba_homography_options* o) {
  if (!o) return fail(BA_ERR_INVALID, "null argument");
  memset(o, 0, sizeof *o);
  o->n_hyp = 256;
  o->lo_rounds = 2;
  o->max_px = 3.0;
  o->refine_iters = 20;
  o->min_inliers = 8;
  o->max_depth = 50.0;
  o->ambiguity_ratio = 0.75;
  o->min_translation = 0.024;
  return BA_OK;
}
extern "C" int ba_homography(ba_handle* h, const double K[9], int32_t n_pairs, const int64_t* pair_off, const double* pts1, const double* pts2,
                             const ba_homography_options* opts, double* H, uint8_t* status, int32_t* n_inliers, double* rms_px, int32_t* best_hyp,
                             uint8_t* match_inlier, int32_t* n_pose, double* R, double* t, double* normal, double* t_over_d, int32_t* votes,
                             double* pose_cost) {
  if (!h || !K || !opts) return fail(BA_ERR_INVALID, "null argument");
  if (int rc = pairs_check("ba_homography", K, n_pairs, pair_off, pts1, pts2, opts->n_hyp, opts->lo_rounds, opts->refine_iters, opts->min_inliers))
    return rc;
  if (!(opts->max_px > 0)) return fail(BA_ERR_INVALID, "ba_homography: max_px must be positive");
  if (!(opts->ambiguity_ratio >= 0 && opts->ambiguity_ratio <= 1)) return fail(BA_ERR_INVALID, "ba_homography: ambiguity_ratio must lie in [0, 1]");
  if (!(opts->min_translation >= 0)) return fail(BA_ERR_INVALID, "ba_homography: min_translation must not be negative");
  if (n_pairs == 0) return BA_OK;
  const size_t np = (size_t)n_pairs;
  const int n_blk = (opts->n_hyp + HG_THREADS - 1) / HG_THREADS;
  HomogArgs a = {};
  const PairOpts o = {opts->n_hyp, opts->lo_rounds, opts->refine_iters, opts->min_inliers, opts->seed, opts->max_px};
  if (int rc = pairs_upload(h, K, n_pairs, pair_off, pts1, pts2, o, n_blk, HG_BEST, HG_OUT, a)) return rc;
  a.max_depth = opts->max_depth; a.ambiguity = opts->ambiguity_ratio; a.min_translation = opts->min_translation;
  const dim3 b(HG_THREADS);
  BA_LAUNCH(k_homog_score, dim3(n_pairs, n_blk), b, 0, h->stream, a);
  BA_LAUNCH(k_homog_lo, dim3(n_pairs), b, 0, h->stream, a);
  const bool want = H || status || n_inliers || rms_px || best_hyp || n_pose || R || t || normal || t_over_d || votes || pose_cost;
  std::vector<double> res;
  if (int rc = pairs_download(h, a, want, HG_OUT, n_pairs, pair_off, match_inlier, res)) return rc;
  if (want)
    for (size_t p = 0; p < np; ++p) {
      const double* r = res.data() + HG_OUT * p;
      if (H) memcpy(H + 9 * p, r, 9 * sizeof(double));
      if (status) status[p] = (uint8_t)r[9];
      if (n_inliers) n_inliers[p] = (int32_t)r[10];
      if (rms_px) rms_px[p] = r[11];
      if (best_hyp) best_hyp[p] = (int32_t)r[12];
      if (n_pose) n_pose[p] = (int32_t)r[13];
      if (R) memcpy(R + 18 * p, r + 14, 18 * sizeof(double));
      if (t) memcpy(t + 6 * p, r + 32, 6 * sizeof(double));
      if (normal) memcpy(normal + 6 * p, r + 38, 6 * sizeof(double));
      if (t_over_d) memcpy(t_over_d + 2 * p, r + 44, 2 * sizeof(double));
      if (votes) { votes[2 * p] = (int32_t)r[46]; votes[2 * p + 1] = (int32_t)r[47]; }
      if (pose_cost) memcpy(pose_cost + 2 * p, r + 48, 2 * sizeof(double));
    }
  return BA_OK;
}

// ------------------------------------------------------------------------------------------------- Sim(3) from 3D-3D matches
// ba_sim3 (csrc/ba_sim3.hpp): three-point hypotheses and scores, local optimisation, the Hessian of the result.  Needs no problem.
static_assert(S3_OK == BA_SIM3_OK && S3_FEW_MATCHES == BA_SIM3_FEW_MATCHES && S3_DEGENERATE == BA_SIM3_DEGENERATE &&
              S3_FEW_INLIERS == BA_SIM3_FEW_INLIERS && sizeof(ba_sim3_options) == 40, "device status codes (ba_sim3.hpp)");
extern "C" int ba_default_sim3_options(ba_sim3_options* o) {
  if (!o) return fail(BA_ERR_INVALID, "null argument");
  memset(o, 0, sizeof *o);
  o->n_hyp = 256;
  o->lo_rounds = 2;
  o->max_px = 4.0;
  o->refine_iters = 20;
  o->min_inliers = 8;
  o->with_scale = 1;
  return BA_OK;
}
extern "C" int ba_sim3(ba_handle* h, const double K[9], int32_t n_pairs, const int64_t* pair_off, const double* X1, const double* X2,
                       const ba_sim3_options* opts, double* sim, double* R, uint8_t* status, int32_t* n_inliers, double* rms_px,
                       int32_t* best_hyp, uint8_t* match_inlier, double* hessian) {
  if (!h || !K || !opts) return fail(BA_ERR_INVALID, "null argument");
  if (int rc = pairs_check("ba_sim3", K, n_pairs, pair_off, X1, X2, opts->n_hyp, opts->lo_rounds, opts->refine_iters, opts->min_inliers))
    return rc;
  if (!(opts->max_px > 0)) return fail(BA_ERR_INVALID, "ba_sim3: max_px must be positive");
  if (opts->with_scale != 0 && opts->with_scale != 1) return fail(BA_ERR_INVALID, "ba_sim3: with_scale must be 0 or 1");
  if (n_pairs == 0) return BA_OK;
  const size_t np = (size_t)n_pairs;
  const int n_blk = (opts->n_hyp + S3_THREADS - 1) / S3_THREADS;
  Sim3Args a = {};
  const PairOpts o = {opts->n_hyp, opts->lo_rounds, opts->refine_iters, opts->min_inliers, opts->seed, opts->max_px};
  if (int rc = pairs_upload(h, K, n_pairs, pair_off, 3, X1, X2, o, n_blk, S3_BEST, S3_OUT, a, a.X1, a.X2)) return rc;
  a.with_scale = opts->with_scale;
  const dim3 b(S3_THREADS);
  BA_LAUNCH(k_sim3_score, dim3(n_pairs, n_blk), b, 0, h->stream, a);
  BA_LAUNCH(k_sim3_lo, dim3(n_pairs), b, 0, h->stream, a);
  const bool want = sim || R || status || n_inliers || rms_px || best_hyp || hessian;
  std::vector<double> res;
  if (int rc = pairs_download(h, a, want, S3_OUT, n_pairs, pair_off, match_inlier, res)) return rc;
  if (want)
    for (size_t p = 0; p < np; ++p) {
      const double* r = res.data() + S3_OUT * p;
      if (sim) memcpy(sim + 7 * p, r, 7 * sizeof(double));
      if (R) memcpy(R + 9 * p, r + 7, 9 * sizeof(double));
      if (status) status[p] = (uint8_t)r[16];
      if (n_inliers) n_inliers[p] = (int32_t)r[17];
      if (rms_px) rms_px[p] = r[18];
      if (best_hyp) best_hyp[p] = (int32_t)r[19];
      if (hessian)
        for (int i = 0; i < 7; ++i)
          for (int j = i; j < 7; ++j) hessian[49 * p + 7 * i + j] = hessian[49 * p + 7 * j + i] = r[20 + UT(7, i, j)];
    }
  return BA_OK;
}

// ------------------------------------------------------------------------------------------------- two-view fundamental matrix
// ba_fundamental (csrc/ba_fundamental.hpp): Hartley normalisation, seven-point hypotheses, scores, local optimisation.  Needs no
// problem and no K: thr is max_epi_px and the pixels pass as they are.
static_assert(FD_OK == BA_FUNDAMENTAL_OK && FD_FEW_MATCHES == BA_FUNDAMENTAL_FEW_MATCHES && FD_DEGENERATE == BA_FUNDAMENTAL_DEGENERATE &&
              FD_FEW_INLIERS == BA_FUNDAMENTAL_FEW_INLIERS && sizeof(ba_fundamental_options) == 32, "device status codes (ba_fundamental.hpp)");
extern "C" int ba_default_fundamental_options(ba_fundamental_options* o) {
  if (!o) return fail(BA_ERR_INVALID, "null argument");
  memset(o, 0, sizeof *o);
  o->n_hyp = 1024;
  o->lo_rounds = 2;
  o->max_epi_px = 3.0;
  o->refine_iters = 20;
  o->min_inliers = 16;
  return BA_OK;
}
extern "C" int ba_fundamental(ba_handle* h, int32_t n_pairs, const int64_t* pair_off, const double* pts1, const double* pts2,
                              const ba_fundamental_options* opts, double* F, uint8_t* status, int32_t* n_inliers, double* rms_px,
                              int32_t* best_hyp, uint8_t* match_inlier, double* epipole1, double* epipole2) {
  if (!h || !opts) return fail(BA_ERR_INVALID, "null argument");
  if (int rc = pairs_check("ba_fundamental", nullptr, n_pairs, pair_off, pts1, pts2, opts->n_hyp, opts->lo_rounds, opts->refine_iters, opts->min_inliers))
    return rc;
  if (!(opts->max_epi_px > 0)) return fail(BA_ERR_INVALID, "ba_fundamental: max_epi_px must be positive");
  if (n_pairs == 0) return BA_OK;
  const size_t np = (size_t)n_pairs;
  const int n_blk = (FD_SLOTS * opts->n_hyp + FD_THREADS - 1) / FD_THREADS;
  FundArgs a = {};
  const PairOpts o = {opts->n_hyp, opts->lo_rounds, opts->refine_iters, opts->min_inliers, opts->seed, opts->max_epi_px};
  if (int rc = pairs_upload(h, nullptr, n_pairs, pair_off, pts1, pts2, o, n_blk, FD_BEST, FD_OUT, a)) return rc;
  HIPCHECK(h->scratch.take(FD_NORM * np, &a.nrm)); HIPCHECK(h->scratch.take(9 * (size_t)FD_SLOTS * np * opts->n_hyp, &a.F));
  HIPCHECK(h->scratch.take(np * opts->n_hyp, &a.mask));
  const dim3 b(FD_THREADS);
  BA_LAUNCH(k_fund_norm, dim3(n_pairs), b, 0, h->stream, a);
  BA_LAUNCH(k_fund_solve, dim3(n_pairs, (opts->n_hyp + FD_SOLVE_THREADS - 1) / FD_SOLVE_THREADS), dim3(FD_SOLVE_THREADS), 0, h->stream, a);
  BA_LAUNCH(k_fund_score, dim3(n_pairs, n_blk), b, 0, h->stream, a);
  BA_LAUNCH(k_fund_lo, dim3(n_pairs), b, 0, h->stream, a);
  const bool want = F || status || n_inliers || rms_px || best_hyp || epipole1 || epipole2;
  std::vector<double> res;
  if (int rc = pairs_download(h, a, want, FD_OUT, n_pairs, pair_off, match_inlier, res)) return rc;
  if (want)
    for (size_t p = 0; p < np; ++p) {
      const double* r = res.data() + FD_OUT * p;
      if (F) memcpy(F + 9 * p, r, 9 * sizeof(double));
      if (status) status[p] = (uint8_t)r[9];
      if (n_inliers) n_inliers[p] = (int32_t)r[10];
      if (rms_px) rms_px[p] = r[11];
      if (best_hyp) best_hyp[p] = (int32_t)r[12];
      if (epipole1) memcpy(epipole1 + 3 * p, r + 13, 3 * sizeof(double));
      if (epipole2) memcpy(epipole2 + 3 * p, r + 16, 3 * sizeof(double));
    }
  return BA_OK;
}

// ------------------------------------------------------------------------------------------------- descriptor matching
// ba_match_descriptors (csrc/ba_match.hpp): Hamming 2-NN of every pair, ratio / distance / mutual tests.  Needs no problem.
static_assert(sizeof(ba_match_options) == 16, "ba_match_options (include/ba_hip.h)");
extern "C" int ba_default_match_options(ba_match_options* o) {
  if (!o) return fail(BA_ERR_INVALID, "null argument");
  memset(o, 0, sizeof *o);
  o->ratio = 0.75;
  o->max_distance = -1;
  return BA_OK;
}
// What the split rule takes of a partial kernel: queries per workgroup, train descriptors per LDS tile, the shortest split, and
// the waves a workgroup spends on 64 queries
struct MatchGeom { int block, tile, min_split, waves_per_row; };
constexpr MatchGeom MT_GEOM = {MT_THREADS, MT_TILE, MT_MIN_SPLIT, 1};      // k_match_partial, k_guided_partial
constexpr MatchGeom ML_GEOM = {ML_BLOCK, ML_TILE, ML_MIN_SPLIT, 2};        // k_l2_partial
// Train splits of one entry.  `want` splits are asked for (the call-wide wish, or the test hook's number); a split is whole
// tiles and at least min_split descriptors unless it is the whole set; at most MT_MAX_SPLITS.
static void match_plan(MatchPair& e, int want, const MatchGeom& g) {
  if (e.nt == 0 || e.nq == 0) { e.split_len = g.tile; e.n_splits = 0; return; }   // nothing to launch for the entry
  const int tiles = (e.nt + g.tile - 1) / g.tile;
  const int n = std::max(1, std::min({want, MT_MAX_SPLITS, tiles / (g.min_split / g.tile)}));
  e.split_len = (tiles + n - 1) / n * g.tile;
  e.n_splits = (e.nt + e.split_len - 1) / e.split_len;
}
// The statement fn<W>(...) with W = W_, the 64-bit words of a descriptor (1 .. MT_MAX_WORDS = 8)
#define BA_BY_WORDS(W_, fn, ...)                   \
  switch (W_) {                                    \
    case 1: fn<1>(__VA_ARGS__); break;             \
    case 2: fn<2>(__VA_ARGS__); break;             \
    case 3: fn<3>(__VA_ARGS__); break;             \
    case 4: fn<4>(__VA_ARGS__); break;             \
    case 5: fn<5>(__VA_ARGS__); break;             \
    case 6: fn<6>(__VA_ARGS__); break;             \
    case 7: fn<7>(__VA_ARGS__); break;             \
    default: fn<8>(__VA_ARGS__); break;            \
  }
template <int W>
static void launch_match_partial(ba_handle* h, dim3 grid, const MatchArgs& a) {
  BA_LAUNCH(k_match_partial<W>, grid, dim3(MT_THREADS), 0, h->stream, a);
}
// The widths a call takes: the multiples of `unit` bytes in unit .. most
struct WidthRule { int unit, most; };
constexpr WidthRule MT_WIDTHS = {8, 8 * MT_MAX_WORDS};      // binary descriptors: matching, guided matching, place recognition
constexpr WidthRule ML_WIDTHS = {32, 32 * ML_MAX_W};        // ba_match_l2
static int desc_bytes_check(const char* who, int32_t desc_bytes, const WidthRule& w = MT_WIDTHS) {
  if (desc_bytes < w.unit || desc_bytes > w.most || desc_bytes % w.unit != 0)
    return fail(BA_ERR_INVALID, "%s: desc_bytes %d is not a multiple of %d in %d .. %d", who, desc_bytes, w.unit, w.unit, w.most);
  return BA_OK;
}
// What the calls that take descriptor sets (matching, place recognition) refuse alike; `who` is the call the message names.
static int desc_sets_check(const char* who, int32_t desc_bytes, int32_t n_sets, const int64_t* set_off, const uint8_t* desc,
                           const WidthRule& w = MT_WIDTHS) {
  if (int rc = desc_bytes_check(who, desc_bytes, w)) return rc;
  if (n_sets < 0 || n_sets > 65535) return fail(BA_ERR_INVALID, "%s: n_sets %d is outside 0 .. 65535", who, n_sets);
  if (!set_off) return fail(BA_ERR_INVALID, "%s: null set_off", who);
  if (set_off[0] != 0) return fail(BA_ERR_INVALID, "%s: set_off[0] must be 0", who);
  for (int32_t s = 0; s < n_sets; ++s)
    if (set_off[s + 1] < set_off[s]) return fail(BA_ERR_INVALID, "%s: set_off decreases at set %d", who, s);
  if (set_off[n_sets] > 0 && !desc) return fail(BA_ERR_INVALID, "%s: null desc", who);
  return BA_OK;
}
// What ba_match_descriptors, ba_match_guided and ba_match_l2 (with ML_WIDTHS) refuse beyond that
static int match_check(const char* who, int32_t desc_bytes, int32_t n_sets, const int64_t* set_off, const uint8_t* desc, int32_t n_pairs,
                       const int32_t* pair_query, const int32_t* pair_train, double ratio, const WidthRule& w = MT_WIDTHS) {
  if (int rc = desc_sets_check(who, desc_bytes, n_sets, set_off, desc, w)) return rc;
  if (n_pairs < 0 || n_pairs > 65535) return fail(BA_ERR_INVALID, "%s: n_pairs %d is outside 0 .. 65535", who, n_pairs);
  if (!std::isfinite(ratio)) return fail(BA_ERR_INVALID, "%s: ratio must be finite", who);
  for (int32_t s = 0; s < n_sets; ++s)
    if (set_off[s + 1] - set_off[s] > (1LL << MT_IDX_BITS))
      return fail(BA_ERR_INVALID, "%s: set_off: set %d holds %lld descriptors, more than %d", who, s,
                  (long long)(set_off[s + 1] - set_off[s]), 1 << MT_IDX_BITS);
  if (n_pairs > 0 && !pair_query) return fail(BA_ERR_INVALID, "%s: null pair_query", who);
  if (n_pairs > 0 && !pair_train) return fail(BA_ERR_INVALID, "%s: null pair_train", who);
  for (int32_t p = 0; p < n_pairs; ++p) {
    if (pair_query[p] < 0 || pair_query[p] >= n_sets)
      return fail(BA_ERR_INVALID, "%s: pair_query[%d] = %d is outside 0 .. n_sets - 1", who, p, pair_query[p]);
    if (pair_train[p] < 0 || pair_train[p] >= n_sets)
      return fail(BA_ERR_INVALID, "%s: pair_train[%d] = %d is outside 0 .. n_sets - 1", who, p, pair_train[p]);
  }
  return BA_OK;
}
// The entries of a call and what its launches are sized by
struct MatchTable {
  std::vector<MatchPair> tab;        // the call's pairs, then (mutual) the same pairs with the roles swapped
  long long rows = 0, wave_rows = 0, n_part = 0;
  int max_qb = 0, max_splits = 0, fin_qb = 0;
};
// A swapped entry's row0 is 0 (ba_match_descriptors: unused) or, with pair_rows, its pair's row0 (ba_match_guided: the rows of
// the gate records its tiles carry).  Writes row_off when it is asked for.
static void match_entries(MatchTable& m, const int64_t* set_off, int32_t n_pairs, const int32_t* pair_query, const int32_t* pair_train,
                          bool mutual, bool pair_rows, int64_t* row_off) {
  const size_t np = (size_t)n_pairs;
  m.tab.assign((mutual ? 2 : 1) * np, MatchPair{});
  for (size_t p = 0; p < np; ++p) {
    MatchPair& e = m.tab[p];
    e.q0 = set_off[pair_query[p]]; e.nq = (int)(set_off[pair_query[p] + 1] - e.q0);
    e.t0 = set_off[pair_train[p]]; e.nt = (int)(set_off[pair_train[p] + 1] - e.t0);
    e.row0 = m.rows;
    if (row_off) row_off[p] = m.rows;
    m.rows += e.nq;
    m.wave_rows += (e.nq + 63) / 64;
    if (mutual) {
      MatchPair& r = m.tab[np + p];
      r.q0 = e.t0; r.nq = e.nt; r.t0 = e.q0; r.nt = e.nq; r.row0 = pair_rows ? e.row0 : 0;
      m.wave_rows += (r.nq + 63) / 64;
    }
  }
  if (row_off) row_off[np] = m.rows;
}
// The splits of every entry (rows > 0).  Two waves per SIMD over the whole call: want = ceil(8 n_cu / waves of the call's wave rows)
static void match_plan_all(const ba_handle* h, MatchTable& m, size_t n_pairs, const MatchGeom& g = MT_GEOM) {
  const long long target = 8LL * h->n_cu, waves = m.wave_rows * g.waves_per_row;
  const int want = h->debug_match_splits > 0 ? h->debug_match_splits
                                             : (int)std::min<long long>(MT_MAX_SPLITS, (target + waves - 1) / waves);
  for (MatchPair& e : m.tab) {
    match_plan(e, want, g);
    e.part0 = m.n_part;
    m.n_part += (long long)e.nq * e.n_splits;
    if (e.n_splits > 0) m.max_qb = std::max(m.max_qb, (e.nq + g.block - 1) / g.block);
    m.max_splits = std::max(m.max_splits, e.n_splits);
  }
  for (size_t p = 0; p < n_pairs; ++p) m.fin_qb = std::max(m.fin_qb, (m.tab[p].nq + MT_THREADS - 1) / MT_THREADS);
}
// The call begun and what the matching calls share of it: the arrays, the kernels' common arguments, the uploads of descriptors and
// table, n_good zeroed.  part_words: the 8-byte words of one (query, split) of `part` (ba_match_l2: two 64-bit keys)
static int match_stage(ba_handle* h, const MatchTable& m, int32_t desc_bytes, size_t n_desc, const uint8_t* desc, int32_t n_pairs,
                       double ratio, int32_t max_distance, bool mutual, MatchArgs& a, size_t part_words = 1) {
  const size_t nr = (size_t)m.rows, np = (size_t)n_pairs, W = (size_t)desc_bytes / 8;
  Scratch& sc = h->scratch;
  HIPCHECK(sc.begin(h->stream));
  a = {};
  HIPCHECK(sc.put(h->stream, n_desc * W, desc, &a.desc)); HIPCHECK(sc.put(h->stream, m.tab.size(), m.tab.data(), &a.pairs));
  HIPCHECK(sc.take((size_t)m.n_part * part_words, &a.part)); HIPCHECK(sc.take(nr, &a.best, &a.second, &a.dist1, &a.dist2));
  HIPCHECK(sc.take(nr, &a.good)); HIPCHECK(sc.take(np, &a.n_good));
  a.n_pairs = n_pairs; a.mutual = mutual ? 1 : 0; a.max_distance = max_distance; a.ratio = ratio;
  HIPCHECK(hipMemsetAsync(a.n_good, 0, np * sizeof(int), h->stream));
  return BA_OK;
}
// best | second | dist1 | dist2, good and n_good to the caller, where asked for (queued; the caller drains the stream)
static int match_fetch(ba_handle* h, const MatchArgs& a, size_t nr, size_t np, int32_t* best, int32_t* second, int32_t* dist1, int32_t* dist2,
                       uint8_t* good, int32_t* n_good) {
  int32_t* const outs[4] = {best, second, dist1, dist2};
  const int* const from[4] = {a.best, a.second, a.dist1, a.dist2};
  for (int k = 0; k < 4; ++k)
    if (outs[k]) HIPCHECK(hipMemcpyAsync(outs[k], from[k], nr * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  if (good) HIPCHECK(hipMemcpyAsync(good, a.good, nr, hipMemcpyDeviceToHost, h->stream));
  if (n_good) HIPCHECK(hipMemcpyAsync(n_good, a.n_good, np * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  return BA_OK;
}
extern "C" int ba_match_descriptors(ba_handle* h, int32_t desc_bytes, int32_t n_sets, const int64_t* set_off, const uint8_t* desc,
                                    int32_t n_pairs, const int32_t* pair_query, const int32_t* pair_train, const ba_match_options* opts,
                                    int64_t* row_off, int32_t* best, int32_t* second, int32_t* dist1, int32_t* dist2,
                                    uint8_t* good, int32_t* n_good) {
  if (!h || !opts) return fail(BA_ERR_INVALID, "null argument");
  if (int rc = match_check("ba_match_descriptors", desc_bytes, n_sets, set_off, desc, n_pairs, pair_query, pair_train, opts->ratio)) return rc;
  const size_t n_desc = (size_t)set_off[n_sets], np = (size_t)n_pairs, W = (size_t)desc_bytes / 8;
  const bool mutual = opts->mutual != 0;
  MatchTable m;
  match_entries(m, set_off, n_pairs, pair_query, pair_train, mutual, false, row_off);
  if (n_good) memset(n_good, 0, np * sizeof(int32_t));
  if (m.rows == 0) return BA_OK;     // no query anywhere: nothing to compute, and every output is already well-formed
  if (set_device(h)) return BA_ERR_HIP;
  match_plan_all(h, m, np);
  MatchArgs a;
  if (int rc = match_stage(h, m, desc_bytes, n_desc, desc, n_pairs, opts->ratio, opts->max_distance, mutual, a)) return rc;
  if (m.max_splits > 0) {
    const dim3 grid((unsigned)m.tab.size(), (unsigned)m.max_qb, (unsigned)m.max_splits);
    BA_BY_WORDS(W, launch_match_partial, h, grid, a);
  }
  BA_LAUNCH(k_match_finish, dim3((unsigned)np, (unsigned)m.fin_qb), dim3(MT_THREADS), 0, h->stream, a);
  if (int rc = match_fetch(h, a, (size_t)m.rows, np, best, second, dist1, dist2, good, n_good)) return rc;
  BA_SYNC(h);
  return BA_OK;
}

// ba_match_l2 (csrc/ba_match_l2.hpp): the same call under the squared Euclidean distance of uint8 descriptors.  Needs no problem.
template <int W>
static void launch_l2_partial(ba_handle* h, dim3 grid, const L2Args& a) {
  BA_LAUNCH(k_l2_partial<W>, grid, dim3(ML_THREADS), 0, h->stream, a);
}
extern "C" int ba_match_l2(ba_handle* h, int32_t desc_bytes, int32_t n_sets, const int64_t* set_off, const uint8_t* desc,
                           int32_t n_pairs, const int32_t* pair_query, const int32_t* pair_train, const ba_match_options* opts,
                           int64_t* row_off, int32_t* best, int32_t* second, int32_t* dist1, int32_t* dist2,
                           uint8_t* good, int32_t* n_good) {
  if (!h || !opts) return fail(BA_ERR_INVALID, "null argument");
  if (int rc = match_check("ba_match_l2", desc_bytes, n_sets, set_off, desc, n_pairs, pair_query, pair_train, opts->ratio, ML_WIDTHS)) return rc;
  const size_t n_desc = (size_t)set_off[n_sets], np = (size_t)n_pairs, W = (size_t)desc_bytes / 32;
  const bool mutual = opts->mutual != 0;
  MatchTable m;
  match_entries(m, set_off, n_pairs, pair_query, pair_train, mutual, false, row_off);
  if (n_good) memset(n_good, 0, np * sizeof(int32_t));
  if (m.rows == 0) return BA_OK;     // no query anywhere: nothing to compute, and every output is already well-formed
  if (set_device(h)) return BA_ERR_HIP;
  match_plan_all(h, m, np, ML_GEOM);
  L2Args a = {};
  if (int rc = match_stage(h, m, desc_bytes, n_desc, desc, n_pairs, opts->ratio, opts->max_distance, mutual, a.m, 2)) return rc;
  int *norm = nullptr, *tbase = nullptr;
  HIPCHECK(h->scratch.take(n_desc, &norm, &tbase));
  a.norm = norm; a.tbase = tbase;
  if (m.max_splits > 0) {
    BA_LAUNCH(k_l2_norms, dim3((unsigned)((n_desc + 255) / 256)), dim3(256), 0, h->stream, (uint4*)a.m.desc, norm, tbase, (long long)n_desc,
              (int)(2 * W));
    const dim3 grid((unsigned)m.tab.size(), (unsigned)m.max_qb, (unsigned)m.max_splits);
    BA_BY_WORDS(W, launch_l2_partial, h, grid, a);
  }
  BA_LAUNCH(k_l2_finish, dim3((unsigned)np, (unsigned)m.fin_qb), dim3(MT_THREADS), 0, h->stream, a);
  if (int rc = match_fetch(h, a.m, (size_t)m.rows, np, best, second, dist1, dist2, good, n_good)) return rc;
  BA_SYNC(h);
  return BA_OK;
}

// ba_match_guided (csrc/ba_match_guided.hpp): the same 2-NN over the train rows a gate admits.  Needs no problem.
static_assert(sizeof(ba_guided_options) == 32, "ba_guided_options (include/ba_hip.h)");
static_assert(MG_WINDOW == BA_GATE_WINDOW && MG_EPIPOLAR == BA_GATE_EPIPOLAR, "device gate codes (ba_match_guided.hpp)");
extern "C" int ba_default_guided_options(ba_guided_options* o) {
  if (!o) return fail(BA_ERR_INVALID, "null argument");
  memset(o, 0, sizeof *o);
  o->ratio = 0.75;
  o->max_distance = -1;
  o->single = 1;
  o->max_epi_px = 3.0;
  return BA_OK;
}
template <int W>
static void launch_guided_partial(ba_handle* h, dim3 grid, const GuidedArgs& a) {
  if (a.gate == MG_WINDOW) BA_LAUNCH((k_guided_partial<W, MG_WINDOW>), grid, dim3(MT_THREADS), 0, h->stream, a);
  else BA_LAUNCH((k_guided_partial<W, MG_EPIPOLAR>), grid, dim3(MT_THREADS), 0, h->stream, a);
}
extern "C" int ba_match_guided(ba_handle* h, int32_t desc_bytes, int32_t n_sets, const int64_t* set_off, const uint8_t* desc, const float* xy,
                               int32_t n_pairs, const int32_t* pair_query, const int32_t* pair_train, const ba_guided_options* opts,
                               const float* window, const double* F, int64_t* row_off, int32_t* best, int32_t* second, int32_t* dist1,
                               int32_t* dist2, uint8_t* good, int32_t* n_good, int32_t* n_cand) {
  if (!h || !opts) return fail(BA_ERR_INVALID, "null argument");
  if (int rc = match_check("ba_match_guided", desc_bytes, n_sets, set_off, desc, n_pairs, pair_query, pair_train, opts->ratio)) return rc;
  const size_t n_desc = (size_t)set_off[n_sets], np = (size_t)n_pairs, W = (size_t)desc_bytes / 8;
  if (n_desc > 0 && !xy) return fail(BA_ERR_INVALID, "ba_match_guided: null xy");
  if (opts->gate != BA_GATE_WINDOW && opts->gate != BA_GATE_EPIPOLAR)
    return fail(BA_ERR_INVALID, "ba_match_guided: gate %d is neither BA_GATE_WINDOW (1) nor BA_GATE_EPIPOLAR (2)", opts->gate);
  if (opts->single != 0 && opts->single != 1) return fail(BA_ERR_INVALID, "ba_match_guided: single %d is not 0 or 1", opts->single);
  const bool epi = opts->gate == BA_GATE_EPIPOLAR, mutual = opts->mutual != 0;
  if (epi) {
    if (!std::isfinite(opts->max_epi_px) || opts->max_epi_px < 0.0) return fail(BA_ERR_INVALID, "ba_match_guided: max_epi_px must be finite and not negative");
    if (n_pairs > 0 && !F) return fail(BA_ERR_INVALID, "ba_match_guided: null F with the epipolar gate");
    for (size_t k = 0; k < 9 * np; ++k)
      if (!std::isfinite(F[k])) return fail(BA_ERR_INVALID, "ba_match_guided: F of pair %d has a non-finite entry", (int)(k / 9));
  }
  MatchTable m;
  match_entries(m, set_off, n_pairs, pair_query, pair_train, mutual, true, nullptr);
  if (!epi && m.rows > 0 && !window) return fail(BA_ERR_INVALID, "ba_match_guided: null window with the window gate");
  if (row_off)
    for (size_t p = 0; p <= np; ++p) row_off[p] = p < np ? m.tab[p].row0 : m.rows;
  if (n_good) memset(n_good, 0, np * sizeof(int32_t));
  if (m.rows == 0) return BA_OK;     // no query anywhere: nothing to compute, and every output is already well-formed
  if (set_device(h)) return BA_ERR_HIP;
  match_plan_all(h, m, np);
  const size_t nr = (size_t)m.rows;
  GuidedArgs a = {};
  if (int rc = match_stage(h, m, desc_bytes, n_desc, desc, n_pairs, opts->ratio, opts->max_distance, mutual, a.m)) return rc;
  Scratch& sc = h->scratch;
  HIPCHECK(sc.put(h->stream, 2 * n_desc, xy, &a.xy)); HIPCHECK(sc.take(4 * nr, &a.rec)); HIPCHECK(sc.take((size_t)m.n_part, &a.cnt)); HIPCHECK(sc.take(nr, &a.n_cand));
  a.gate = opts->gate; a.single = opts->single; a.max_epi2 = opts->max_epi_px * opts->max_epi_px;
  if (epi) HIPCHECK(sc.put(h->stream, 9 * np, F, &a.F));
  else HIPCHECK(sc.put(h->stream, 3 * nr, window, &a.window));
  BA_LAUNCH(k_guided_prepare, dim3((unsigned)np, (unsigned)m.fin_qb), dim3(MT_THREADS), 0, h->stream, a);
  if (m.max_splits > 0) {
    const dim3 grid((unsigned)m.tab.size(), (unsigned)m.max_qb, (unsigned)m.max_splits);
    BA_BY_WORDS(W, launch_guided_partial, h, grid, a);
  }
  BA_LAUNCH(k_guided_finish, dim3((unsigned)np, (unsigned)m.fin_qb), dim3(MT_THREADS), 0, h->stream, a);
  if (int rc = match_fetch(h, a.m, nr, np, best, second, dist1, dist2, good, n_good)) return rc;
  if (n_cand) HIPCHECK(hipMemcpyAsync(n_cand, a.n_cand, nr * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  BA_SYNC(h);
  return BA_OK;
}

// ------------------------------------------------------------------------------------------------- ORB extraction
// ba_orb_extract (csrc/ba_orb.hpp): pyramid, FAST-9, Harris ranking, orientation, steered BRIEF.  Needs no problem.
static_assert(sizeof(ba_orb_options) == 24, "ba_orb_options (include/ba_hip.h)");
constexpr int ORB_MAX_FEATURES = 65536, ORB_MAX_IMAGES = 1024;
constexpr long long ORB_MAX_PIXELS = 1LL << 26, ORB_MAX_BATCH_PIXELS = 1LL << 28;
extern "C" int ba_default_orb_options(ba_orb_options* o) {
  if (!o) return fail(BA_ERR_INVALID, "null argument");
  memset(o, 0, sizeof *o);
  o->scale_factor = 1.2;
  o->n_features = 3000;
  o->n_levels = 8;
  o->edge_threshold = 31;
  o->fast_threshold = 20;
  return BA_OK;
}
extern "C" int ba_orb_default_pattern(int8_t* pattern) {
  if (!pattern) return fail(BA_ERR_INVALID, "null argument");
  memcpy(pattern, kOrbDefaultPattern, sizeof kOrbDefaultPattern);
  return BA_OK;
}
static int orb_check_options(const char* who, const ba_orb_options* o, int32_t height, int32_t width) {
  if (!(o->scale_factor > 1.0) || !(o->scale_factor <= 2.0)) return fail(BA_ERR_INVALID, "%s: scale_factor must be above 1 and at most 2", who);
  if (o->n_features < 1 || o->n_features > ORB_MAX_FEATURES)
    return fail(BA_ERR_INVALID, "%s: n_features %d is outside 1 .. %d", who, o->n_features, ORB_MAX_FEATURES);
  if (o->n_levels < 1 || o->n_levels > ORB_MAX_LEVELS) return fail(BA_ERR_INVALID, "%s: n_levels %d is outside 1 .. %d", who, o->n_levels, ORB_MAX_LEVELS);
  if (o->edge_threshold < 25) return fail(BA_ERR_INVALID, "%s: edge_threshold %d is below 25", who, o->edge_threshold);
  if (o->fast_threshold < 1 || o->fast_threshold > 254) return fail(BA_ERR_INVALID, "%s: fast_threshold %d is outside 1 .. 254", who, o->fast_threshold);
  if (height <= 0) return fail(BA_ERR_INVALID, "%s: height %d is not positive", who, height);
  if (width <= 0) return fail(BA_ERR_INVALID, "%s: width %d is not positive", who, width);
  return BA_OK;
}
// The definition's levels (include/ba_hip.h): every operation on its own, in the order written there
static void orb_levels(const ba_orb_options* o, int32_t height, int32_t width, int32_t* lw, int32_t* lh, double* ls, int32_t* lq) {
  const int L = o->n_levels;
  double s = 1.0;
  for (int l = 0; l < L; ++l) {
    if (l > 0) s = s * o->scale_factor;
    ls[l] = s;
    lw[l] = (int32_t)std::nearbyint((double)width / s);
    lh[l] = (int32_t)std::nearbyint((double)height / s);
  }
  const double f = 1.0 / o->scale_factor;
  double p = 1.0;
  for (int l = 0; l < L; ++l) p = p * f;
  if (L == 1) { lq[0] = o->n_features; return; }
  double d = (double)o->n_features * (1.0 - f) / (1.0 - p);
  int sum = 0;
  for (int l = 0; l < L - 1; ++l) {
    lq[l] = std::min((int32_t)std::nearbyint(d), o->n_features - sum);      // (the roundings of a small n_features can add up to more)
    sum += lq[l];
    d = d * f;
  }
  lq[L - 1] = o->n_features - sum;
}
extern "C" int ba_orb_levels(const ba_orb_options* opts, int32_t height, int32_t width, int32_t* level_w, int32_t* level_h,
                             double* level_scale, int32_t* level_quota) {
  if (!opts) return fail(BA_ERR_INVALID, "null argument");
  if (int rc = orb_check_options("ba_orb_levels", opts, height, width)) return rc;
  int32_t lw[ORB_MAX_LEVELS], lh[ORB_MAX_LEVELS], lq[ORB_MAX_LEVELS];
  double ls[ORB_MAX_LEVELS];
  orb_levels(opts, height, width, lw, lh, ls, lq);
  const size_t L = (size_t)opts->n_levels;
  if (level_w) memcpy(level_w, lw, L * sizeof(int32_t));
  if (level_h) memcpy(level_h, lh, L * sizeof(int32_t));
  if (level_scale) memcpy(level_scale, ls, L * sizeof(double));
  if (level_quota) memcpy(level_quota, lq, L * sizeof(int32_t));
  return BA_OK;
}
extern "C" int ba_orb_stage_times(ba_handle* h, int32_t enable, double* ms) {
  if (!h) return fail(BA_ERR_INVALID, "null handle");
  if (enable < -1 || enable > 1) return fail(BA_ERR_INVALID, "ba_orb_stage_times: enable %d is not -1, 0 or 1", enable);
  if (set_device(h)) return BA_ERR_HIP;
  if (enable == 1)
    for (auto& e : h->orb_ev)
      if (!e) HIPCHECK(hipEventCreate(&e));
  if (enable >= 0) h->orb_timing = enable != 0;
  if (ms) memcpy(ms, h->orb_ms, sizeof h->orb_ms);
  return BA_OK;
}
extern "C" int ba_orb_extract(ba_handle* h, int32_t n_images, int32_t height, int32_t width, const uint8_t* images, const int8_t* pattern,
                              const ba_orb_options* opts, int32_t* n_kp, float* xy, float* size, float* angle, float* response,
                              int32_t* octave, int32_t* level_xy, double* cs, uint8_t* desc) {
  if (!h || !opts) return fail(BA_ERR_INVALID, "null argument");
  if (int rc = orb_check_options("ba_orb_extract", opts, height, width)) return rc;
  if (n_images < 0 || n_images > ORB_MAX_IMAGES) return fail(BA_ERR_INVALID, "ba_orb_extract: n_images %d is outside 0 .. %d", n_images, ORB_MAX_IMAGES);
  if (n_images > 0 && !images) return fail(BA_ERR_INVALID, "ba_orb_extract: null images");
  const long long px = (long long)height * width;
  if (px > ORB_MAX_PIXELS) return fail(BA_ERR_INVALID, "ba_orb_extract: height * width = %lld is above the cap of %lld pixels", px, ORB_MAX_PIXELS);
  if (px * n_images > ORB_MAX_BATCH_PIXELS)
    return fail(BA_ERR_INVALID, "ba_orb_extract: the batch n_images * height * width = %lld is above the cap of %lld pixels", px * n_images, ORB_MAX_BATCH_PIXELS);
  const int8_t* pat = pattern ? pattern : &kOrbDefaultPattern[0][0];
  for (int i = 0; i < 1024; ++i)
    if (pat[i] < -15 || pat[i] > 15)
      return fail(BA_ERR_INVALID, "ba_orb_extract: pattern row %d holds the coordinate %d, outside -15 .. 15", i / 4, (int)pat[i]);
  const size_t B = (size_t)n_images, N = (size_t)opts->n_features;
  if (n_kp) memset(n_kp, 0, B * sizeof(int32_t));
  int32_t lw[ORB_MAX_LEVELS], lh[ORB_MAX_LEVELS], lq[ORB_MAX_LEVELS];
  double ls[ORB_MAX_LEVELS];
  orb_levels(opts, height, width, lw, lh, ls, lq);
  const int edge = opts->edge_threshold;
  OrbArgs a = {};
  while (a.n_levels < opts->n_levels && lw[a.n_levels] > 2 * edge && lh[a.n_levels] > 2 * edge) ++a.n_levels;   // (sizes do not grow)
  if (B == 0 || a.n_levels == 0) return BA_OK;       // no image, or none with an interior: zero keypoints
  if (set_device(h)) return BA_ERR_HIP;
  const int L = a.n_levels;
  a.n_features = opts->n_features; a.edge = edge; a.thr = opts->fast_threshold; a.n_images = n_images;
  long long pix = 0;
  int max_cap = 0;
  for (int l = 0; l < L; ++l) {
    a.w[l] = lw[l]; a.h[l] = lh[l]; a.quota[l] = lq[l]; a.scale[l] = ls[l];
    a.row0[l] = a.rows; a.rows += lh[l];
    a.list0[l] = a.list_cap; a.list_cap += 2 * lq[l];
    a.off[l] = pix; pix += (long long)B * lw[l] * lh[l];
    max_cap = std::max(max_cap, 2 * lq[l]);
  }
  // the outputs by row: xy | size | angle | response, octave | level_xy | n_kp (each group is read back in one copy)
  const size_t npx = (size_t)pix, cap = (size_t)a.list_cap;
  Scratch& sc = h->scratch;
  HIPCHECK(sc.begin(h->stream));
  HIPCHECK(sc.take(npx, &a.pyr, &a.score, &a.blur));
  HIPCHECK(sc.take(B * L * 256, &a.hist)); HIPCHECK(sc.take(B * L, &a.cut)); HIPCHECK(sc.take(B * a.rows, &a.row_a, &a.row_b));
  HIPCHECK(sc.take(B * cap, &a.list)); HIPCHECK(sc.take(B * cap, &a.hs));
  HIPCHECK(sc.take(5 * B * N, &a.xy)); HIPCHECK(sc.take(3 * B * N + B, &a.octave)); HIPCHECK(sc.take(2 * B * N, &a.cs)); HIPCHECK(sc.take(32 * B * N, &a.desc));
  a.size = a.xy + 2 * B * N; a.angle = a.size + B * N; a.response = a.angle + B * N;
  a.level_xy = a.octave + B * N; a.n_kp = a.level_xy + 2 * B * N;
  int stamp = 0;
#define ORB_STAMP() do { if (h->orb_timing) HIPCHECK(hipEventRecord(h->orb_ev[stamp++], h->stream)); } while (0)
  ORB_STAMP();
  HIPCHECK(hipMemcpyAsync(a.pyr, images, B * (size_t)px, hipMemcpyHostToDevice, h->stream));      // level 0 of every image
  HIPCHECK(sc.put(h->stream, 1024, pat, &a.pattern));
  HIPCHECK(hipMemsetAsync(a.hist, 0, B * L * 256 * sizeof(unsigned), h->stream));
  const unsigned nb = (unsigned)B;
  auto tiles = [&](int l) { return dim3((unsigned)((a.w[l] + ORB_TILE_W - 1) / ORB_TILE_W), (unsigned)((a.h[l] + ORB_TILE_H - 1) / ORB_TILE_H), nb); };
  ORB_STAMP();
  for (int l = 1; l < L; ++l)
    BA_LAUNCH(k_orb_resize, dim3((unsigned)((a.w[l] * a.h[l] + ORB_THREADS - 1) / ORB_THREADS), nb), dim3(ORB_THREADS), 0, h->stream, a, l);
  ORB_STAMP();
  for (int l = 0; l < L; ++l) BA_LAUNCH(k_orb_fast, tiles(l), dim3(ORB_THREADS), 0, h->stream, a, l);
  ORB_STAMP();
  BA_LAUNCH(k_orb_cut, dim3(nb), dim3(64), 0, h->stream, a);
  BA_LAUNCH(k_orb_rowcount, dim3((unsigned)a.rows, nb), dim3(64), 0, h->stream, a);
  BA_LAUNCH(k_orb_scan, dim3((unsigned)L, nb), dim3(ORB_THREADS), 0, h->stream, a);
  BA_LAUNCH(k_orb_compact, dim3((unsigned)a.rows, nb), dim3(64), 0, h->stream, a);
  ORB_STAMP();
  if (max_cap > 0) {
    const dim3 grid((unsigned)((max_cap + ORB_THREADS - 1) / ORB_THREADS), (unsigned)L, nb);
    BA_LAUNCH(k_orb_harris, grid, dim3(ORB_THREADS), 0, h->stream, a);
    BA_LAUNCH(k_orb_rank, grid, dim3(ORB_THREADS), 0, h->stream, a);
  }
  ORB_STAMP();
  for (int l = 0; l < L; ++l) BA_LAUNCH(k_orb_blur, tiles(l), dim3(ORB_THREADS), 0, h->stream, a, l);
  ORB_STAMP();
  BA_LAUNCH(k_orb_describe, dim3((unsigned)((N + ORB_KP_PER_BLOCK - 1) / ORB_KP_PER_BLOCK), nb), dim3(ORB_THREADS), 0, h->stream, a);
  ORB_STAMP();
  // the outputs come back whole (stride n_features) into pinned staging; only the rows an image owns go to the caller's arrays
  const size_t stage_bytes = 2 * B * N * sizeof(double) + 5 * B * N * sizeof(float) + (3 * B * N + B) * sizeof(int32_t) + 32 * B * N;
  HIPCHECK(h->orb_stage.reserve(stage_bytes, stage_bytes + stage_bytes / 2, h->stream));      // pinned, kept with the handle
  double* const hc = (double*)h->orb_stage.p;
  float* const hf = (float*)(hc + 2 * B * N);
  int32_t* const hi = (int32_t*)(hf + 5 * B * N);
  int32_t* const hn = hi + 3 * B * N;
  uint8_t* const hd = (uint8_t*)(hn + B);
  HIPCHECK(hipMemcpyAsync(hn, a.n_kp, B * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  if (xy || size || angle || response) HIPCHECK(hipMemcpyAsync(hf, a.xy, 5 * B * N * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  if (octave || level_xy) HIPCHECK(hipMemcpyAsync(hi, a.octave, 3 * B * N * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  if (cs) HIPCHECK(hipMemcpyAsync(hc, a.cs, 2 * B * N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (desc) HIPCHECK(hipMemcpyAsync(hd, a.desc, 32 * B * N, hipMemcpyDeviceToHost, h->stream));
  ORB_STAMP();
#undef ORB_STAMP
  BA_SYNC(h);
  for (int k = 0; k + 1 < stamp; ++k) {
    float ms = 0;
    HIPCHECK(hipEventElapsedTime(&ms, h->orb_ev[k], h->orb_ev[k + 1]));
    h->orb_ms[k] = ms;
  }
  for (size_t b = 0; b < B; ++b) {
    const size_t n = std::min((size_t)std::max(hn[b], 0), N), r = b * N;      // (n_kp <= n_features: the quotas sum to it)
    if (n_kp) n_kp[b] = (int32_t)n;
    if (xy) memcpy(xy + 2 * r, hf + 2 * r, 2 * n * sizeof(float));
    if (size) memcpy(size + r, hf + 2 * B * N + r, n * sizeof(float));
    if (angle) memcpy(angle + r, hf + 3 * B * N + r, n * sizeof(float));
    if (response) memcpy(response + r, hf + 4 * B * N + r, n * sizeof(float));
    if (octave) memcpy(octave + r, hi + r, n * sizeof(int32_t));
    if (level_xy) memcpy(level_xy + 2 * r, hi + B * N + 2 * r, 2 * n * sizeof(int32_t));
    if (cs) memcpy(cs + 2 * r, hc + 2 * r, 2 * n * sizeof(double));
    if (desc) memcpy(desc + 32 * r, hd + 32 * r, 32 * n);
  }
  return BA_OK;
}

// ------------------------------------------------------------------------------------------------- KLT tracking
// ba_track_klt (csrc/ba_klt.hpp): pyramidal Lucas-Kanade.  Needs no problem; its device memory is the scratch arena's.
static_assert(sizeof(ba_klt_options) == 40, "ba_klt_options (include/ba_hip.h)");
static_assert(BA_KLT_OK == KLT_OK && BA_KLT_OUT == KLT_OUT && BA_KLT_FLAT == KLT_FLAT && BA_KLT_FB_FAIL == KLT_FB_FAIL, "device status codes (ba_klt.hpp)");
constexpr int KLT_MAX_PAIRS = 65535;
constexpr long long KLT_MAX_POINTS = 1LL << 24;
extern "C" int ba_default_klt_options(ba_klt_options* o) {
  if (!o) return fail(BA_ERR_INVALID, "null argument");
  memset(o, 0, sizeof *o);
  o->half_window = 10;
  o->max_level = 3;
  o->max_iters = 30;
  o->eps = 0.01;
  o->min_eig = 1e-4;
  o->fb_max_px = 0.0;
  return BA_OK;
}
static int klt_check_options(const char* who, const ba_klt_options* o, int32_t height, int32_t width) {
  if (o->half_window < 1 || o->half_window > KLT_MAX_HALF) return fail(BA_ERR_INVALID, "%s: half_window %d is outside 1 .. %d", who, o->half_window, KLT_MAX_HALF);
  if (o->max_level < 0 || o->max_level > KLT_MAX_LEVELS - 1) return fail(BA_ERR_INVALID, "%s: max_level %d is outside 0 .. %d", who, o->max_level, KLT_MAX_LEVELS - 1);
  if (o->max_iters < 1 || o->max_iters > 100) return fail(BA_ERR_INVALID, "%s: max_iters %d is outside 1 .. 100", who, o->max_iters);
  if (!(o->eps >= 0.0)) return fail(BA_ERR_INVALID, "%s: eps is negative or NaN", who);
  if (!(o->min_eig >= 0.0)) return fail(BA_ERR_INVALID, "%s: min_eig is negative or NaN", who);
  if (o->fb_max_px != o->fb_max_px) return fail(BA_ERR_INVALID, "%s: fb_max_px is NaN", who);
  if (height <= 0) return fail(BA_ERR_INVALID, "%s: height %d is not positive", who, height);
  if (width <= 0) return fail(BA_ERR_INVALID, "%s: width %d is not positive", who, width);
  const int n = 2 * o->half_window + 1;
  if (std::min(height, width) < n) return fail(BA_ERR_INVALID, "%s: the image, width %d x height %d, is smaller than the %d x %d window", who, width, height, n, n);
  return BA_OK;
}
// The definition's levels (include/ba_hip.h) -> the number of levels, L + 1
static int klt_levels(const ba_klt_options* o, int32_t height, int32_t width, int32_t* lw, int32_t* lh) {
  const int n = 2 * o->half_window + 1;
  int l = 0;
  lw[0] = width; lh[0] = height;
  while (l < o->max_level && std::min((lw[l] + 1) / 2, (lh[l] + 1) / 2) >= n) {
    lw[l + 1] = (lw[l] + 1) / 2; lh[l + 1] = (lh[l] + 1) / 2;
    ++l;
  }
  return l + 1;
}
extern "C" int ba_klt_levels(const ba_klt_options* opts, int32_t height, int32_t width, int32_t* n_levels, int32_t* level_w, int32_t* level_h) {
  if (!opts) return fail(BA_ERR_INVALID, "null argument");
  if (int rc = klt_check_options("ba_klt_levels", opts, height, width)) return rc;
  int32_t lw[KLT_MAX_LEVELS], lh[KLT_MAX_LEVELS];
  const int nl = klt_levels(opts, height, width, lw, lh);
  if (n_levels) *n_levels = nl;
  if (level_w) memcpy(level_w, lw, (size_t)nl * sizeof(int32_t));
  if (level_h) memcpy(level_h, lh, (size_t)nl * sizeof(int32_t));
  return BA_OK;
}
extern "C" int ba_klt_stage_times(ba_handle* h, int32_t enable, double* ms) {
  if (!h) return fail(BA_ERR_INVALID, "null handle");
  if (enable < -1 || enable > 1) return fail(BA_ERR_INVALID, "ba_klt_stage_times: enable %d is not -1, 0 or 1", enable);
  if (set_device(h)) return BA_ERR_HIP;
  if (enable == 1)
    for (auto& e : h->klt_ev)
      if (!e) HIPCHECK(hipEventCreate(&e));
  if (enable >= 0) h->klt_timing = enable != 0;
  if (ms) memcpy(ms, h->klt_ms, sizeof h->klt_ms);
  return BA_OK;
}
extern "C" int ba_track_klt(ba_handle* h, int32_t n_images, int32_t height, int32_t width, const uint8_t* images, int32_t n_pairs,
                            const int32_t* pairs, const int64_t* pt_off, const float* prev, const float* guess, const ba_klt_options* opts,
                            float* next, uint8_t* status, float* err, float* fb_err) {
  if (!h || !opts) return fail(BA_ERR_INVALID, "null argument");
  if (int rc = klt_check_options("ba_track_klt", opts, height, width)) return rc;
  if (n_images < 0 || n_images > ORB_MAX_IMAGES) return fail(BA_ERR_INVALID, "ba_track_klt: n_images %d is outside 0 .. %d", n_images, ORB_MAX_IMAGES);
  const long long px = (long long)height * width;
  if (px > ORB_MAX_PIXELS) return fail(BA_ERR_INVALID, "ba_track_klt: height * width = %lld is above the cap of %lld pixels", px, ORB_MAX_PIXELS);
  if (px * n_images > ORB_MAX_BATCH_PIXELS)
    return fail(BA_ERR_INVALID, "ba_track_klt: the batch n_images * height * width = %lld is above the cap of %lld pixels", px * n_images, ORB_MAX_BATCH_PIXELS);
  if (n_pairs < 0 || n_pairs > KLT_MAX_PAIRS) return fail(BA_ERR_INVALID, "ba_track_klt: n_pairs %d is outside 0 .. %d", n_pairs, KLT_MAX_PAIRS);
  if (n_pairs == 0) return BA_OK;
  if (!pairs || !pt_off) return fail(BA_ERR_INVALID, "ba_track_klt: null pairs or pt_off");
  if (pt_off[0] != 0) return fail(BA_ERR_INVALID, "ba_track_klt: pt_off[0] = %lld is not 0", (long long)pt_off[0]);
  for (int p = 0; p < n_pairs; ++p) {
    if (pt_off[p + 1] < pt_off[p]) return fail(BA_ERR_INVALID, "ba_track_klt: pt_off decreases at pair %d", p);
    if (pt_off[p + 1] > KLT_MAX_POINTS) return fail(BA_ERR_INVALID, "ba_track_klt: more than %lld points (pt_off[%d] = %lld)", KLT_MAX_POINTS, p + 1, (long long)pt_off[p + 1]);
    for (int k = 0; k < 2; ++k)
      if (pairs[2 * p + k] < 0 || pairs[2 * p + k] >= n_images)
        return fail(BA_ERR_INVALID, "ba_track_klt: pairs[%d][%d] = %d is no image index (n_images %d)", p, k, pairs[2 * p + k], n_images);
  }
  const size_t N = (size_t)pt_off[n_pairs];
  if (N == 0) return BA_OK;
  if (!images) return fail(BA_ERR_INVALID, "ba_track_klt: null images");
  if (!prev) return fail(BA_ERR_INVALID, "ba_track_klt: null prev");
  // a slot for every image that a pair with points names
  std::vector<int> slot((size_t)n_images, -1), slots(2 * (size_t)n_pairs, 0);
  for (int p = 0; p < n_pairs; ++p)
    if (pt_off[p + 1] > pt_off[p]) slot[pairs[2 * p]] = slot[pairs[2 * p + 1]] = 0;
  int S = 0;
  for (int b = 0; b < n_images; ++b)
    if (slot[b] == 0) slot[b] = S++;
  for (int p = 0; p < n_pairs; ++p)
    for (int k = 0; k < 2; ++k) slots[2 * p + k] = std::max(slot[pairs[2 * p + k]], 0);
  KltArgs a = {};
  int32_t lw[KLT_MAX_LEVELS], lh[KLT_MAX_LEVELS];
  a.n_levels = klt_levels(opts, height, width, lw, lh);
  a.hw = opts->half_window; a.n = 2 * a.hw + 1; a.max_iters = opts->max_iters; a.fb = opts->fb_max_px > 0.0; a.n_pairs = n_pairs;
  a.eps2 = opts->eps * opts->eps; a.min_eig = opts->min_eig; a.fb_max = opts->fb_max_px;
  long long pix = 0;
  for (int l = 0; l < a.n_levels; ++l) {
    a.w[l] = lw[l]; a.h[l] = lh[l];
    a.off[l] = pix; pix += (long long)S * lw[l] * lh[l];
  }
  if (set_device(h)) return BA_ERR_HIP;
  Scratch& sc = h->scratch;
  HIPCHECK(sc.begin(h->stream));
  HIPCHECK(sc.take((size_t)pix, &a.pyr));
  int stamp = 0;
#define KLT_STAMP() do { if (h->klt_timing) HIPCHECK(hipEventRecord(h->klt_ev[stamp++], h->stream)); } while (0)
  KLT_STAMP();
  HIPCHECK(sc.put(h->stream, 2 * (size_t)n_pairs, slots.data(), &a.pair_slot));
  HIPCHECK(sc.put(h->stream, (size_t)n_pairs + 1, pt_off, &a.pt_off));
  HIPCHECK(sc.put(h->stream, 2 * N, prev, &a.prev));
  if (guess) HIPCHECK(sc.put(h->stream, 2 * N, guess, &a.guess));
  HIPCHECK(sc.take(2 * N, &a.next)); HIPCHECK(sc.take(N, &a.err, &a.fb_err)); HIPCHECK(sc.take(N, &a.status));
  for (int b = 0; b < n_images;) {      // level 0 of the slots: the used images, a copy per run of consecutive ones
    if (slot[b] < 0) { ++b; continue; }
    int e = b + 1;
    while (e < n_images && slot[e] >= 0) ++e;
    HIPCHECK(hipMemcpyAsync(a.pyr + (size_t)slot[b] * (size_t)px, images + (size_t)b * (size_t)px, (size_t)(e - b) * (size_t)px, hipMemcpyHostToDevice, h->stream));
    b = e;
  }
  KLT_STAMP();
  for (int l = 1; l < a.n_levels; ++l)
    BA_LAUNCH(k_klt_down, dim3((unsigned)((a.w[l] + KLT_TILE_W - 1) / KLT_TILE_W), (unsigned)((a.h[l] + KLT_TILE_H - 1) / KLT_TILE_H), (unsigned)S),
              dim3(KLT_THREADS), 0, h->stream, a, l);
  KLT_STAMP();
  // the window's elements per lane, ceil(n^2 / 64), rounded up to an instantiation
  const int epl = (a.n * a.n + 63) / 64;
  const dim3 grid((unsigned)N), block(64);
  if (epl <= 2) BA_LAUNCH(k_klt_track<2>, grid, block, 0, h->stream, a);
  else if (epl <= 4) BA_LAUNCH(k_klt_track<4>, grid, block, 0, h->stream, a);
  else if (epl <= 7) BA_LAUNCH(k_klt_track<7>, grid, block, 0, h->stream, a);
  else BA_LAUNCH(k_klt_track<16>, grid, block, 0, h->stream, a);
  static_assert((2 * KLT_MAX_HALF + 1) * (2 * KLT_MAX_HALF + 1) <= 16 * 64, "k_klt_track<16> holds the largest window");
  KLT_STAMP();
  if (next) HIPCHECK(hipMemcpyAsync(next, a.next, 2 * N * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  if (status) HIPCHECK(hipMemcpyAsync(status, a.status, N, hipMemcpyDeviceToHost, h->stream));
  if (err) HIPCHECK(hipMemcpyAsync(err, a.err, N * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  if (fb_err) HIPCHECK(hipMemcpyAsync(fb_err, a.fb_err, N * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  KLT_STAMP();
#undef KLT_STAMP
  BA_SYNC(h);
  for (int k = 0; k + 1 < stamp; ++k) {
    float ms = 0;
    HIPCHECK(hipEventElapsedTime(&ms, h->klt_ev[k], h->klt_ev[k + 1]));
    h->klt_ms[k] = ms;
  }
  return BA_OK;
}

// ------------------------------------------------------------------------------------------------- similarity
// ba_get_centres, ba_transform, ba_align (csrc/ba_similarity.hpp).  Local to the rank: no collective.
extern "C" int ba_get_centres(ba_handle* h, double* centres) {
  if (!h || !centres) return fail(BA_ERR_INVALID, "null argument");
  if (!h->have_problem || !h->have_params) return fail(BA_ERR_STATE, "ba_get_centres: ba_set_problem / ba_set_params first");
  if (set_device(h)) return BA_ERR_HIP;
  const int Nc = h->Nc;
  HIPCHECK(h->sim_buf.alloc(3 * (size_t)Nc));
  BA_LAUNCH(k_sim_centres, dim3((Nc + 255) / 256), dim3(256), 0, h->stream, (const double*)h->cs[h->cur].p, Nc, h->sim_buf.p);
  HIPCHECK(hipMemcpyAsync(centres, h->sim_buf.p, 3 * (size_t)Nc * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  BA_SYNC(h);
  return BA_OK;
}

static const char* kSimPriors = "%s: priors are set (ba_set_priors) and their means live in the old frame: align first, set the priors afterwards";
// What ba_set_params(transformed cameras, transformed points) leaves behind, from the similarity in the device record:
// parameter set 0 written from set `cur`, its point table and camera state rebuilt.  A record that is not OK makes every
// kernel a no-op.  The caller drains the stream, reads the record's status and, when it is OK, calls commit_transform
// (set 0 current, the linearisation forgotten, held_x2 from held_pts, where the held points' new positions were copied).
static int launch_transform(ba_handle* h, std::vector<double>* held_pts) {
  const int Nc = h->Nc, Np = h->Np;
  if (Np > 0)
    BA_LAUNCH(k_sim_transform_points, dim3((Np + 255) / 256), dim3(256), 0, h->stream, (const SimRec*)h->sim_rec.p,
              (const double*)h->ptab[h->cur].p, Np, h->ptab[0].p);
  BA_LAUNCH(k_sim_transform_cams, dim3((Nc + 63) / 64), dim3(64), 0, h->stream, (const SimRec*)h->sim_rec.p,
            (const double*)h->cs[h->cur].p, Nc, h->cams[0].p);
  BA_LAUNCH(k_sim_cam_prepare, dim3((Nc + 63) / 64), dim3(64), 0, h->stream, (const SimRec*)h->sim_rec.p, (const double*)h->cams[0].p,
            (const double*)h->intr[0].p, h->cs[0].p, h->camA[0].p, Nc);
  if (h->any_pt_held && Np > 0) {
    held_pts->resize(3 * (size_t)Np);
    BA_LAUNCH(k_unpack_points, dim3((Np + 255) / 256), dim3(256), 0, h->stream, h->ptab[0].p, h->slot.p, Np, h->stage.p);
    HIPCHECK(hipMemcpyAsync(held_pts->data(), h->stage.p, 3 * (size_t)Np * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  }
  return BA_OK;
}
static void commit_transform(ba_handle* h, const std::vector<double>& held_pts) {
  adopt_set0(h, true);
  if (!held_pts.empty()) h->held_x2 = held_points_x2(h, held_pts.data());
}

extern "C" int ba_transform(ba_handle* h, const ba_similarity* sim) {
  if (!h || !sim) return fail(BA_ERR_INVALID, "null argument");
  if (!h->have_problem || !h->have_params) return fail(BA_ERR_STATE, "ba_transform: ba_set_problem / ba_set_params first");
  if (any_prior(h)) return fail(BA_ERR_STATE, kSimPriors, "ba_transform");
  if (!std::isfinite(sim->s) || !(sim->s > 0)) return fail(BA_ERR_INVALID, "ba_transform: the scale s must be finite and positive");
  for (int i = 0; i < 9; ++i) if (!std::isfinite(sim->R[i])) return fail(BA_ERR_INVALID, "ba_transform: R is not finite");
  for (int i = 0; i < 3; ++i) if (!std::isfinite(sim->t[i])) return fail(BA_ERR_INVALID, "ba_transform: t is not finite");
  const double* R = sim->R;
  double dev = 0.0;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      dev = std::max(dev, std::fabs(R[3 * i] * R[3 * j] + R[3 * i + 1] * R[3 * j + 1] + R[3 * i + 2] * R[3 * j + 2] - (i == j ? 1.0 : 0.0)));
  if (!(dev <= 1e-9)) return fail(BA_ERR_INVALID, "ba_transform: R is not orthogonal (max |R R^T - I| = %.3g > 1e-9)", dev);
  const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
  if (det < 0) return fail(BA_ERR_INVALID, "ba_transform: R is a reflection (det R = %.3g < 0)", det);
  if (set_device(h)) return BA_ERR_HIP;
  HIPCHECK(h->sim_rec.alloc(1));
  SimRec rec = {};
  rec.s = sim->s;
  memcpy(rec.R, sim->R, sizeof rec.R);
  memcpy(rec.t, sim->t, sizeof rec.t);
  rec.status = SIM_OK;
  BA_LAUNCH(k_sim_set, dim3(1), dim3(64), 0, h->stream, rec, h->sim_rec.p);
  std::vector<double> held_pts;
  if (int rc = launch_transform(h, &held_pts)) return rc;
  BA_SYNC(h);
  commit_transform(h, held_pts);
  return BA_OK;
}

extern "C" int ba_default_align_options(ba_align_options* o) {
  if (!o) return fail(BA_ERR_INVALID, "null argument");
  memset(o, 0, sizeof *o);
  o->loss = BA_LOSS_LINEAR;
  o->iters = 10;
  o->f_scale = 1.0;
  o->with_scale = 1;
  o->apply = 0;
  return BA_OK;
}

extern "C" int ba_align(ba_handle* h, const ba_align_options* opts, const double* cam_ref, const double* cam_w, const double* pt_ref,
                        const double* pt_w, ba_align_result* out, double* cam_err, double* pt_err) {
  if (!h || !opts || !out) return fail(BA_ERR_INVALID, "null argument");
  if (!h->have_problem || !h->have_params) return fail(BA_ERR_STATE, "ba_align: ba_set_problem / ba_set_params first");
  if (!loss_valid(opts->loss)) return fail(BA_ERR_INVALID, "ba_align: unknown loss %d", opts->loss);
  if (!(opts->f_scale > 0)) return fail(BA_ERR_INVALID, "ba_align: f_scale must be positive");
  if (opts->iters < 0) return fail(BA_ERR_INVALID, "ba_align: iters must not be negative");
  if (!cam_ref && !pt_ref) return fail(BA_ERR_INVALID, "ba_align: no reference positions (cam_ref and pt_ref are both NULL)");
  // points are rank-local: a similarity estimated with pt_ref differs from rank to rank, and applying it would split the
  // replicated cameras (cam_ref alone sees the same cameras on every rank and gives every rank the same similarity)
  if (opts->apply && pt_ref && h->world > 1)
    return fail(BA_ERR_INVALID, "ba_align: apply = 1 with pt_ref on a multi-rank handle (world %d): every rank would estimate its "
                                "own similarity from its shard's points and the replicated cameras would differ; align with "
                                "apply = 0 and pass every rank the same similarity (ba_transform), or give cam_ref alone", h->world);
  if (opts->apply && any_prior(h)) return fail(BA_ERR_STATE, kSimPriors, "ba_align with apply = 1");
  const int Nc = h->Nc, Np = h->Np;
  const int n_cam = cam_ref ? Nc : 0, n_pt = pt_ref ? Np : 0;
  const size_t n = (size_t)n_cam + (size_t)n_pt;
  if (n > 0x7fffffffULL) return fail(BA_ERR_INVALID, "ba_align: too many correspondences");
  // references and weights in correspondence order (cameras, then points); a row without a reference is uploaded as it is
  // (it may hold NaN) and never enters a sum
  std::vector<double> bw(4 * std::max<size_t>(n, 1));
  double* hb = bw.data();
  double* hw = hb + 3 * n;
  int n_used = 0;
  for (int part = 0; part < 2; ++part) {
    const double* ref = part ? pt_ref : cam_ref;
    const double* w = part ? pt_w : cam_w;
    const int m = part ? n_pt : n_cam, off = part ? n_cam : 0;
    if (!ref) continue;
    memcpy(hb + 3 * (size_t)off, ref, 3 * (size_t)m * sizeof(double));
    for (int i = 0; i < m; ++i) {
      const double wi = w ? w[i] : 1.0;
      if (!std::isfinite(wi) || wi < 0) return fail(BA_ERR_INVALID, "ba_align: %s weight %d is negative or not finite", part ? "point" : "camera", i);
      hw[off + i] = wi;
      n_used += wi > 0;
    }
  }
  const double nan = std::nan("");
  memset(out, 0, sizeof *out);
  out->sim.s = 1.0;
  out->sim.R[0] = out->sim.R[4] = out->sim.R[8] = 1.0;
  out->rms = out->max = nan;
  out->n_used = n_used;
  if (n_used < 3) {
    out->status = BA_ALIGN_TOO_FEW;
    if (cam_err) for (int i = 0; i < n_cam; ++i) cam_err[i] = nan;
    if (pt_err) for (int i = 0; i < n_pt; ++i) pt_err[i] = nan;
    return BA_OK;
  }
  if (set_device(h)) return BA_ERR_HIP;
  const int nn = (int)n;
  const int nblk = std::min((nn + SIM_THREADS - 1) / SIM_THREADS, SIM_MAX_BLOCKS);      // from the correspondence count alone
  HIPCHECK(h->sim_buf.alloc(9 * n));
  HIPCHECK(h->sim_part.alloc((size_t)SIM_PART * SIM_MAX_BLOCKS));
  HIPCHECK(h->sim_rec.alloc(1));
  double* const a = h->sim_buf.p;
  double* const b = a + 3 * n;
  double* const w = b + 3 * n;
  double* const u = w + n;
  double* const err = u + n;
  HIPCHECK(hipMemcpyAsync(b, hb, 4 * n * sizeof(double), hipMemcpyHostToDevice, h->stream));
  SimRec rec = {};
  rec.s = 1.0;
  rec.R[0] = rec.R[4] = rec.R[8] = 1.0;
  rec.status = SIM_OK;
  BA_LAUNCH(k_sim_set, dim3(1), dim3(64), 0, h->stream, rec, h->sim_rec.p);
  BA_LAUNCH(k_sim_gather, dim3((nn + 255) / 256), dim3(256), 0, h->stream, (const double*)h->cs[h->cur].p, n_cam,
            (const double*)h->ptab[h->cur].p, (const int*)h->slot.p, n_pt, a);
  // every round on the stream, no host synchronisation in between: the fold kernels leave the similarity and the status
  // in the device record, which the next pass reads
  const double inv_f2 = 1.0 / (opts->f_scale * opts->f_scale);
  for (int round = 0; round <= opts->iters; ++round) {
    BA_LAUNCH(k_sim_pass_a, dim3(nblk), dim3(SIM_THREADS), 0, h->stream, (const SimRec*)h->sim_rec.p, nn, (const double*)a,
              (const double*)b, (const double*)w, round > 0 ? 1 : 0, (int)opts->loss, inv_f2, u, h->sim_part.p);
    BA_LAUNCH(k_sim_centroid, dim3(1), dim3(64), 0, h->stream, (const double*)h->sim_part.p, nblk, h->sim_rec.p);
    BA_LAUNCH(k_sim_pass_b, dim3(nblk), dim3(SIM_THREADS), 0, h->stream, (const SimRec*)h->sim_rec.p, nn, (const double*)a,
              (const double*)b, (const double*)u, h->sim_part.p);
    BA_LAUNCH(k_sim_solve, dim3(1), dim3(64), 0, h->stream, (const double*)h->sim_part.p, nblk, opts->with_scale ? 1 : 0, h->sim_rec.p);
  }
  BA_LAUNCH(k_sim_errors, dim3(nblk), dim3(SIM_THREADS), 0, h->stream, (const SimRec*)h->sim_rec.p, nn, (const double*)a,
            (const double*)b, (const double*)w, err, h->sim_part.p);
  BA_LAUNCH(k_sim_finish, dim3(1), dim3(64), 0, h->stream, (const double*)h->sim_part.p, nblk, n_used, h->sim_rec.p);
  HIPCHECK(hipMemcpyAsync(&rec, h->sim_rec.p, sizeof rec, hipMemcpyDeviceToHost, h->stream));
  if (cam_err && n_cam > 0) HIPCHECK(hipMemcpyAsync(cam_err, err, (size_t)n_cam * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (pt_err && n_pt > 0) HIPCHECK(hipMemcpyAsync(pt_err, err + n_cam, (size_t)n_pt * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  std::vector<double> held_pts;
  if (opts->apply)      // reads the similarity from the device record; a status that is not OK makes the kernels no-ops
    if (int rc = launch_transform(h, &held_pts)) return rc;
  BA_SYNC(h);
  if (opts->apply && rec.status == SIM_OK) commit_transform(h, held_pts);   // else the handle stays exactly as found
  out->status = rec.status;
  out->sim.s = rec.s;
  memcpy(out->sim.R, rec.R, sizeof rec.R);
  memcpy(out->sim.t, rec.t, sizeof rec.t);
  out->rms = rec.rms;
  out->max = rec.max;
  return BA_OK;
}

// ------------------------------------------------------------------------------------------------- pose graph
// ba_pose_graph, ba_pose_graph_system (csrc/ba_posegraph.hpp).  Local to the rank: no collective.  Own buffers and own trace:
// a resident problem, its parameters and the trace of its last solve stay as they are.
extern "C" int ba_default_posegraph_options(ba_posegraph_options* o) {
  if (!o) return fail(BA_ERR_INVALID, "null options");
  memset(o, 0, sizeof *o);
  o->loss = BA_LOSS_LINEAR;
  o->max_iters = 50;
  o->f_scale = 1.0;
  o->ftol = 1e-5; o->xtol = 1e-5; o->gtol = 1e-8;      // ba_default_options' values
  o->initial_lambda = 1e-4;
  o->pcg_tol = 0.1;
  o->pcg_max_iters = 200;
  o->pcg_min_iters = 1;
  o->with_scale = 1;
  return BA_OK;
}

// the similarity rvec | t | s of row `idx` of `what` (poses or meas): finite, s > 0, |rvec| <= pi, s == 1 without scale
static int pg_check_sim(const char* fn, const char* what, int idx, const double* v, bool with_scale) {
  for (int q = 0; q < 7; ++q)
    if (!std::isfinite(v[q])) return fail(BA_ERR_INVALID, "%s: %s[%d]: non-finite entry", fn, what, idx);
  if (!(v[6] > 0)) return fail(BA_ERR_INVALID, "%s: %s[%d]: the scale s must be positive", fn, what, idx);
  if (std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]) > M_PI + 1e-9)
    return fail(BA_ERR_INVALID, "%s: %s[%d]: |rvec| exceeds pi", fn, what, idx);
  if (!with_scale && v[6] != 1.0) return fail(BA_ERR_INVALID, "%s: %s[%d]: with_scale = 0 needs every scale s to be exactly 1", fn, what, idx);
  return BA_OK;
}
static int pg_validate(const char* fn, const ba_handle* h, int n, const double* poses, int m, const int32_t* ei, const int32_t* ej,
                       const double* meas, const double* info, const ba_posegraph_options* o) {
  if (!h || !o) return fail(BA_ERR_INVALID, "null argument");
  if (n < 0) return fail(BA_ERR_INVALID, "%s: n must not be negative", fn);
  if (m < 0) return fail(BA_ERR_INVALID, "%s: m must not be negative", fn);
  if ((n > 0 && !poses) || (m > 0 && (!ei || !ej || !meas))) return fail(BA_ERR_INVALID, "%s: null array", fn);
  if (!loss_valid(o->loss)) return fail(BA_ERR_INVALID, "%s: unknown loss %d", fn, o->loss);
  if (!(o->f_scale > 0) || !std::isfinite(o->f_scale)) return fail(BA_ERR_INVALID, "%s: f_scale must be positive", fn);
  if (o->max_iters < 0) return fail(BA_ERR_INVALID, "%s: max_iters must not be negative", fn);
  if (o->pcg_max_iters < 0) return fail(BA_ERR_INVALID, "%s: pcg_max_iters must not be negative", fn);
  if (o->pcg_min_iters < 0) return fail(BA_ERR_INVALID, "%s: pcg_min_iters must not be negative", fn);
  if (!(o->ftol >= 0)) return fail(BA_ERR_INVALID, "%s: ftol must not be negative", fn);
  if (!(o->xtol >= 0)) return fail(BA_ERR_INVALID, "%s: xtol must not be negative", fn);
  if (!(o->gtol >= 0)) return fail(BA_ERR_INVALID, "%s: gtol must not be negative", fn);
  if (!(o->pcg_tol >= 0)) return fail(BA_ERR_INVALID, "%s: pcg_tol must not be negative", fn);
  if (!(o->initial_lambda > 0) || !std::isfinite(o->initial_lambda)) return fail(BA_ERR_INVALID, "%s: initial_lambda must be positive", fn);
  if (o->reserved0 != 0) return fail(BA_ERR_INVALID, "%s: reserved0 must be 0", fn);
  const bool ws = o->with_scale != 0;
  for (int k = 0; k < n; ++k)
    if (int rc = pg_check_sim(fn, "poses", k, poses + 7 * (size_t)k, ws)) return rc;
  for (int e = 0; e < m; ++e) {
    if (ei[e] < 0 || ei[e] >= n) return fail(BA_ERR_INVALID, "%s: edge_i[%d] = %d outside 0 .. %d", fn, e, ei[e], n - 1);
    if (ej[e] < 0 || ej[e] >= n) return fail(BA_ERR_INVALID, "%s: edge_j[%d] = %d outside 0 .. %d", fn, e, ej[e], n - 1);
    if (ei[e] == ej[e]) return fail(BA_ERR_INVALID, "%s: edge %d: edge_i == edge_j (%d)", fn, e, ei[e]);
    if (int rc = pg_check_sim(fn, "meas", e, meas + 7 * (size_t)e, ws)) return rc;
    if (!info) continue;
    const double* I = info + 49 * (size_t)e;
    double big = 0.0;
    for (int q = 0; q < 49; ++q) {
      if (!std::isfinite(I[q])) return fail(BA_ERR_INVALID, "%s: info[%d]: non-finite entry", fn, e);
      big = std::max(big, std::fabs(I[q]));
    }
    double packed[28];
    for (int a = 0; a < 7; ++a)
      for (int b = a; b < 7; ++b) {
        if (std::fabs(I[7 * a + b] - I[7 * b + a]) > 1e-12 * big) return fail(BA_ERR_INVALID, "%s: info[%d] is not symmetric", fn, e);
        packed[UT(7, a, b)] = I[7 * a + b];
      }
    if (big == 0.0) continue;
    double lo, hi;
    sym_eig_range(packed, 7, &lo, &hi);
    if (lo < -1e-12 * hi || !(hi > 0.0))
      return fail(BA_ERR_INVALID, "%s: info[%d] is not positive semidefinite (eigenvalues %g .. %g)", fn, e, lo, hi);
  }
  return BA_OK;
}

struct PgPlan {
  PgGraph G;
  double* poses[2];
  int nbe, nbn, nbt, nbs;          // workgroups: edge passes, nodes that are no hubs, those plus the hubs, the step
};
// incidence lists, masks, hubs; every array uploaded; the device's view filled in
static int pg_prepare(ba_handle* h, int n, const double* poses, int m, const int32_t* ei, const int32_t* ej, const double* meas,
                      const double* info, const uint8_t* held, const ba_posegraph_options* o, bool want_e, PgPlan* P) {
  std::vector<int> iv((size_t)2 * m + (n + 1) + (size_t)2 * m + n);
  int* hei = iv.data();
  int* hej = hei + m;
  int* off = hej + m;
  int* inc = off + n + 1;
  int* mask = inc + 2 * (size_t)m;
  memcpy(hei, ei, (size_t)m * sizeof(int));
  memcpy(hej, ej, (size_t)m * sizeof(int));
  std::fill(off, off + n + 1, 0);
  for (int e = 0; e < m; ++e) { off[ei[e] + 1]++; off[ej[e] + 1]++; }
  for (int k = 0; k < n; ++k) off[k + 1] += off[k];
  std::vector<int> fill(off, off + n);
  for (int e = 0; e < m; ++e) { inc[fill[ei[e]]++] = 2 * e; inc[fill[ej[e]]++] = 2 * e + 1; }      // by edge number; low bit: the node is j
  std::vector<int> hubs;
  for (int k = 0; k < n; ++k) {
    const int deg = off[k + 1] - off[k];
    mask[k] = ((held && held[k]) || deg == 0) ? 0x7f : (o->with_scale ? 0 : 0x40);
    if (deg > PG_HUB_MIN) { hubs.push_back(k); }
  }
  const int nh = (int)hubs.size();
  std::vector<int> hub_len(nh);
  for (int q = 0; q < nh; ++q) hub_len[q] = pg_chunk_len(off[hubs[q] + 1] - off[hubs[q]]);
  P->nbe = std::min((m + PG_TEAMS - 1) / PG_TEAMS, PG_MAX_BLOCKS);
  P->nbn = std::min((n + PG_TEAMS - 1) / PG_TEAMS, PG_MAX_BLOCKS);
  P->nbt = P->nbn + nh;
  P->nbs = std::min((n + PG_THREADS - 1) / PG_THREADS, PG_MAX_BLOCKS);
  const size_t nn = (size_t)n, mm = (size_t)m, nbt = (size_t)P->nbt;
  Scratch& sc = h->scratch;
  HIPCHECK(sc.begin(h->stream));
  PgGraph& G = P->G;
  memset(&G, 0, sizeof G);
  G.n = n; G.m = m;
  // (pageable sources: the copies have left the host arrays when the calls return)
  HIPCHECK(sc.take(7 * nn, &P->poses[0], &P->poses[1])); HIPCHECK(sc.put(h->stream, 7 * mm, meas, &G.meas));
  if (info) HIPCHECK(sc.put(h->stream, 49 * mm, info, &G.info));
  HIPCHECK(hipMemcpyAsync(P->poses[0], poses, 7 * nn * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHECK(sc.take(49 * mm, &G.At, &G.Bt, &G.WA, &G.WB)); HIPCHECK(sc.take(8 * mm, &G.We, &G.u)); HIPCHECK(sc.take(mm, &G.chi2, &G.wgt));
  if (want_e) HIPCHECK(sc.take(7 * mm, &G.e));                 // (the residuals leave the device for the inspection entry only)
  HIPCHECK(sc.take(49 * nn, &G.Hd, &G.Minv)); HIPCHECK(sc.take(8 * nn, &G.g, &G.D, &G.x, &G.r, &G.z, &G.p, &G.q));
  HIPCHECK(sc.take(2 * PG_MAX_BLOCKS, &G.part_cost)); HIPCHECK(sc.take(nbt, &G.part_g, &G.part_rz, &G.part_pq)); HIPCHECK(sc.take(5 * PG_MAX_BLOCKS, &G.part_step));
  HIPCHECK(sc.put(h->stream, iv.size(), iv.data(), &G.ei));     // ei | ej | inc_off | inc | mask, as iv holds them
  G.ej = G.ei + m; G.inc_off = G.ei + 2 * mm; G.inc = G.inc_off + n + 1; G.mask = G.inc + 2 * mm;
  int* dhub;
  HIPCHECK(sc.take(2 * (size_t)nh + 1, &dhub));                 // hub_node | hub_len | bad
  G.hub_node = dhub; G.hub_len = dhub + nh; G.bad = dhub + 2 * nh;
  HIPCHECK(sc.take(2, &G.st)); HIPCHECK(sc.take(1, &G.rec));
  G.n_hubs = nh; G.nb_nodes = P->nbn;
  G.hub_teams = (h->debug_pg_splits > 0) ? std::min(h->debug_pg_splits, PG_TEAMS) : PG_TEAMS;
  hubs.insert(hubs.end(), hub_len.begin(), hub_len.end());
  hubs.push_back(0);                                            // the `bad` word
  HIPCHECK(hipMemcpyAsync(dhub, hubs.data(), hubs.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHECK(hipStreamSynchronize(h->stream));                    // the host vectors above go out of scope
  return BA_OK;
}
// linearisation at parameter set `which`: edge records, node blocks, gradient; cost and max |g| into the record
static void pg_linearize(ba_handle* h, const PgPlan& P, int which, int loss, double inv_f2) {
  BA_LAUNCH(k_pg_edge<true>, dim3(P.nbe), dim3(PG_THREADS), 0, h->stream, P.G, (const double*)P.poses[which], loss, inv_f2);
  BA_LAUNCH(k_pg_node_lin, dim3(P.nbt), dim3(PG_THREADS), 0, h->stream, P.G);
  BA_LAUNCH(k_pg_fold, dim3(1), dim3(64), 0, h->stream, P.G, P.nbe, P.nbt, 0, -1, 0, 0.0, 0);
}
static int pg_read_rec(ba_handle* h, const PgPlan& P, PgRec* rec) {
  HIPCHECK(hipMemcpyAsync(rec, P.G.rec, sizeof *rec, hipMemcpyDeviceToHost, h->stream));
  BA_SYNC(h);
  return BA_OK;
}

extern "C" int ba_pose_graph(ba_handle* h, int32_t n, const double* poses, int32_t m, const int32_t* edge_i, const int32_t* edge_j,
                             const double* meas, const double* info, const uint8_t* held, const ba_posegraph_options* opts,
                             double* poses_out, ba_summary* sum, double* edge_chi2, double* edge_weight) {
  if (int rc = pg_validate("ba_pose_graph", h, n, poses, m, edge_i, edge_j, meas, info, opts)) return rc;
  ba_summary local;
  if (!sum) sum = &local;
  memset(sum, 0, sizeof *sum);
  h->pg_trace.clear();
  if (n == 0 || m == 0) {          // nothing to adjust
    if (poses_out && n > 0) memcpy(poses_out, poses, 7 * (size_t)n * sizeof(double));
    sum->status = 3;
    sum->final_lambda = opts->initial_lambda;
    return BA_OK;
  }
  if (set_device(h)) return BA_ERR_HIP;
  const double t_begin = now_s();
  PgPlan P;
  if (int rc = pg_prepare(h, n, poses, m, edge_i, edge_j, meas, info, held, opts, false, &P)) return rc;
  const int loss = opts->loss;
  const double fs2 = opts->f_scale * opts->f_scale, inv_f2 = 1.0 / fs2, tol2 = opts->pcg_tol * opts->pcg_tol;
  LmState st(opts->initial_lambda);
  PgRec rec;
  int cur = 0;
  pg_linearize(h, P, cur, loss, inv_f2);
  if (int rc = pg_read_rec(h, P, &rec)) return rc;
  st.sse = rec.sse; st.cost = 0.5 * fs2 * rec.rho;
  sum->initial_sse = st.sse; sum->initial_cost = st.cost;
  if (!std::isfinite(st.cost)) return fail(BA_ERR_NUMERIC, "ba_pose_graph: non-finite cost at the initial poses");
  st.need_linearize = false;
  bool fresh = true;               // the gradient in `rec` has not met the gtol test yet (ba_solve: fresh linearisations only, gtol > 0 only)
  while (st.it < opts->max_iters && !st.stop) {
    const double t0 = now_s();
    if (st.need_linearize) {
      pg_linearize(h, P, cur, loss, inv_f2);
      if (int rc = pg_read_rec(h, P, &rec)) return rc;
      st.need_linearize = false;
      fresh = true;
    }
    if (fresh) {
      fresh = false;
      if (!std::isfinite(rec.gmax) || rec.gmax >= 1e308) return fail(BA_ERR_NUMERIC, "ba_pose_graph: non-finite gradient at LM iteration %d", st.it);
      if (opts->gtol > 0 && rec.gmax <= opts->gtol) { st.status = 3; break; }
    }
    const double t1 = now_s();
    sum->seconds_linearize += t1 - t0;
    // ---- the inner solve: three launches per iteration, the verdicts on the device; the host looks once per batch
    BA_LAUNCH(k_pg_damp, dim3(P.nbn), dim3(PG_THREADS), 0, h->stream, P.G, st.lambda);
    int k = 0, batch = 4;
    PgRec pr;
    while (true) {
      for (int b = 0; b < batch && k < opts->pcg_max_iters; ++b, ++k) {
        BA_LAUNCH(k_pg_pcg_edge, dim3(P.nbe), dim3(PG_THREADS), 0, h->stream, P.G, k, P.nbn, tol2, (int)opts->pcg_min_iters);
        BA_LAUNCH(k_pg_pcg_node, dim3(P.nbt), dim3(PG_THREADS), 0, h->stream, P.G, k, st.lambda);
        BA_LAUNCH(k_pg_pcg_step, dim3(P.nbn), dim3(PG_THREADS), 0, h->stream, P.G, k, P.nbt);
      }
      BA_LAUNCH(k_pg_fold, dim3(1), dim3(64), 0, h->stream, P.G, P.nbe, 0, 0, k, P.nbn, tol2, (int)opts->pcg_min_iters);
      if (int rc = pg_read_rec(h, P, &pr)) return rc;
      if (pr.bad) return fail(BA_ERR_NUMERIC, "ba_pose_graph: a damped diagonal block is not positive definite (LM iteration %d)", st.it);
      if (pr.pcg.done || k >= opts->pcg_max_iters) break;
      batch = std::min(2 * batch, 32);
    }
    const int pcg_iters = pr.pcg.done ? pr.pcg.iters : k;
    sum->pcg_iterations += pcg_iters;
    if (pcg_iters >= opts->pcg_max_iters) st.lam_floor = std::max(st.lam_floor, 3.0 * st.lambda);      // ba_solve's cap-aware damping
    const double t2 = now_s();
    sum->seconds_pcg += t2 - t1;
    // ---- step, trial cost, the LM sums
    BA_LAUNCH(k_pg_step, dim3(P.nbs), dim3(PG_THREADS), 0, h->stream, P.G, (const double*)P.poses[cur], P.poses[1 - cur]);
    BA_LAUNCH(k_pg_edge<false>, dim3(P.nbe), dim3(PG_THREADS), 0, h->stream, P.G, (const double*)P.poses[1 - cur], loss, inv_f2);
    BA_LAUNCH(k_pg_fold, dim3(1), dim3(64), 0, h->stream, P.G, P.nbe, 0, P.nbs, -1, 0, 0.0, 0);
    PgRec tr;
    if (int rc = pg_read_rec(h, P, &tr)) return rc;
    // ---- verdict: ba_solve's rules (apply_verdict, lm_decide)
    const double cost_new = 0.5 * fs2 * tr.rho, sse_new = tr.sse;
    const double model = 0.5 * (st.lambda * tr.dDd - tr.gTd + tr.dr);
    const double rho = model > 0 ? (st.cost - cost_new) / model : -1.0;
    const bool accept = rho > 0 && std::isfinite(cost_new);
    const int it = ++st.it;
    ba_iter_record r = {};
    r.iteration = it; r.accepted = accept ? 1 : 0; r.pcg_iterations = pcg_iters;
    r.cost = st.cost; r.cost_trial = cost_new; r.sse_trial = sse_new; r.lambda = st.lambda; r.gain_ratio = rho;
    r.step_norm = std::sqrt(tr.step2); r.seconds = now_s() - t0;
    h->pg_trace.push_back(r);
    if (accept) {
      const double dcost = st.cost - cost_new;
      cur = 1 - cur;
      st.cost = cost_new; st.sse = sse_new;
      sum->accepted++;
      const double t = 2.0 * rho - 1.0;
      st.lambda = std::max(std::max(st.lambda * std::max(1.0 / 3.0, 1.0 - t * t * t), 1e-12), st.lam_floor);
      st.nu = 2.0;
      st.need_linearize = true;
      if (dcost <= opts->ftol * st.cost) { st.status = 1; st.stop = true; }
    } else {
      if (!std::isfinite(cost_new) && st.lambda >= 1e12)
        return fail(BA_ERR_NUMERIC, "ba_pose_graph: non-finite cost at the trial point of LM iteration %d with the damping at its cap", it);
      st.lambda = std::min(st.lambda * st.nu, 1e12);
      st.nu *= 2.0;
    }
    if (!st.stop && std::sqrt(tr.step2) <= opts->xtol * (opts->xtol + std::sqrt(tr.x2))) { st.status = 2; st.stop = true; }
    sum->seconds_update += now_s() - t2;
  }
  // chi2_e and w_e at the returned poses
  BA_LAUNCH(k_pg_edge<false>, dim3(P.nbe), dim3(PG_THREADS), 0, h->stream, P.G, (const double*)P.poses[cur], loss, inv_f2);
  if (poses_out) HIPCHECK(hipMemcpyAsync(poses_out, P.poses[cur], 7 * (size_t)n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (edge_chi2) HIPCHECK(hipMemcpyAsync(edge_chi2, P.G.chi2, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (edge_weight) HIPCHECK(hipMemcpyAsync(edge_weight, P.G.wgt, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  BA_SYNC(h);
  return finish_solve(sum, st, t_begin);
}

extern "C" int ba_pose_graph_trace(ba_handle* h, ba_iter_record* out, int32_t capacity, int32_t* n) {
  if (!h || !n) return fail(BA_ERR_INVALID, "null argument");
  *n = (int32_t)h->pg_trace.size();
  if (out)
    for (int i = 0; i < *n && i < capacity; ++i) out[i] = h->pg_trace[i];
  return BA_OK;
}

extern "C" int ba_pose_graph_system(ba_handle* h, int32_t n, const double* poses, int32_t m, const int32_t* edge_i, const int32_t* edge_j,
                                    const double* meas, const double* info, const uint8_t* held, const ba_posegraph_options* opts,
                                    double lambda, double* e, double* A, double* B, double* H, double* g) {
  if (int rc = pg_validate("ba_pose_graph_system", h, n, poses, m, edge_i, edge_j, meas, info, opts)) return rc;
  if (7 * (long long)n > 4096) return fail(BA_ERR_INVALID, "ba_pose_graph_system: n = %d: the dense system is offered up to 7 n = 4096", n);
  if (!(lambda >= 0)) return fail(BA_ERR_INVALID, "ba_pose_graph_system: lambda must not be negative");
  if (n == 0 || m == 0) return fail(BA_ERR_INVALID, "ba_pose_graph_system: n and m must be positive");
  if (set_device(h)) return BA_ERR_HIP;
  PgPlan P;
  if (int rc = pg_prepare(h, n, poses, m, edge_i, edge_j, meas, info, held, opts, true, &P)) return rc;
  pg_linearize(h, P, 0, opts->loss, 1.0 / (opts->f_scale * opts->f_scale));
  const size_t N = 7 * (size_t)n, mm = (size_t)m;
  if (H) {
    double* dense;
    HIPCHECK(h->scratch.take(N * N, &dense));
    BA_LAUNCH(k_pg_dense, dim3((unsigned)((N * N + PG_THREADS - 1) / PG_THREADS)), dim3(PG_THREADS), 0, h->stream, P.G, lambda, dense);
    HIPCHECK(hipMemcpyAsync(H, dense, N * N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  }
  std::vector<double> at, bt, g8;
  if (e) HIPCHECK(hipMemcpyAsync(e, P.G.e, 7 * mm * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (A) { at.resize(49 * mm); HIPCHECK(hipMemcpyAsync(at.data(), P.G.At, 49 * mm * sizeof(double), hipMemcpyDeviceToHost, h->stream)); }
  if (B) { bt.resize(49 * mm); HIPCHECK(hipMemcpyAsync(bt.data(), P.G.Bt, 49 * mm * sizeof(double), hipMemcpyDeviceToHost, h->stream)); }
  if (g) { g8.resize(8 * (size_t)n); HIPCHECK(hipMemcpyAsync(g8.data(), P.G.g, 8 * (size_t)n * sizeof(double), hipMemcpyDeviceToHost, h->stream)); }
  BA_SYNC(h);
  for (size_t q = 0; q < mm; ++q)          // the device keeps the transposes
    for (int a = 0; a < 7; ++a)
      for (int c = 0; c < 7; ++c) {
        if (A) A[49 * q + 7 * a + c] = at[49 * q + 7 * c + a];
        if (B) B[49 * q + 7 * a + c] = bt[49 * q + 7 * c + a];
      }
  if (g)
    for (int k = 0; k < n; ++k)
      for (int c = 0; c < 7; ++c) g[7 * (size_t)k + c] = g8[8 * (size_t)k + c];
  return BA_OK;
}

// ------------------------------------------------------------------------------------------------- place recognition
// ba_vocab_train / ba_vocab_set / ba_vocab_get / ba_bow_transform / ba_bow_score (csrc/ba_bow.hpp).  Need no problem.
static_assert(sizeof(ba_vocab_options) == 24, "ba_vocab_options (include/ba_hip.h)");
static_assert(BW_MAX_SET >= 65536 && BW_CHUNK % 64 == 0, "a set holds at least ORB's most features");
extern "C" int ba_default_vocab_options(ba_vocab_options* o) {
  if (!o) return fail(BA_ERR_INVALID, "null argument");
  memset(o, 0, sizeof *o);
  o->branching = 10;
  o->levels = 6;
  o->iters = 10;
  return BA_OK;
}
// The tree becomes the handle's vocabulary: words numbered, depth measured, device arrays uploaded
static int vocab_install(ba_handle* h, BowVocab& v, int branching, int levels) {
  const size_t nn = v.child0.size(), W = (size_t)v.desc_bytes / 8;
  v.word_of_node.assign(nn, -1);
  v.n_words = 0;
  for (size_t n = 0; n < nn; ++n)
    if (v.child0[n] < 0) v.word_of_node[n] = v.n_words++;
  v.branching = branching;
  v.levels = levels;
  HIPCHECK(h->bw_child0.alloc(nn)); HIPCHECK(h->bw_nchild.alloc(nn)); HIPCHECK(h->bw_wordof.alloc(nn));
  HIPCHECK(h->bw_idf.alloc((size_t)v.n_words)); HIPCHECK(h->bw_ndesc.alloc(nn * W));
  HIPCHECK(hipMemcpyAsync(h->bw_child0.p, v.child0.data(), nn * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHECK(hipMemcpyAsync(h->bw_nchild.p, v.n_child.data(), nn * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHECK(hipMemcpyAsync(h->bw_wordof.p, v.word_of_node.data(), nn * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHECK(hipMemcpyAsync(h->bw_idf.p, v.idf_q.data(), (size_t)v.n_words * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHECK(hipMemcpyAsync(h->bw_ndesc.p, v.node_desc.data(), nn * W * 8, hipMemcpyHostToDevice, h->stream));
  HIPCHECK(hipStreamSynchronize(h->stream));       // (v's arrays may move below)
  h->vocab = std::move(v);
  return BA_OK;
}
template <int W>
static void launch_vocab_assign(ba_handle* h, unsigned grid, const VocabArgs& a) {
  BA_LAUNCH(k_vocab_assign<W>, dim3(grid), dim3(BW_THREADS), 0, h->stream, a);
}
template <int W>
static void launch_vocab_vote(ba_handle* h, unsigned grid, const VocabArgs& a) {
  BA_LAUNCH(k_vocab_vote<W>, dim3(grid), dim3(BW_THREADS), 0, h->stream, a);
}
template <int W>
static void launch_bow_descend(ba_handle* h, unsigned grid, const BowArgs& a) {
  BA_LAUNCH(k_bow_descend<W>, dim3(grid), dim3(BW_THREADS), 0, h->stream, a);
}
extern "C" int ba_vocab_train(ba_handle* h, int32_t desc_bytes, int32_t n_sets, const int64_t* set_off, const uint8_t* desc,
                              const ba_vocab_options* opts, int32_t* train_word, int32_t* n_nodes, int32_t* n_words) {
  if (!h || !opts) return fail(BA_ERR_INVALID, "null argument");
  if (int rc = desc_sets_check("ba_vocab_train", desc_bytes, n_sets, set_off, desc)) return rc;
  if (set_off[n_sets] >= (1LL << BW_ROW_BITS))
    return fail(BA_ERR_INVALID, "ba_vocab_train: rows %lld is not below 2^%d", (long long)set_off[n_sets], BW_ROW_BITS);
  if (opts->branching < 2 || opts->branching > BW_MAX_K) return fail(BA_ERR_INVALID, "ba_vocab_train: branching %d is outside 2 .. %d", opts->branching, BW_MAX_K);
  if (opts->levels < 1 || opts->levels > BW_MAX_LEVELS) return fail(BA_ERR_INVALID, "ba_vocab_train: levels %d is outside 1 .. %d", opts->levels, BW_MAX_LEVELS);
  if (opts->iters < 1) return fail(BA_ERR_INVALID, "ba_vocab_train: iters %d is below 1", opts->iters);
  if (opts->min_split != 0 && opts->min_split < 2) return fail(BA_ERR_INVALID, "ba_vocab_train: min_split %d is neither 0 nor at least 2", opts->min_split);
  const int k = opts->branching, rows = (int)set_off[n_sets], W = desc_bytes / 8, BITS = 64 * W;
  const int min_split = opts->min_split == 0 ? 2 * k : opts->min_split;
  if (set_device(h)) return BA_ERR_HIP;
  BowVocab v;
  v.desc_bytes = desc_bytes;
  v.child0.assign(1, -1);
  v.n_child.assign(1, 0);
  v.node_desc.assign((size_t)desc_bytes, 0);
  std::vector<int> count(1, rows), node_of_row((size_t)rows, 0);
  if (rows >= min_split) {
    const size_t nr = (size_t)rows;
    const unsigned row_grid = (unsigned)((nr + BW_THREADS - 1) / BW_THREADS);
    Scratch& sc = h->scratch;
    HIPCHECK(sc.begin(h->stream));
    VocabArgs a = {};
    HIPCHECK(sc.put(h->stream, nr * W, desc, &a.desc)); HIPCHECK(sc.take(nr, &a.perm, &a.node, &a.slot));
    const Scratch::Mark levels_from = sc.mark();      // what a level takes holds nothing across levels
    a.rows = rows; a.k = k; a.words = W;
    {
      std::vector<int> iota(nr);
      for (size_t r = 0; r < nr; ++r) iota[r] = (int)r;
      HIPCHECK(hipMemcpyAsync(a.perm, iota.data(), nr * sizeof(int), hipMemcpyHostToDevice, h->stream));
      HIPCHECK(hipMemsetAsync(a.node, 0, nr * sizeof(int), h->stream));
      HIPCHECK(hipMemsetAsync(a.slot, 0xff, nr * sizeof(int), h->stream));
      HIPCHECK(hipStreamSynchronize(h->stream));
    }
    int lvl_begin = 0, lvl_n = 1;
    std::vector<unsigned char> open;
    std::vector<int> size, child, cursor;
    std::vector<unsigned long long> centre;
    for (int d = 0; d < opts->levels && lvl_n > 0; ++d) {
      open.assign((size_t)lvl_n, 0);
      bool any = false;
      for (int n = 0; n < lvl_n; ++n) any |= (open[n] = count[lvl_begin + n] >= min_split) != 0;
      if (!any) break;
      const size_t ns = (size_t)lvl_n * k, n_cursor = v.child0.size() + ns;
      sc.rewind(levels_from);
      int* d_child;
      HIPCHECK(sc.take(ns, &a.size, &d_child)); HIPCHECK(sc.take(1, &a.changed)); HIPCHECK(sc.take(n_cursor, &a.cursor)); HIPCHECK(sc.take(ns * BITS, &a.votes));
      HIPCHECK(sc.take(ns, &a.seed_key)); HIPCHECK(sc.take(ns * W, &a.centre)); HIPCHECK(sc.put(h->stream, (size_t)lvl_n, open.data(), &a.open)); HIPCHECK(sc.take(ns, &a.usable));
      a.lvl_begin = lvl_begin; a.lvl_n = lvl_n; a.child = d_child;
      for (int j = 0; j < k; ++j) a.pre[j] = bw_mix(bw_mix(bw_mix(opts->seed + BW_GOLDEN) + (unsigned long long)d) + (unsigned long long)j);
      HIPCHECK(hipMemsetAsync(a.seed_key, 0xff, ns * 8, h->stream));
      const unsigned slot_grid = (unsigned)((ns + BW_THREADS - 1) / BW_THREADS);
      BA_LAUNCH(k_vocab_seed_key, dim3(row_grid), dim3(BW_THREADS), 0, h->stream, a);
      BA_LAUNCH(k_vocab_seed_set, dim3(slot_grid), dim3(BW_THREADS), 0, h->stream, a);
      // iters rounds of (assign, stop when nothing moved, vote, centres), then the closing assignment
      for (int it = 0; it <= opts->iters; ++it) {
        HIPCHECK(hipMemsetAsync(a.size, 0, ns * sizeof(int), h->stream));
        HIPCHECK(hipMemsetAsync(a.changed, 0, sizeof(int), h->stream));
        BA_BY_WORDS(W, launch_vocab_assign, h, row_grid, a);
        if (it == opts->iters) break;
        int changed = 0;
        HIPCHECK(hipMemcpyAsync(&changed, a.changed, sizeof(int), hipMemcpyDeviceToHost, h->stream));
        BA_SYNC(h);
        if (changed == 0) break;      // (this assignment already is the closing one: same centres, same slots, same sizes)
        HIPCHECK(hipMemsetAsync(a.votes, 0, ns * BITS * sizeof(int), h->stream));
        BA_BY_WORDS(W, launch_vocab_vote, h, row_grid, a);
        BA_LAUNCH(k_vocab_centre, dim3((unsigned)((ns * W + BW_THREADS - 1) / BW_THREADS)), dim3(BW_THREADS), 0, h->stream, a);
      }
      size.resize(ns); centre.resize(ns * W);
      HIPCHECK(hipMemcpyAsync(size.data(), a.size, ns * sizeof(int), hipMemcpyDeviceToHost, h->stream));
      HIPCHECK(hipMemcpyAsync(centre.data(), a.centre, ns * W * 8, hipMemcpyDeviceToHost, h->stream));
      BA_SYNC(h);
      // the children, breadth-first by (parent, slot)
      child.assign(ns, -1);
      const int first_new = (int)v.child0.size();
      for (int n = 0; n < lvl_n; ++n) {
        if (!open[n]) continue;
        int full = 0;
        for (int j = 0; j < k; ++j) full += size[(size_t)n * k + j] > 0;
        if (full < 2) continue;
        v.child0[lvl_begin + n] = (int)v.child0.size();
        v.n_child[lvl_begin + n] = full;
        count[lvl_begin + n] = 0;
        for (int j = 0; j < k; ++j) {
          const size_t e = (size_t)n * k + j;
          if (size[e] == 0) continue;
          child[e] = (int)v.child0.size();
          v.child0.push_back(-1);
          v.n_child.push_back(0);
          count.push_back(size[e]);
          const uint8_t* c = (const uint8_t*)(centre.data() + e * W);
          v.node_desc.insert(v.node_desc.end(), c, c + desc_bytes);
        }
      }
      const int n_new = (int)v.child0.size() - first_new;
      if (n_new == 0) break;
      cursor.assign(v.child0.size(), 0);
      for (size_t n = 0, at = 0; n < v.child0.size(); ++n) { cursor[n] = (int)at; at += (size_t)count[n]; }
      HIPCHECK(hipMemcpyAsync(d_child, child.data(), ns * sizeof(int), hipMemcpyHostToDevice, h->stream));
      HIPCHECK(hipMemcpyAsync(a.cursor, cursor.data(), cursor.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
      BA_LAUNCH(k_vocab_children, dim3(row_grid), dim3(BW_THREADS), 0, h->stream, a);
      BA_LAUNCH(k_vocab_scatter, dim3(row_grid), dim3(BW_THREADS), 0, h->stream, a);
      BA_SYNC(h);                     // (the host vectors above are reused by the next level)
      lvl_begin = first_new;
      lvl_n = n_new;
    }
    HIPCHECK(hipMemcpyAsync(node_of_row.data(), a.node, nr * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    BA_SYNC(h);
  }
  // words, the sets that reach each word, idf
  int nw = 0;
  std::vector<int> word_of((size_t)v.child0.size(), -1);
  for (size_t n = 0; n < v.child0.size(); ++n)
    if (v.child0[n] < 0) word_of[n] = nw++;
  std::vector<int> n_with((size_t)nw, 0), last((size_t)nw, -1);
  for (int32_t s = 0; s < n_sets; ++s)
    for (int64_t r = set_off[s]; r < set_off[s + 1]; ++r) {
      const int w = word_of[node_of_row[r]];
      if (train_word) train_word[r] = w;
      if (last[w] != s) { last[w] = s; ++n_with[w]; }
    }
  v.idf_q.assign((size_t)nw, 0);
  for (int w = 0; w < nw; ++w)
    if (n_with[w] > 0) v.idf_q[w] = (int32_t)std::floor(std::log((double)n_sets / (double)n_with[w]) * 4096.0 + 0.5);
  if (n_nodes) *n_nodes = (int32_t)v.child0.size();
  if (n_words) *n_words = nw;
  return vocab_install(h, v, k, opts->levels);
}

extern "C" int ba_vocab_size(ba_handle* h, int32_t* desc_bytes, int32_t* n_nodes, int32_t* n_words, int32_t* branching, int32_t* levels) {
  if (!h) return fail(BA_ERR_INVALID, "null handle");
  const BowVocab& v = h->vocab;       // (no vocabulary: every number is 0)
  if (desc_bytes) *desc_bytes = v.desc_bytes;
  if (n_nodes) *n_nodes = (int32_t)v.child0.size();
  if (n_words) *n_words = v.n_words;
  if (branching) *branching = v.branching;
  if (levels) *levels = v.levels;
  return BA_OK;
}
extern "C" int ba_vocab_get(ba_handle* h, int32_t* child0, int32_t* n_child, uint8_t* node_desc, int32_t* word_of_node, int32_t* idf_q) {
  if (!h) return fail(BA_ERR_INVALID, "null handle");
  const BowVocab& v = h->vocab;
  if (v.child0.empty()) return fail(BA_ERR_STATE, "ba_vocab_get: no vocabulary: call ba_vocab_train or ba_vocab_set first");
  if (child0) memcpy(child0, v.child0.data(), v.child0.size() * sizeof(int32_t));
  if (n_child) memcpy(n_child, v.n_child.data(), v.n_child.size() * sizeof(int32_t));
  if (node_desc) memcpy(node_desc, v.node_desc.data(), v.node_desc.size());
  if (word_of_node) memcpy(word_of_node, v.word_of_node.data(), v.word_of_node.size() * sizeof(int32_t));
  if (idf_q) memcpy(idf_q, v.idf_q.data(), v.idf_q.size() * sizeof(int32_t));
  return BA_OK;
}
extern "C" int ba_vocab_set(ba_handle* h, int32_t desc_bytes, int32_t n_nodes, const int32_t* child0, const int32_t* n_child,
                            const uint8_t* node_desc, const int32_t* idf_q) {
  if (!h) return fail(BA_ERR_INVALID, "null handle");
  if (int rc = desc_bytes_check("ba_vocab_set", desc_bytes)) return rc;
  if (n_nodes < 1) return fail(BA_ERR_INVALID, "ba_vocab_set: n_nodes %d is below 1", n_nodes);
  if (!child0 || !n_child || !node_desc || !idf_q) return fail(BA_ERR_INVALID, "ba_vocab_set: null argument");
  // breadth-first and contiguous: walking the nodes in order, the children of the inner nodes tile 1 .. n_nodes - 1 exactly
  // once, in order -- so every node but the root is the child of exactly one node, and children follow their parent
  std::vector<int> depth((size_t)n_nodes, 0);
  int next = 1, deepest = 0, widest = 0, nw = 0;
  for (int n = 0; n < n_nodes; ++n) {
    if (child0[n] < 0) {
      if (n_child[n] != 0) return fail(BA_ERR_INVALID, "ba_vocab_set: n_child[%d] = %d at a leaf (child0 < 0) must be 0", n, n_child[n]);
      ++nw;
      continue;
    }
    if (n_child[n] < 2 || n_child[n] > BW_MAX_K)
      return fail(BA_ERR_INVALID, "ba_vocab_set: n_child[%d] = %d is neither 0 nor in 2 .. %d", n, n_child[n], BW_MAX_K);
    if (child0[n] != next)
      return fail(BA_ERR_INVALID, "ba_vocab_set: child0[%d] = %d: children are not breadth-first contiguous (expected %d)", n, child0[n], next);
    if (n_child[n] > n_nodes - next)
      return fail(BA_ERR_INVALID, "ba_vocab_set: the children of node %d reach past n_nodes", n);
    if (depth[n] + 1 > BW_MAX_LEVELS) return fail(BA_ERR_INVALID, "ba_vocab_set: depth of the children of node %d exceeds %d", n, BW_MAX_LEVELS);
    for (int c = next; c < next + n_child[n]; ++c) depth[c] = depth[n] + 1;
    deepest = std::max(deepest, depth[n] + 1);
    widest = std::max(widest, n_child[n]);
    next += n_child[n];
  }
  if (next != n_nodes) return fail(BA_ERR_INVALID, "ba_vocab_set: node %d is the child of no node (every node but the root must be the child of exactly one)", next);
  for (int w = 0; w < nw; ++w) {
    if (idf_q[w] < 0) return fail(BA_ERR_INVALID, "ba_vocab_set: idf_q[%d] = %d is negative", w, idf_q[w]);
    if (idf_q[w] > BW_MAX_IDF) return fail(BA_ERR_INVALID, "ba_vocab_set: idf_q[%d] = %d is above %d", w, idf_q[w], BW_MAX_IDF);
  }
  if (set_device(h)) return BA_ERR_HIP;
  BowVocab v;
  v.desc_bytes = desc_bytes;
  v.child0.assign(child0, child0 + n_nodes);
  v.n_child.assign(n_child, n_child + n_nodes);
  v.node_desc.assign(node_desc, node_desc + (size_t)n_nodes * desc_bytes);
  v.idf_q.assign(idf_q, idf_q + nw);
  return vocab_install(h, v, widest, deepest);
}

extern "C" int ba_bow_transform(ba_handle* h, int32_t desc_bytes, int32_t n_sets, const int64_t* set_off, const uint8_t* desc,
                                int32_t weighting, int32_t* desc_word, int64_t* vec_off, int32_t* vec_word, int32_t* vec_val) {
  if (!h) return fail(BA_ERR_INVALID, "null handle");
  if (int rc = desc_sets_check("ba_bow_transform", desc_bytes, n_sets, set_off, desc)) return rc;
  if (weighting != BA_BOW_TF_IDF && weighting != BA_BOW_TF)
    return fail(BA_ERR_INVALID, "ba_bow_transform: weighting %d is neither BA_BOW_TF_IDF (0) nor BA_BOW_TF (1)", weighting);
  for (int32_t s = 0; s < n_sets; ++s)
    if (set_off[s + 1] - set_off[s] > BW_MAX_SET)
      return fail(BA_ERR_INVALID, "ba_bow_transform: set_off: set %d holds %lld descriptors, more than %d", s,
                  (long long)(set_off[s + 1] - set_off[s]), BW_MAX_SET);
  if (set_off[n_sets] > 0x7fffffffLL) return fail(BA_ERR_INVALID, "ba_bow_transform: rows %lld is above 2^31 - 1", (long long)set_off[n_sets]);
  const BowVocab& v = h->vocab;
  if (v.child0.empty()) return fail(BA_ERR_STATE, "ba_bow_transform: no vocabulary: call ba_vocab_train or ba_vocab_set first");
  if (desc_bytes != v.desc_bytes)
    return fail(BA_ERR_INVALID, "ba_bow_transform: desc_bytes %d is not the vocabulary's %d", desc_bytes, v.desc_bytes);
  if (vec_off) memset(vec_off, 0, ((size_t)n_sets + 1) * sizeof(int64_t));
  const size_t nr = (size_t)set_off[n_sets], W = (size_t)desc_bytes / 8, ns = (size_t)n_sets, nw = (size_t)v.n_words;
  if (nr == 0) return BA_OK;
  if (set_device(h)) return BA_ERR_HIP;
  const size_t batch = std::max<size_t>(1, std::min(ns, ((size_t)1 << 26) / nw));
  Scratch& sc = h->scratch;
  HIPCHECK(sc.begin(h->stream));
  BowArgs a = {};
  HIPCHECK(sc.put(h->stream, nr * W, desc, &a.desc)); HIPCHECK(sc.put(h->stream, ns + 1, set_off, &a.set_off));
  HIPCHECK(sc.take(nr, &a.word, &a.out_word, &a.out_val)); HIPCHECK(sc.take(ns, &a.nnz)); HIPCHECK(sc.take(batch * nw, &a.cnt));      // cnt: dense counts of a batch of sets
  a.child0 = h->bw_child0.p; a.n_child = h->bw_nchild.p; a.node_desc = h->bw_ndesc.p; a.word_of_node = h->bw_wordof.p; a.idf_q = h->bw_idf.p;
  a.rows = (int)nr; a.n_sets = n_sets; a.n_words = v.n_words; a.tf = weighting == BA_BOW_TF;
  BA_BY_WORDS(W, launch_bow_descend, h, (unsigned)((nr + BW_THREADS - 1) / BW_THREADS), a);
  for (size_t s0 = 0; s0 < ns; s0 += batch) {
    a.s0 = (int)s0; a.s1 = (int)std::min(ns, s0 + batch);
    const size_t n = (size_t)(set_off[a.s1] - set_off[a.s0]);
    HIPCHECK(hipMemsetAsync(a.cnt, 0, (size_t)(a.s1 - a.s0) * nw * sizeof(int), h->stream));
    if (n > 0) BA_LAUNCH(k_bow_count, dim3((unsigned)((n + BW_THREADS - 1) / BW_THREADS)), dim3(BW_THREADS), 0, h->stream, a);
    BA_LAUNCH(k_bow_vector, dim3((unsigned)(a.s1 - a.s0)), dim3(BW_THREADS), 0, h->stream, a);
  }
  std::vector<int32_t> nnz(ns), ow, ov;
  if (desc_word) HIPCHECK(hipMemcpyAsync(desc_word, a.word, nr * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHECK(hipMemcpyAsync(nnz.data(), a.nnz, ns * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  if (vec_word) { ow.resize(nr); HIPCHECK(hipMemcpyAsync(ow.data(), a.out_word, nr * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream)); }
  if (vec_val) { ov.resize(nr); HIPCHECK(hipMemcpyAsync(ov.data(), a.out_val, nr * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream)); }
  BA_SYNC(h);
  // the sets wrote from their own first row: close the gaps
  int64_t at = 0;
  for (size_t s = 0; s < ns; ++s) {
    if (vec_word) memcpy(vec_word + at, ow.data() + set_off[s], (size_t)nnz[s] * sizeof(int32_t));
    if (vec_val) memcpy(vec_val + at, ov.data() + set_off[s], (size_t)nnz[s] * sizeof(int32_t));
    at += nnz[s];
    if (vec_off) vec_off[s + 1] = at;
  }
  return BA_OK;
}

// A CSR of bag-of-words vectors as ba_bow_score takes it; `who` names the side in the message
static int bow_csr_check(const char* who, int32_t n, const int64_t* off, const int32_t* word, const int32_t* val, int32_t* max_word) {
  if (n < 0) return fail(BA_ERR_INVALID, "ba_bow_score: the number of %s vectors %d is negative", who, n);
  if (!off) return fail(BA_ERR_INVALID, "ba_bow_score: null %s offsets", who);
  if (off[0] != 0) return fail(BA_ERR_INVALID, "ba_bow_score: %s offsets must start at 0", who);
  for (int32_t i = 0; i < n; ++i)
    if (off[i + 1] < off[i]) return fail(BA_ERR_INVALID, "ba_bow_score: %s offsets decrease at vector %d", who, i);
  if (off[n] > 0x7fffffffLL) return fail(BA_ERR_INVALID, "ba_bow_score: %s entries %lld is above 2^31 - 1", who, (long long)off[n]);
  if (off[n] > 0 && (!word || !val)) return fail(BA_ERR_INVALID, "ba_bow_score: null %s words or values", who);
  for (int32_t i = 0; i < n; ++i) {
    int64_t sum = 0;
    for (int64_t e = off[i]; e < off[i + 1]; ++e) {
      if (word[e] < 0 || (e > off[i] && word[e] <= word[e - 1]))
        return fail(BA_ERR_INVALID, "ba_bow_score: the words of %s vector %d are not ascending from 0", who, i);
      if (val[e] < 0) return fail(BA_ERR_INVALID, "ba_bow_score: %s vector %d has a negative value", who, i);
      sum += val[e];
      *max_word = std::max(*max_word, word[e]);
    }
    if (sum > (1LL << 30)) return fail(BA_ERR_INVALID, "ba_bow_score: the values of %s vector %d sum to more than 2^30", who, i);
  }
  return BA_OK;
}
extern "C" int ba_bow_score(ba_handle* h, int32_t nq, const int64_t* q_off, const int32_t* q_word, const int32_t* q_val, int32_t nd,
                            const int64_t* d_off, const int32_t* d_word, const int32_t* d_val, const int32_t* db_end, int32_t top_k,
                            int32_t* top_idx, int32_t* top_score, int32_t* score) {
  if (!h) return fail(BA_ERR_INVALID, "null handle");
  if (top_k < 1 || top_k > BW_MAX_TOPK) return fail(BA_ERR_INVALID, "ba_bow_score: top_k %d is outside 1 .. %d", top_k, BW_MAX_TOPK);
  int32_t q_max = -1, d_max = -1;
  if (int rc = bow_csr_check("query", nq, q_off, q_word, q_val, &q_max)) return rc;
  if (int rc = bow_csr_check("database", nd, d_off, d_word, d_val, &d_max)) return rc;
  const size_t nqs = (size_t)nq, nds = (size_t)nd, kq = nqs * (size_t)top_k, qn = (size_t)q_off[nq], dn = (size_t)d_off[nd];
  for (size_t i = 0; i < kq; ++i) {
    if (top_idx) top_idx[i] = -1;
    if (top_score) top_score[i] = 0;
  }
  if (score) memset(score, 0, nqs * nds * sizeof(int32_t));
  if (qn == 0 || dn == 0) return BA_OK;        // no common word anywhere: every output is already well-formed
  const int chunk = h->debug_bow_chunk > 0 ? std::min(h->debug_bow_chunk, BW_CHUNK) : BW_CHUNK;
  const size_t n_chunks = (nds + chunk - 1) / chunk, nw = (size_t)d_max + 1, n_keys = n_chunks * nw;
  if (n_chunks > 65535 || n_keys > 0x7fffffffULL)
    return fail(BA_ERR_INVALID, "ba_bow_score: %zu database chunks of %d vectors times %zu words is more than one call indexes", n_chunks, chunk, nw);
  if (set_device(h)) return BA_ERR_HIP;
  const size_t n_part = nqs * n_chunks * (size_t)top_k;
  Scratch& sc = h->scratch;
  HIPCHECK(sc.begin(h->stream));
  ScoreArgs a = {};
  HIPCHECK(sc.put(h->stream, nqs + 1, q_off, &a.q_off)); HIPCHECK(sc.put(h->stream, nds + 1, d_off, &a.d_off));
  HIPCHECK(sc.put(h->stream, qn, q_word, &a.q_word)); HIPCHECK(sc.put(h->stream, qn, q_val, &a.q_val));
  HIPCHECK(sc.put(h->stream, dn, d_word, &a.d_word)); HIPCHECK(sc.put(h->stream, dn, d_val, &a.d_val));
  if (db_end) HIPCHECK(sc.put(h->stream, nqs, db_end, &a.db_end));
  HIPCHECK(sc.take(n_part, &a.part)); HIPCHECK(sc.take(dn, &a.inv_j, &a.inv_v)); HIPCHECK(sc.take(kq, &a.top_idx, &a.top_score));
  HIPCHECK(sc.take(n_keys + 1, &a.hist)); HIPCHECK(sc.take(n_keys, &a.cursor));
  if (score) HIPCHECK(sc.take(nqs * nds, &a.dense));
  a.nq = nq; a.nd = nd; a.n_words = (int)nw; a.chunk = chunk; a.n_chunks = (int)n_chunks; a.top_k = top_k; a.d_nnz = (long long)dn; a.n_keys = (long long)n_keys;
  HIPCHECK(hipMemsetAsync(a.hist, 0, (n_keys + 1) * sizeof(int), h->stream));
  const unsigned entry_grid = (unsigned)((dn + BW_THREADS - 1) / BW_THREADS);
  BA_LAUNCH(k_bow_inv_hist, dim3(entry_grid), dim3(BW_THREADS), 0, h->stream, a);
  BA_LAUNCH(k_bow_scan, dim3(1), dim3(BW_SCAN_THREADS), 0, h->stream, a);
  HIPCHECK(hipMemcpyAsync(a.cursor, a.hist, n_keys * sizeof(int), hipMemcpyDeviceToDevice, h->stream));
  BA_LAUNCH(k_bow_inv_scatter, dim3(entry_grid), dim3(BW_THREADS), 0, h->stream, a);
  BA_LAUNCH(k_bow_score_chunk, dim3((unsigned)nq, (unsigned)n_chunks), dim3(BW_THREADS), 0, h->stream, a);
  BA_LAUNCH(k_bow_score_merge, dim3((unsigned)((nqs + BW_THREADS - 1) / BW_THREADS)), dim3(BW_THREADS), 0, h->stream, a);
  if (top_idx) HIPCHECK(hipMemcpyAsync(top_idx, a.top_idx, kq * 4, hipMemcpyDeviceToHost, h->stream));
  if (top_score) HIPCHECK(hipMemcpyAsync(top_score, a.top_score, kq * 4, hipMemcpyDeviceToHost, h->stream));
  if (score) HIPCHECK(hipMemcpyAsync(score, a.dense, nqs * nds * 4, hipMemcpyDeviceToHost, h->stream));
  BA_SYNC(h);
  return BA_OK;
}

// ------------------------------------------------------------------------ feature tracks
// ba_build_tracks (csrc/ba_trackbuild.hpp).  Needs no problem.
extern "C" int ba_default_trackbuild_options(ba_trackbuild_options* o) {
  if (!o) return fail(BA_ERR_INVALID, "null options");
  o->min_length = 2; o->conflict = BA_TRACKS_DROP; o->max_rounds = 0; o->reserved = 0;
  return BA_OK;
}
static_assert(TB_DROP == BA_TRACKS_DROP && TB_FIRST == BA_TRACKS_FIRST && TB_IN_TRACK == BA_TRACKBUILD_IN_TRACK &&
              TB_ISOLATED == BA_TRACKBUILD_ISOLATED && TB_CONFLICT == BA_TRACKBUILD_CONFLICT && TB_SHORT == BA_TRACKBUILD_SHORT,
              "device codes of ba_build_tracks (ba_trackbuild.hpp)");
extern "C" int ba_build_tracks(ba_handle* h, int32_t n_images, const int64_t* kp_off, int64_t n_edges, const int32_t* edge_a,
                               const int32_t* edge_b, const uint8_t* edge_keep, const ba_trackbuild_options* opts, int32_t* node_label,
                               int32_t* node_track, uint8_t* node_status, int64_t* track_off, int32_t* track_node, int64_t* counts) {
  if (!h) return fail(BA_ERR_INVALID, "null handle");
  if (!kp_off) return fail(BA_ERR_INVALID, "ba_build_tracks: kp_off is NULL");
  if (!opts) return fail(BA_ERR_INVALID, "ba_build_tracks: opts is NULL");
  if (!node_label) return fail(BA_ERR_INVALID, "ba_build_tracks: node_label is NULL");
  if (!node_track) return fail(BA_ERR_INVALID, "ba_build_tracks: node_track is NULL");
  if (!node_status) return fail(BA_ERR_INVALID, "ba_build_tracks: node_status is NULL");
  if (!track_off) return fail(BA_ERR_INVALID, "ba_build_tracks: track_off is NULL");
  if (!track_node) return fail(BA_ERR_INVALID, "ba_build_tracks: track_node is NULL");
  if (!counts) return fail(BA_ERR_INVALID, "ba_build_tracks: counts is NULL");
  if (n_images < 0) return fail(BA_ERR_INVALID, "ba_build_tracks: n_images %d is negative", n_images);
  if (n_edges < 0 || n_edges > (1LL << 36)) return fail(BA_ERR_INVALID, "ba_build_tracks: n_edges %lld is outside 0 .. 2^36", (long long)n_edges);
  if (n_edges > 0 && !edge_a) return fail(BA_ERR_INVALID, "ba_build_tracks: edge_a is NULL");
  if (n_edges > 0 && !edge_b) return fail(BA_ERR_INVALID, "ba_build_tracks: edge_b is NULL");
  if (kp_off[0] != 0) return fail(BA_ERR_INVALID, "ba_build_tracks: kp_off must start at 0, not %lld", (long long)kp_off[0]);
  for (int32_t i = 0; i < n_images; ++i)
    if (kp_off[i + 1] < kp_off[i]) return fail(BA_ERR_INVALID, "ba_build_tracks: kp_off decreases at image %d", i);
  if (kp_off[n_images] > 0x7fffffffLL) return fail(BA_ERR_INVALID, "ba_build_tracks: kp_off: N = %lld nodes is above 2^31 - 1", (long long)kp_off[n_images]);
  if (opts->min_length < 2) return fail(BA_ERR_INVALID, "ba_build_tracks: min_length %d is below 2", opts->min_length);
  if (opts->conflict != BA_TRACKS_DROP && opts->conflict != BA_TRACKS_FIRST)
    return fail(BA_ERR_INVALID, "ba_build_tracks: conflict %d is neither BA_TRACKS_DROP (0) nor BA_TRACKS_FIRST (1)", opts->conflict);
  if (opts->max_rounds < 0) return fail(BA_ERR_INVALID, "ba_build_tracks: max_rounds %d is negative", opts->max_rounds);
  const size_t N = (size_t)kp_off[n_images], E = (size_t)n_edges, H = N / 2 + 2, ni = (size_t)n_images;
  const int n = (int)N;
  memset(counts, 0, 8 * sizeof(int64_t));
  track_off[0] = 0;
  if (N == 0 && E == 0) return BA_OK;
  if (set_device(h)) return BA_ERR_HIP;
  // two rounds do it (ba_trackbuild.hpp: a lane leaves the first hook round only with its edge's ends in one tree); the cap is a
  // net far above that, ceil(log2 max(N, 2)) + 2
  int cap = 2;
  while (cap - 2 < 31 && ((size_t)1 << (cap - 2)) < std::max<size_t>(N, 2)) ++cap;
  if (opts->max_rounds > 0) cap = opts->max_rounds;
  Scratch& sc = h->scratch;
  HIPCHECK(sc.begin(h->stream));
  const int *d_ea, *d_eb;
  const unsigned char* d_keep = nullptr;
  const long long* d_kpoff;
  int *d_parent, *d_img, *d_cnt, *d_seglen, *d_segoff, *d_iscomp, *d_compid, *d_seg, *d_sorted, *d_ntrack, *d_tnode;
  int *d_croot, *d_coff, *d_nconf, *d_istrack, *d_trkid, *d_big, *d_giant, *d_toff, *d_bsum, *d_flag, *d_lists;
  unsigned char *d_use, *d_status, *d_conf;
  unsigned long long* d_stat;                            // [0] smallest bad edge, [3 .. 5] k_tb_comp_verdict, [6] same-image edges
  HIPCHECK(sc.put(h->stream, ni + 1, kp_off, &d_kpoff)); HIPCHECK(sc.put(h->stream, E, edge_a, &d_ea)); HIPCHECK(sc.put(h->stream, E, edge_b, &d_eb));
  if (edge_keep) HIPCHECK(sc.put(h->stream, E, edge_keep, &d_keep));
  HIPCHECK(sc.take(N, &d_parent, &d_img, &d_seglen, &d_iscomp, &d_seg, &d_sorted, &d_ntrack, &d_tnode));
  HIPCHECK(sc.take(2 * N, &d_cnt)); HIPCHECK(sc.take(N + 1, &d_segoff, &d_compid));      // cnt | fill: cleared together
  HIPCHECK(sc.take(H, &d_croot, &d_coff, &d_nconf, &d_istrack, &d_trkid, &d_big, &d_giant, &d_toff));
  HIPCHECK(sc.take(1026, &d_bsum)); HIPCHECK(sc.take(1, &d_flag)); HIPCHECK(sc.take(2, &d_lists));
  HIPCHECK(sc.take(E, &d_use)); HIPCHECK(sc.take(N, &d_status)); HIPCHECK(sc.take(N + 1, &d_conf)); HIPCHECK(sc.take(8, &d_stat));
  int* const d_fill = d_cnt + N;
  int* const d_out = d_seglen; int* const d_pos = d_segoff;      // (seg_len and seg_off are used up when out and pos are written)
  auto grid = [](size_t items) { return dim3((unsigned)((items + TB_THREADS - 1) / TB_THREADS)); };
  HIPCHECK(hipMemsetAsync(d_stat, 0, 8 * sizeof(unsigned long long), h->stream));
  HIPCHECK(hipMemsetAsync(d_stat, 0xff, sizeof(unsigned long long), h->stream));
  if (N > 0) BA_LAUNCH(k_tb_init, grid(N), dim3(TB_THREADS), 0, h->stream, n, (const long long*)d_kpoff, n_images, d_parent, d_img, d_ntrack, d_status);
  int rounds = 0;
  if (E > 0) {
    BA_LAUNCH(k_tb_edges, grid(E), dim3(TB_THREADS), 0, h->stream, (const int*)d_ea, (const int*)d_eb, (const unsigned char*)(edge_keep ? d_keep : nullptr),
              (long long)E, n, (const int*)d_img, d_use, d_stat, d_stat + 6);
    unsigned long long bad = 0;
    HIPCHECK(hipMemcpyAsync(&bad, d_stat, sizeof bad, hipMemcpyDeviceToHost, h->stream));
    BA_SYNC(h);
    if (bad != ~0ULL)
      return fail(BA_ERR_INVALID, "ba_build_tracks: edge %llu: edge_a = %d, edge_b = %d is outside 0 .. N - 1 = %d", bad, edge_a[bad], edge_b[bad], n - 1);
    for (;;) {
      if (rounds == cap)
        return fail(BA_ERR_INTERNAL, "ba_build_tracks: BA_ERR_INTERNAL: max_rounds: the components of %d nodes were not finished after %d hook rounds", n, cap);
      int differed = 0;
      HIPCHECK(hipMemsetAsync(d_flag, 0, sizeof(int), h->stream));
      BA_LAUNCH(k_tb_hook, grid(E), dim3(TB_THREADS), 0, h->stream, (const int*)d_ea, (const int*)d_eb, (const unsigned char*)d_use, (long long)E, d_parent, d_flag);
      ++rounds;
      HIPCHECK(hipMemcpyAsync(&differed, d_flag, sizeof(int), hipMemcpyDeviceToHost, h->stream));
      BA_SYNC(h);
      if (!differed) break;                    // no link was made in this round: the trees are the stars the last compress left
      BA_LAUNCH(k_tb_compress, grid(N), dim3(TB_THREADS), 0, h->stream, n, d_parent);
    }
  }
  int M = 0, C = 0, T = 0, members = 0;
  if (N > 0) {
    const int* label = d_parent;
    HIPCHECK(hipMemsetAsync(d_cnt, 0, 2 * N * sizeof(int), h->stream));        // cnt | fill
    BA_LAUNCH(k_tb_sizes, grid(N), dim3(TB_THREADS), 0, h->stream, n, label, d_cnt);
    BA_LAUNCH(k_tb_roots, grid(N), dim3(TB_THREADS), 0, h->stream, n, label, (const int*)d_cnt, d_seglen, d_iscomp);
    if (int rc = dev_scan(h, d_seglen, N, d_bsum, d_segoff)) return rc;
    if (int rc = dev_scan(h, d_iscomp, N, d_bsum, d_compid)) return rc;
    HIPCHECK(hipMemcpyAsync(&M, d_segoff + N, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipMemcpyAsync(&C, d_compid + N, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    BA_SYNC(h);
  }
  if (C > 0) {
    const int* label = d_parent;
    const size_t Ms = (size_t)M, Cs = (size_t)C;
    const int wave_max = h->debug_track_seg > 0 ? std::max(1, std::min(TB_WAVE_MAX, h->debug_track_seg / 2)) : TB_WAVE_MAX;
    const int lds_max = h->debug_track_seg > 0 ? std::max(wave_max, std::min(TB_LDS_MAX, h->debug_track_seg)) : TB_LDS_MAX;
    BA_LAUNCH(k_tb_comp_list, grid(N), dim3(TB_THREADS), 0, h->stream, n, (const int*)d_iscomp, (const int*)d_compid, (const int*)d_segoff, d_croot, d_coff);
    BA_LAUNCH(k_tb_scatter, grid(N), dim3(TB_THREADS), 0, h->stream, n, label, (const int*)d_cnt, (const int*)d_segoff, lds_max, d_fill, d_seg);
    HIPCHECK(hipMemsetAsync(d_lists, 0, 2 * sizeof(int), h->stream));
    HIPCHECK(hipMemsetAsync(d_nconf, 0, Cs * sizeof(int), h->stream));
    const unsigned sort_grid = (unsigned)std::min<size_t>(Cs, TB_SORT_GRID);
    BA_LAUNCH(k_tb_sort_wave, dim3((unsigned)((Cs + TB_THREADS / 64 - 1) / (TB_THREADS / 64))), dim3(TB_THREADS), 0, h->stream, C, (const int*)d_coff,
              (const int*)d_seg, d_sorted, wave_max, lds_max, d_big, d_giant, d_lists);
    BA_LAUNCH(k_tb_sort_lds, dim3(sort_grid), dim3(TB_THREADS), 0, h->stream, (const int*)d_big, (const int*)d_lists, (const int*)d_coff, (const int*)d_seg, d_sorted);
    int n_giant = 0;
    HIPCHECK(hipMemcpyAsync(&n_giant, d_lists + 1, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    BA_SYNC(h);
    for (int g = 0; g < n_giant; ++g) {        // (d_out and d_pos are free here: seg_len and seg_off have been used up)
      BA_LAUNCH(k_tb_giant_flags, grid(N), dim3(TB_THREADS), 0, h->stream, n, label, (const int*)(d_giant + g), (const int*)d_croot, d_out);
      if (int rc = dev_scan(h, d_out, N, d_bsum, d_pos)) return rc;
      BA_LAUNCH(k_tb_giant_place, grid(N), dim3(TB_THREADS), 0, h->stream, n, (const int*)d_out, (const int*)d_pos, (const int*)(d_giant + g), (const int*)d_coff,
                d_sorted);
    }
    BA_LAUNCH(k_tb_conflict, grid(Ms), dim3(TB_THREADS), 0, h->stream, M, (const int*)d_sorted, label, (const int*)d_compid, (const int*)d_coff, (const int*)d_img,
              d_conf, d_nconf);
    BA_LAUNCH(k_tb_comp_verdict, grid(Cs), dim3(TB_THREADS), 0, h->stream, C, (const int*)d_coff, (const int*)d_nconf, (int)opts->conflict, (int)opts->min_length,
              d_istrack, d_stat);
    if (int rc = dev_scan(h, d_istrack, Cs, d_bsum, d_trkid)) return rc;
    BA_LAUNCH(k_tb_out_flags, grid(Ms), dim3(TB_THREADS), 0, h->stream, M, (const int*)d_sorted, label, (const int*)d_compid, (const int*)d_istrack,
              (const unsigned char*)d_conf, d_out);
    if (int rc = dev_scan(h, d_out, Ms, d_bsum, d_pos)) return rc;
    BA_LAUNCH(k_tb_emit, grid(Ms), dim3(TB_THREADS), 0, h->stream, M, (const int*)d_sorted, label, (const int*)d_compid, (const int*)d_coff, (const int*)d_istrack,
              (const int*)d_trkid, (const int*)d_nconf, (const unsigned char*)d_conf, (const int*)d_pos, (int)opts->conflict, d_tnode, d_toff, d_ntrack, d_status);
    HIPCHECK(hipMemcpyAsync(&T, d_trkid + C, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipMemcpyAsync(&members, d_pos + M, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    BA_SYNC(h);
  }
  unsigned long long stat[8] = {};
  std::vector<int32_t> toff((size_t)T);
  HIPCHECK(hipMemcpyAsync(stat, d_stat, sizeof stat, hipMemcpyDeviceToHost, h->stream));
  if (N > 0) {
    HIPCHECK(hipMemcpyAsync(node_label, d_parent, N * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipMemcpyAsync(node_track, d_ntrack, N * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipMemcpyAsync(node_status, d_status, N, hipMemcpyDeviceToHost, h->stream));
  }
  if (T > 0) HIPCHECK(hipMemcpyAsync(toff.data(), d_toff, (size_t)T * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  if (members > 0) HIPCHECK(hipMemcpyAsync(track_node, d_tnode, (size_t)members * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  BA_SYNC(h);
  for (int t = 0; t < T; ++t) track_off[t] = toff[t];
  track_off[T] = members;
  counts[0] = T; counts[1] = members; counts[2] = C; counts[3] = (int64_t)stat[3]; counts[4] = (int64_t)stat[4]; counts[5] = (int64_t)stat[5];
  counts[6] = (int64_t)stat[6]; counts[7] = rounds;
  return BA_OK;
}

// ------------------------------------------------------------------------ bench hook
extern "C" int ba_time_kernel(ba_handle* h, int slot, int reps, double* mean_us) {
  if (!h || !mean_us || reps < 1) return fail(BA_ERR_INVALID, "bad argument");
  if (!h->have_params) return fail(BA_ERR_STATE, "no parameters set");
  if (slot == BA_K_TRACKS && !h->trk_valid) return fail(BA_ERR_STATE, "BA_K_TRACKS repeats the last ba_triangulate_tracks: call it first");
  if (slot == BA_K_RESECT && !h->rs.valid) return fail(BA_ERR_STATE, "BA_K_RESECT repeats the last ba_resect: call it first");
  if (slot == BA_K_RESECT_RANSAC && !h->rn.valid) return fail(BA_ERR_STATE, "BA_K_RESECT_RANSAC repeats the last ba_resect_ransac: call it first");
  if (set_device(h)) return BA_ERR_HIP;
  const bool saved = h->profile;
  h->profile = false;
  const ba_loss loss = h->lin_loss;
  const bool robust = loss != BA_LOSS_LINEAR;
  launch_lin_cam(h, h->cur, h->lb, loss, h->lin_fscale);
  launch_lin_finalize(h);
  launch_lin_pt(h, h->cur, h->pb, loss, h->lin_fscale, 1e-4);
  h->linearized = true;
  if (int rc = damped_system(h, 1e-4, true)) return rc;
  BA_LAUNCH(k_pcg_reset, dim3(1), dim3(64), 0, h->stream, h->st.p, h->partV.p, nbv(h));
  hipEvent_t e0, e1;
  HIPCHECK(hipEventCreate(&e0));
  HIPCHECK(hipEventCreate(&e1));
  auto once = [&]() {
    switch (slot) {
      case BA_K_RESIDUAL: launch_residual(h, h->cur, loss, h->lin_fscale, nullptr); break;
      case BA_K_LINEARIZE_CAM: launch_lin_cam(h, h->cur, h->lb, loss, h->lin_fscale); break;
      case BA_K_LINEARIZE_PT: launch_lin_pt(h, h->cur, h->pb, loss, h->lin_fscale, 1e-4); break;
      case BA_K_SCHUR_PT: launch_pt_schur(h, robust, 0, 0, -1.0, 1 << 30); break;
      case BA_K_SCHUR_CAM: launch_cam_schur(h, robust, false, false, 0); break;
      case BA_K_PRECOND: launch_cam_schur(h, robust, true, false, 0); break;
      case BA_K_POINT_INVERT: launch_point_invert(h, 1e-4); break;
      case BA_K_TRACKS: launch_tracks(h); break;
      case BA_K_RESECT: launch_resect(h); break;
      case BA_K_RESECT_RANSAC: (void)launch_ransac(h); break;
      default: break;
    }
  };
  once();
  HIPCHECK(hipEventRecord(e0, h->stream));
  for (int i = 0; i < reps; ++i) once();
  HIPCHECK(hipEventRecord(e1, h->stream));
  HIPCHECK(hipEventSynchronize(e1));
  float ms = 0;
  HIPCHECK(hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  h->profile = saved;
  *mean_us = 1e3 * ms / reps;
  return BA_OK;
}

// --------------------------------------------------------------- diagnostic build only
#ifdef BA_STAMPS
extern "C" int ba_debug_mode(ba_handle* h, int mode) {
  if (!h) return fail(BA_ERR_INVALID, "null handle");
  if (set_device(h)) return BA_ERR_HIP;
  HIPCHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_dbg_mode), &mode, sizeof(int)));
  return BA_OK;
}
// copy the stamps of the last launch of kind 0 (PCG point pass), 1 (PCG camera pass), 2 (k_pcg_step), 3 (k_pcg_setup)
extern "C" int ba_debug_stamps(ba_handle* h, int kind, unsigned long long* out, int n_blocks) {
  if (!h || !out || kind < 0 || kind > 3 || n_blocks < 1 || n_blocks > STAMP_BLOCKS) return fail(BA_ERR_INVALID, "bad argument");
  if (set_device(h)) return BA_ERR_HIP;
  BA_SYNC(h);
  HIPCHECK(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps), (size_t)n_blocks * 8 * sizeof(unsigned long long),
                               (size_t)kind * STAMP_BLOCKS * 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return BA_OK;
}
#endif
