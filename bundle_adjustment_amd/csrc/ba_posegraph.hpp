// Sim(3) pose-graph optimisation (ba_pose_graph, ba_pose_graph_system): the step between a loop closure and the global
// adjustment that spreads accumulated drift -- rotation, translation and, for a monocular trajectory, scale -- over the
// keyframes (ORB-SLAM's OptimizeEssentialGraph, g2o's EdgeSim3).  Stand-alone fp64 kernels: they read and write the
// handle's pose-graph buffers and none of the LM / Schur / PCG kernels of the adjustment.
//
// Conventions (include/ba_hip.h has them in full): node k = rvec | t | s, x_k = s_k R_k X + t_k; edge (i, j) measures
// S_j o S_i^-1 as rvec_ij | t_ij | s_ij.  With s_r = s_j / s_i, R_r = R_j R_i^T, q = s_r R_r t_i, t_r = t_j - q:
//   e = [ log(R_ij^T R_r) ; t_r - t_ij ; ln(s_r / s_ij) ]
// and, for the local parameters d = (d_omega, d_t, d_sigma) with R <- exp(d_omega) R, t <- t + d_t, s <- s exp(d_sigma),
// the analytic Jacobians at d = 0 (N = Jl^-1(e_rot) R_ij^T, Jl^-1 the inverse left Jacobian of SO(3)):
//   B = de/dd_j = [ N 0 0 ; [q]x I -q ; 0 0 1 ]      A = de/dd_i = [ -N R_r 0 0 ; -[q]x R_r  -s_r R_r  q ; 0 0 -1 ]
//
// Layout: a TEAM of 8 lanes per edge or node, lane r holding row r of a 7 x 7 block (lane 7 idles): one lane with A, B,
// info and e would hold 150 doubles and spill.
//   edge pass    k_pg_edge<true>: every lane of the team forms the 3 x 3 geometry, lane r row r of A and B (into an LDS tile),
//                row r of info, chi2 = e^T info e through the tile in index order, w = rho'(chi2 / f_scale^2), and the
//                record A^T, B^T, w info A, w info B (49 each), w info e (7).  k_pg_edge<false>: e, chi2, w alone (the
//                cost at a trial point).  Per-workgroup partials of sum chi2 and sum rho.
//   node pass    k_pg_node_lin: a team per node walks its incidence list (CSR, by edge number, low bit = side) in list order:
//                H_kk = sum J^T (w info J), g_k = sum J^T (w info e), made bit-symmetric through LDS (lower := upper), held
//                rows / columns cut, D = max(diag, 1e-12).  A HUB (more than PG_HUB_MIN incident edges) gets a workgroup of
//                its own: its list is cut into chunks whose length depends on the degree alone, the teams take chunks
//                round-robin, the chunk partials land in LDS and team 0 adds them in chunk order -- the same bits for
//                any number of teams.  k_pg_damp: Cholesky of H_kk + lambda D per node (every lane of the team factorises,
//                lane c solves for column c of the inverse), then the first PCG vectors.
//   PCG          three launches per iteration, every verdict on the device:
//                k_pg_pcg_edge  folds the r.z partials, takes the verdict (every workgroup the same bits; workgroup 0 writes the
//                               next state record), forms p = z + beta p at both ends on the fly and u_e = w info (A p_i + B p_j);
//                k_pg_pcg_node  stores p, gathers q_k = sum J^T u_e + lambda D p in list order (hubs as above), p.q partials;
//                k_pg_pcg_step  folds p.q, x += alpha p, r -= alpha q, z = M^-1 r, r.z partials.
//                Two state records alternate so that no workgroup USES a word another one of the same launch writes: a
//                launch reads one record and workgroup 0 writes the other.  One exception, harmless: k_pg_pcg_step's
//                workgroup 0 sets `curv` in the record the other workgroups of that launch copy; none of them looks at
//                that field of its copy, the next launch's verdict does.
//   step         k_pg_step: trial poses, the five LM sums; k_pg_edge<false> at the trial poses; k_pg_fold: every partial row
//                in index order into the record the host reads.
// Sums: fixed order everywhere -- list order inside a team, wave_total_dpp inside a wave, waves through LDS in wave order,
// partial rows in index order; no floating-point atomics.  The grids depend on n, m and the degrees alone.
#pragma once
#include "ba_kernels.hpp"
#include "ba_linalg.hpp"

namespace ba {

constexpr int PG_THREADS = 256;
constexpr int PG_TEAMS = PG_THREADS / 8;   // teams of 8 lanes per workgroup
constexpr int PG_WAVES = PG_THREADS / 64;
constexpr int PG_MAX_BLOCKS = 256;         // most workgroups of an edge pass / of the nodes that are no hubs
constexpr int PG_HUB_MIN = 64;             // a node with more incident edges is a hub
constexpr int PG_HUB_CHUNKS = 64;          // most chunks of a hub's list (their partials live in LDS)
constexpr int PG_CHUNK_MIN = 16;           // shortest chunk
constexpr int PG_TILE = 108;               // doubles of an edge team's LDS tile: A (49), B (49), chi2 terms (8), pad

struct PgPcg {                             // PCG state of one iteration
  double rz, rz0, beta;
  int done, iters, curv, pad;
};
struct PgRec {                             // what the host reads back
  double sse, rho, gmax;                   // sum chi2, sum rho(z), max |g| over the free parameters
  double gTd, dDd, dr, step2, x2;          // g.d, d.D d, d.r_pcg, |d|^2, |x|^2 over the free parameters
  PgPcg pcg;
  int bad, pad;                            // a damped diagonal block was not positive definite
};

struct PgGraph {                           // the device's view of the call
  int n, m;
  const int *ei, *ej, *inc_off, *inc, *mask, *hub_node, *hub_len;
  int n_hubs, nb_nodes, hub_teams;         // nb_nodes: workgroups of the nodes that are no hubs
  const double *meas, *info;
  double *At, *Bt, *WA, *WB, *We, *e, *chi2, *wgt;
  double *Hd, *g, *D, *Minv;
  double *x, *r, *z, *p, *q, *u;
  double *part_cost, *part_g, *part_rz, *part_pq, *part_step;
  PgPcg* st;
  PgRec* rec;
  int* bad;
};

__device__ inline void pg_rodrigues(const double* __restrict__ v, double* __restrict__ R) {
  const double rx = v[0], ry = v[1], rz = v[2];
  const double th = sqrt(rx * rx + ry * ry + rz * rz);
  if (th < DBL_EPS) {
    R[0] = 1; R[1] = 0; R[2] = 0; R[3] = 0; R[4] = 1; R[5] = 0; R[6] = 0; R[7] = 0; R[8] = 1;
    return;
  }
  const double c = cos(th), s = sin(th), c1 = 1.0 - c;
  const double kx = rx / th, ky = ry / th, kz = rz / th;
  R[0] = c + c1 * kx * kx;      R[1] = c1 * kx * ky - s * kz; R[2] = c1 * kx * kz + s * ky;
  R[3] = c1 * kx * ky + s * kz; R[4] = c + c1 * ky * ky;      R[5] = c1 * ky * kz - s * kx;
  R[6] = c1 * kx * kz - s * ky; R[7] = c1 * ky * kz + s * kx; R[8] = c + c1 * kz * kz;
}

// rho(z) and rho'(z) of the five losses (include/ba_hip.h, enum ba_loss)
__device__ inline double pg_rho(const int loss, const double z) {
  if (loss == LOSS_LINEAR) return z;
  if (loss == LOSS_HUBER) return z <= 1.0 ? z : 2.0 * sqrt(z) - 1.0;
  return smooth_rho(loss, z);
}

// entry k (0 .. 2, a run-time value) of a register-resident triple, without indexing the registers
__device__ __forceinline__ double pg_sel(const int k, const double a, const double b, const double c) { return k == 0 ? a : (k == 1 ? b : c); }

// v[0 .. NS) summed over the workgroup into out[0 .. NS): DPP inside a wave, the waves through LDS in wave order
template <int NS>
__device__ __forceinline__ void pg_block_sums(const double (&v)[NS], double* __restrict__ lds, double* __restrict__ out) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    const double t = wave_total_dpp(v[j]);
    if (lane == 0) lds[wv * NS + j] = t;
  }
  __syncthreads();
  if (threadIdx.x < NS) {
    double s = lds[threadIdx.x];
#pragma unroll
    for (int k = 1; k < PG_WAVES; ++k) s += lds[k * NS + threadIdx.x];
    out[threadIdx.x] = s;
  }
}

// sum of part[0], part[stride], ... (n rows) in a fixed order, the same bits in every thread of every workgroup: wave 0's lane
// l adds rows l, l + 64, ..., then the wave total
__device__ inline double pg_fold(const double* __restrict__ part, const int n, const int stride, double* __restrict__ sh) {
  if (threadIdx.x < 64) {
    double s = 0.0;
    for (int k = threadIdx.x; k < n; k += 64) s += part[(size_t)k * stride];
    s = wave_total_dpp(s);
    if (threadIdx.x == 0) *sh = s;
  }
  __syncthreads();
  const double v = *sh;
  __syncthreads();
  return v;
}

// ---- edge pass ------------------------------------------------------------------------------------------------------
template <bool JAC>
__global__ void __launch_bounds__(PG_THREADS)
k_pg_edge(const PgGraph G, const double* __restrict__ poses, const int loss, const double inv_f2) {
  __shared__ double tile[PG_TEAMS * (JAC ? PG_TILE : 8)];
  __shared__ double shc[2 * PG_TEAMS];
  constexpr int TS = JAC ? PG_TILE : 8, CO = JAC ? 98 : 0;
  const int team = threadIdx.x >> 3, r = threadIdx.x & 7, rr = r < 7 ? r : 6;
  double* const T = tile + team * TS;
  double tot[2] = {0.0, 0.0};                  // thread 0: this workgroup's sum chi2, sum rho
  for (int base = blockIdx.x * PG_TEAMS; base < G.m; base += gridDim.x * PG_TEAMS) {
    const bool on = base + team < G.m;
    const int e = on ? base + team : G.m - 1;
    const int i = G.ei[e], j = G.ej[e];
    const double* pi = poses + 7 * (size_t)i;
    const double* pj = poses + 7 * (size_t)j;
    const double* ms = G.meas + 7 * (size_t)e;
    double Rr[9], er[3], q[3], ev[7], Rm[9], sr;
    {
      double Ri[9], Rj[9], E[9];
      pg_rodrigues(pi, Ri);
      pg_rodrigues(pj, Rj);
      pg_rodrigues(ms, Rm);
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) Rr[3 * a + b] = Rj[3 * a] * Ri[3 * b] + Rj[3 * a + 1] * Ri[3 * b + 1] + Rj[3 * a + 2] * Ri[3 * b + 2];
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) E[3 * a + b] = Rm[a] * Rr[b] + Rm[3 + a] * Rr[3 + b] + Rm[6 + a] * Rr[6 + b];
      sim_log_map(E, er);
    }
    sr = pj[6] / pi[6];
#pragma unroll
    for (int a = 0; a < 3; ++a) q[a] = sr * (Rr[3 * a] * pi[3] + Rr[3 * a + 1] * pi[4] + Rr[3 * a + 2] * pi[5]);
    ev[0] = er[0]; ev[1] = er[1]; ev[2] = er[2];
    ev[3] = (pj[3] - q[0]) - ms[3]; ev[4] = (pj[4] - q[1]) - ms[4]; ev[5] = (pj[5] - q[2]) - ms[5];
    ev[6] = log(sr / ms[6]);
    // row rr of info, (info e)[rr] and this lane's term of chi2
    double irow[7];
#pragma unroll
    for (int c = 0; c < 7; ++c) irow[c] = G.info ? G.info[49 * (size_t)e + 7 * rr + c] : (c == rr ? 1.0 : 0.0);
    double tr = 0.0;
#pragma unroll
    for (int c = 0; c < 7; ++c) tr += irow[c] * ev[c];
    const double e_r = rr < 3 ? pg_sel(rr, ev[0], ev[1], ev[2]) : (rr < 6 ? pg_sel(rr - 3, ev[3], ev[4], ev[5]) : ev[6]);
    T[CO + r] = r < 7 ? e_r * tr : 0.0;
    if (JAC) {
      // N = Jl^-1(e_rot) R_ij^T with Jl^-1 = I - 1/2 [phi]x + c [phi]x^2, c = (1 - (theta / 2) cot(theta / 2)) / theta^2
      const double t2 = er[0] * er[0] + er[1] * er[1] + er[2] * er[2];
      double cc;
      if (t2 < 1e-4) cc = 1.0 / 12.0 + t2 / 720.0 + t2 * t2 / 30240.0;
      else { const double th = sqrt(t2), hh = 0.5 * th; cc = (1.0 - hh * cos(hh) / sin(hh)) / t2; }
      double Jl[9];
      Jl[0] = 1.0 + cc * (er[0] * er[0] - t2); Jl[1] = 0.5 * er[2] + cc * er[0] * er[1];  Jl[2] = -0.5 * er[1] + cc * er[0] * er[2];
      Jl[3] = -0.5 * er[2] + cc * er[0] * er[1]; Jl[4] = 1.0 + cc * (er[1] * er[1] - t2); Jl[5] = 0.5 * er[0] + cc * er[1] * er[2];
      Jl[6] = 0.5 * er[1] + cc * er[0] * er[2];  Jl[7] = -0.5 * er[0] + cc * er[1] * er[2]; Jl[8] = 1.0 + cc * (er[2] * er[2] - t2);
      // this lane's row of A and B
      double ar[7] = {0, 0, 0, 0, 0, 0, 0}, br[7] = {0, 0, 0, 0, 0, 0, 0};
      if (rr < 3) {
        const double j0 = pg_sel(rr, Jl[0], Jl[3], Jl[6]), j1 = pg_sel(rr, Jl[1], Jl[4], Jl[7]), j2 = pg_sel(rr, Jl[2], Jl[5], Jl[8]);
        double nr[3];                      // row rr of N = Jl^-1 Rm^T
#pragma unroll
        for (int b = 0; b < 3; ++b) nr[b] = j0 * Rm[3 * b] + j1 * Rm[3 * b + 1] + j2 * Rm[3 * b + 2];
#pragma unroll
        for (int b = 0; b < 3; ++b) {
          br[b] = nr[b];
          ar[b] = -(nr[0] * Rr[b] + nr[1] * Rr[3 + b] + nr[2] * Rr[6 + b]);
        }
      } else if (rr < 6) {
        const int k = rr - 3;
        // row k of [q]x
        const double x0 = pg_sel(k, 0.0, q[2], -q[1]), x1 = pg_sel(k, -q[2], 0.0, q[0]), x2 = pg_sel(k, q[1], -q[0], 0.0);
#pragma unroll
        for (int b = 0; b < 3; ++b) {
          ar[b] = -(x0 * Rr[b] + x1 * Rr[3 + b] + x2 * Rr[6 + b]);
          ar[3 + b] = -sr * pg_sel(k, Rr[b], Rr[3 + b], Rr[6 + b]);
          br[3 + b] = (b == k) ? 1.0 : 0.0;
        }
        br[0] = x0; br[1] = x1; br[2] = x2;
        const double qk = pg_sel(k, q[0], q[1], q[2]);
        ar[6] = qk; br[6] = -qk;
      } else {
        ar[6] = -1.0; br[6] = 1.0;
      }
      if (r < 7) {
#pragma unroll
        for (int c = 0; c < 7; ++c) { T[7 * r + c] = ar[c]; T[49 + 7 * r + c] = br[c]; }
      }
    }
    __syncthreads();
    double chi2 = 0.0;
#pragma unroll
    for (int k = 0; k < 7; ++k) chi2 += T[CO + k];
    const double z = chi2 * inv_f2;
    const double w = sim_rho_prime(loss, z);
    if (r == 0) {
      shc[team] = on ? chi2 : 0.0;
      shc[PG_TEAMS + team] = on ? pg_rho(loss, z) : 0.0;
      if (on) { G.chi2[e] = chi2; G.wgt[e] = w; }
    }
    if (on && r < 7 && G.e) G.e[7 * (size_t)e + r] = e_r;
    if (JAC && on && r < 7) {
      double wa[7] = {0, 0, 0, 0, 0, 0, 0}, wb[7] = {0, 0, 0, 0, 0, 0, 0};
#pragma unroll
      for (int b = 0; b < 7; ++b) {
        const double wi = w * irow[b];
#pragma unroll
        for (int c = 0; c < 7; ++c) { wa[c] += wi * T[7 * b + c]; wb[c] += wi * T[49 + 7 * b + c]; }
      }
      const size_t o = 49 * (size_t)e + 7 * r;
#pragma unroll
      for (int c = 0; c < 7; ++c) {
        G.WA[o + c] = wa[c]; G.WB[o + c] = wb[c];
        G.At[o + c] = T[7 * c + r]; G.Bt[o + c] = T[49 + 7 * c + r];
      }
      G.We[8 * (size_t)e + r] = w * tr;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int k = 0; k < PG_TEAMS; ++k) { tot[0] += shc[k]; tot[1] += shc[PG_TEAMS + k]; }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) { G.part_cost[2 * blockIdx.x] = tot[0]; G.part_cost[2 * blockIdx.x + 1] = tot[1]; }
}

// ---- node pass ------------------------------------------------------------------------------------------------------
// entries [t0, t1) of the incidence list: H row rr and g[rr] of sum J^T (w info J), sum J^T (w info e)
__device__ __forceinline__ void pg_walk_lin(const PgGraph& G, const int t0, const int t1, const int rr, double (&H)[7], double& g) {
  for (int t = t0; t < t1; ++t) {
    const int code = G.inc[t], e = code >> 1, side = code & 1;
    const double* Jt = (side ? G.Bt : G.At) + 49 * (size_t)e + 7 * rr;
    const double* WJ = (side ? G.WB : G.WA) + 49 * (size_t)e;
    const double* We = G.We + 8 * (size_t)e;
#pragma unroll
    for (int a = 0; a < 7; ++a) {
      const double jv = Jt[a];
#pragma unroll
      for (int c = 0; c < 7; ++c) H[c] += jv * WJ[7 * a + c];
      g += jv * We[a];
    }
  }
}
// entries [t0, t1): (J^T u)[rr]
__device__ __forceinline__ double pg_walk_pcg(const PgGraph& G, const int t0, const int t1, const int rr) {
  double y = 0.0;
  for (int t = t0; t < t1; ++t) {
    const int code = G.inc[t], e = code >> 1, side = code & 1;
    const double* Jt = (side ? G.Bt : G.At) + 49 * (size_t)e + 7 * rr;
    const double* u = G.u + 8 * (size_t)e;
#pragma unroll
    for (int a = 0; a < 7; ++a) y += Jt[a] * u[a];
  }
  return y;
}
// chunk length of a hub's list: from its degree alone
__host__ __device__ inline int pg_chunk_len(const int deg) {
  const int c = (deg + PG_HUB_CHUNKS - 1) / PG_HUB_CHUNKS;
  return c > PG_CHUNK_MIN ? c : PG_CHUNK_MIN;
}

// the team's block row (H, g) of node k -> symmetric block, held rows and columns, D, max |g|.  Called by every thread of
// the workgroup (it synchronises); `on` = this team holds a node.
__device__ __forceinline__ double pg_finish_lin(const PgGraph& G, const bool on, const int k, const int r, double (&H)[7], double g,
                                                double* __restrict__ T) {
  if (on && r < 7) {
#pragma unroll
    for (int c = 0; c < 7; ++c) T[7 * r + c] = H[c];
  }
  __syncthreads();
  double gm = 0.0;
  if (on && r < 7) {
    const int mk = G.mask[k];
#pragma unroll
    for (int c = 0; c < 7; ++c) {
      if (c < r) H[c] = T[7 * c + r];                  // lower := upper
      if ((mk >> c) & 1) H[c] = 0.0;
    }
    double d;
    if ((mk >> r) & 1) {
#pragma unroll
      for (int c = 0; c < 7; ++c) H[c] = (c == r) ? 1.0 : 0.0;
      g = 0.0; d = 0.0;
    } else {
      const double hrr = T[8 * r];
      d = hrr > DIAG_FLOOR ? hrr : DIAG_FLOOR;
    }
#pragma unroll
    for (int c = 0; c < 7; ++c) G.Hd[49 * (size_t)k + 7 * r + c] = H[c];
    G.g[8 * (size_t)k + r] = g;
    G.D[8 * (size_t)k + r] = d;
    gm = fabs(g);
    if (g != g) gm = g;
  }
  __syncthreads();
  return gm;
}

__global__ void __launch_bounds__(PG_THREADS) k_pg_node_lin(const PgGraph G) {
  __shared__ double tile[PG_TEAMS * 56];
  __shared__ double hub[PG_HUB_CHUNKS * 64];
  __shared__ double shm[PG_WAVES];
  const int team = threadIdx.x >> 3, r = threadIdx.x & 7, rr = r < 7 ? r : 6;
  double gm = 0.0;
  if ((int)blockIdx.x < G.nb_nodes) {
    for (int base = blockIdx.x * PG_TEAMS; base < G.n; base += G.nb_nodes * PG_TEAMS) {
      const int k = base + team;
      bool on = k < G.n;
      double H[7] = {0, 0, 0, 0, 0, 0, 0}, g = 0.0;
      if (on) {
        const int t0 = G.inc_off[k], t1 = G.inc_off[k + 1];
        if (t1 - t0 > PG_HUB_MIN) on = false;          // a hub: its own workgroup
        else pg_walk_lin(G, t0, t1, rr, H, g);
      }
      gm = nanmax(gm, pg_finish_lin(G, on, k, r, H, g, tile + team * 56));
    }
  } else {
    const int hb = blockIdx.x - G.nb_nodes, k = G.hub_node[hb], len = G.hub_len[hb];
    const int t0 = G.inc_off[k], t1 = G.inc_off[k + 1];
    const int n_chunks = (t1 - t0 + len - 1) / len;
    if (team < G.hub_teams)
      for (int ch = team; ch < n_chunks; ch += G.hub_teams) {
        double H[7] = {0, 0, 0, 0, 0, 0, 0}, g = 0.0;
        const int a = t0 + ch * len, b = a + len < t1 ? a + len : t1;
        pg_walk_lin(G, a, b, rr, H, g);
#pragma unroll
        for (int c = 0; c < 7; ++c) hub[64 * ch + 8 * r + c] = H[c];
        hub[64 * ch + 8 * r + 7] = g;
      }
    __syncthreads();
    double H[7] = {0, 0, 0, 0, 0, 0, 0}, g = 0.0;
    if (team == 0)
      for (int ch = 0; ch < n_chunks; ++ch) {
#pragma unroll
        for (int c = 0; c < 7; ++c) H[c] += hub[64 * ch + 8 * r + c];
        g += hub[64 * ch + 8 * r + 7];
      }
    gm = pg_finish_lin(G, team == 0, k, r, H, g, tile);
  }
  gm = wave_max_dpp(gm != gm ? 1.7976931348623157e308 : gm);
  if ((threadIdx.x & 63) == 0) shm[threadIdx.x >> 6] = gm;
  __syncthreads();
  if (threadIdx.x == 0) {
    double m = shm[0];
    for (int k = 1; k < PG_WAVES; ++k) m = fmax(m, shm[k]);
    G.part_g[blockIdx.x] = m;
  }
}

// Cholesky of H_kk + lambda D (lower triangle in registers; every lane of the team factorises), column c of the inverse by
// lane c, then the first PCG vectors: x = 0, r = -g, z = M^-1 r, p = 0 (the first direction is z + 0 p), r.z partials.
__global__ void __launch_bounds__(PG_THREADS) k_pg_damp(const PgGraph G, const double lambda) {
  __shared__ double lds[PG_WAVES];
  const int team = threadIdx.x >> 3, c = threadIdx.x & 7, cc = c < 7 ? c : 6;
  double acc[1] = {0.0};
  for (int base = blockIdx.x * PG_TEAMS; base < G.n; base += gridDim.x * PG_TEAMS) {
    const int k = base + team;
    if (k >= G.n) continue;
    const double* Hk = G.Hd + 49 * (size_t)k;
    const double* Dk = G.D + 8 * (size_t)k;
    double L[7][7];
#pragma unroll
    for (int i = 0; i < 7; ++i)
#pragma unroll
      for (int j = 0; j <= i; ++j) L[i][j] = Hk[7 * i + j] + (i == j ? lambda * Dk[i] : 0.0);
    bool bad = false;
#pragma unroll
    for (int j = 0; j < 7; ++j) {
      double d = L[j][j];
#pragma unroll
      for (int s = 0; s < j; ++s) d -= L[j][s] * L[j][s];
      if (!(d > 0.0)) { bad = true; d = 1.0; }
      const double ld = sqrt(d), il = 1.0 / ld;
      L[j][j] = il;                                     // the reciprocal of the pivot is what the solves use
#pragma unroll
      for (int i = j + 1; i < 7; ++i) {
        double v = L[i][j];
#pragma unroll
        for (int s = 0; s < j; ++s) v -= L[i][s] * L[j][s];
        L[i][j] = v * il;
      }
    }
    if (bad) *G.bad = 1;
    double y[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) {
      double v = (i == cc) ? 1.0 : 0.0;
#pragma unroll
      for (int s = 0; s < i; ++s) v -= L[i][s] * y[s];
      y[i] = v * L[i][i];
    }
#pragma unroll
    for (int i = 6; i >= 0; --i) {
      double v = y[i];
#pragma unroll
      for (int s = i + 1; s < 7; ++s) v -= L[s][i] * y[s];
      y[i] = v * L[i][i];
    }
    if (c < 7) {
      const double* gk = G.g + 8 * (size_t)k;
      double zc = 0.0;
#pragma unroll
      for (int i = 0; i < 7; ++i) { G.Minv[49 * (size_t)k + 7 * c + i] = y[i]; zc -= y[i] * gk[i]; }
      const double rc = -gk[c];
      const size_t o = 8 * (size_t)k + c;
      G.x[o] = 0.0; G.r[o] = rc; G.z[o] = zc; G.p[o] = 0.0;
      acc[0] += rc * zc;
    }
  }
  pg_block_sums<1>(acc, lds, G.part_rz + blockIdx.x);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    PgPcg s0 = {};
    G.st[0] = s0; G.st[1] = s0;
  }
}

// ---- PCG ------------------------------------------------------------------------------------------------------------
__device__ inline PgPcg pg_verdict(const PgPcg in, const double rz_new, const int k, const double tol2, const int min_iters) {
  PgPcg o = in;
  o.curv = 0;
  if (in.done) return o;
  if (in.curv) { o.done = 1; return o; }             // the last iteration met p.q <= 0 and changed nothing
  if (k == 0) {
    o.rz = o.rz0 = rz_new; o.beta = 0.0; o.iters = 0;
    if (!(rz_new > 0.0)) o.done = 1;
    return o;
  }
  o.iters = k; o.rz = rz_new;
  if (k >= min_iters && rz_new <= tol2 * in.rz0) { o.done = 1; return o; }
  o.beta = rz_new / in.rz;
  return o;
}

__global__ void __launch_bounds__(PG_THREADS)
k_pg_pcg_edge(const PgGraph G, const int k, const int n_rz, const double tol2, const int min_iters) {
  __shared__ double sh;
  const double rz_new = pg_fold(G.part_rz, n_rz, 1, &sh);
  const PgPcg S = pg_verdict(G.st[k & 1], rz_new, k, tol2, min_iters);
  if (blockIdx.x == 0 && threadIdx.x == 0) G.st[(k + 1) & 1] = S;
  if (S.done) return;
  const int team = threadIdx.x >> 3, r = threadIdx.x & 7;
  if (r == 7) return;
  for (int e = blockIdx.x * PG_TEAMS + team; e < G.m; e += gridDim.x * PG_TEAMS) {
    const size_t oi = 8 * (size_t)G.ei[e], oj = 8 * (size_t)G.ej[e];
    const double* wa = G.WA + 49 * (size_t)e + 7 * r;
    const double* wb = G.WB + 49 * (size_t)e + 7 * r;
    double u = 0.0;
#pragma unroll
    for (int c = 0; c < 7; ++c) u += wa[c] * (G.z[oi + c] + S.beta * G.p[oi + c]);
#pragma unroll
    for (int c = 0; c < 7; ++c) u += wb[c] * (G.z[oj + c] + S.beta * G.p[oj + c]);
    G.u[8 * (size_t)e + r] = u;
  }
}

// p <- z + beta p (stored), q = H p + lambda D p (held rows: q = p = 0), p.q partials; state record (k + 1) & 1
__global__ void __launch_bounds__(PG_THREADS) k_pg_pcg_node(const PgGraph G, const int k, const double lambda) {
  __shared__ double hub[PG_HUB_CHUNKS * 8];
  __shared__ double lds[PG_WAVES];
  const PgPcg S = G.st[(k + 1) & 1];
  if (S.done) return;
  const int team = threadIdx.x >> 3, r = threadIdx.x & 7, rr = r < 7 ? r : 6;
  double acc[1] = {0.0};
  if ((int)blockIdx.x < G.nb_nodes) {
    for (int node = blockIdx.x * PG_TEAMS + team; node < G.n; node += G.nb_nodes * PG_TEAMS) {
      const int t0 = G.inc_off[node], t1 = G.inc_off[node + 1];
      if (t1 - t0 > PG_HUB_MIN || r == 7) continue;
      const size_t o = 8 * (size_t)node + r;
      const double pv = G.z[o] + S.beta * G.p[o];
      const double y = pg_walk_pcg(G, t0, t1, rr);
      const double qv = ((G.mask[node] >> r) & 1) ? pv : y + lambda * G.D[o] * pv;
      G.p[o] = pv; G.q[o] = qv;
      acc[0] += pv * qv;
    }
  } else {
    const int hb = blockIdx.x - G.nb_nodes, node = G.hub_node[hb], len = G.hub_len[hb];
    const int t0 = G.inc_off[node], t1 = G.inc_off[node + 1];
    const int n_chunks = (t1 - t0 + len - 1) / len;
    if (team < G.hub_teams)
      for (int ch = team; ch < n_chunks; ch += G.hub_teams) {
        const int a = t0 + ch * len, b = a + len < t1 ? a + len : t1;
        hub[8 * ch + r] = pg_walk_pcg(G, a, b, rr);
      }
    __syncthreads();
    if (team == 0 && r < 7) {
      double y = 0.0;
      for (int ch = 0; ch < n_chunks; ++ch) y += hub[8 * ch + r];
      const size_t o = 8 * (size_t)node + r;
      const double pv = G.z[o] + S.beta * G.p[o];
      const double qv = ((G.mask[node] >> r) & 1) ? pv : y + lambda * G.D[o] * pv;
      G.p[o] = pv; G.q[o] = qv;
      acc[0] += pv * qv;
    }
  }
  pg_block_sums<1>(acc, lds, G.part_pq + blockIdx.x);
}

// alpha = r.z / p.q; x += alpha p, r -= alpha q, z = M^-1 r, r.z partials.  p.q <= 0: nothing changes, the state says so.
__global__ void __launch_bounds__(PG_THREADS) k_pg_pcg_step(const PgGraph G, const int k, const int n_pq) {
  __shared__ double sh;
  __shared__ double lds[PG_WAVES];
  const PgPcg S = G.st[(k + 1) & 1];
  if (S.done) return;
  const double pq = pg_fold(G.part_pq, n_pq, 1, &sh);
  if (!(pq > 0.0)) {
    if (blockIdx.x == 0 && threadIdx.x == 0) G.st[(k + 1) & 1].curv = 1;
    return;
  }
  const double alpha = S.rz / pq;
  const int team = threadIdx.x >> 3, r = threadIdx.x & 7;
  double acc[1] = {0.0};
  for (int base = blockIdx.x * PG_TEAMS; base < G.n; base += gridDim.x * PG_TEAMS) {
    const int node = base + team;
    const bool on = node < G.n && r < 7;
    const size_t o = 8 * (size_t)(node < G.n ? node : 0) + (r < 7 ? r : 0);
    double rn = 0.0;
    if (on) {
      G.x[o] += alpha * G.p[o];
      rn = G.r[o] - alpha * G.q[o];
      G.r[o] = rn;
    }
    double zc = 0.0;
#pragma unroll
    for (int c = 0; c < 7; ++c) {
      const double rc = __shfl(rn, c, 8);
      if (on) zc += G.Minv[49 * (size_t)node + 7 * r + c] * rc;
    }
    if (on) { G.z[o] = zc; acc[0] += rn * zc; }
  }
  pg_block_sums<1>(acc, lds, G.part_rz + blockIdx.x);
}

// ---- step, folds ----------------------------------------------------------------------------------------------------
// trial poses R <- exp(d_omega) R, t <- t + d_t, s <- s exp(d_sigma) (a node whose d_omega is exactly zero keeps its rvec bit for
// bit), and the five sums of the LM scalars
__global__ void __launch_bounds__(PG_THREADS)
k_pg_step(const PgGraph G, const double* __restrict__ poses, double* __restrict__ trial) {
  __shared__ double lds[PG_WAVES * 5];
  double v[5] = {0, 0, 0, 0, 0};
  for (int k = blockIdx.x * PG_THREADS + threadIdx.x; k < G.n; k += gridDim.x * PG_THREADS) {
    const double* d = G.x + 8 * (size_t)k;
    const double* ps = poses + 7 * (size_t)k;
    double* out = trial + 7 * (size_t)k;
    const int mk = G.mask[k];
    double dd[7];
#pragma unroll
    for (int c = 0; c < 7; ++c) {
      dd[c] = d[c];
      v[0] += G.g[8 * (size_t)k + c] * dd[c];
      v[1] += G.D[8 * (size_t)k + c] * dd[c] * dd[c];
      v[2] += dd[c] * G.r[8 * (size_t)k + c];
      v[3] += dd[c] * dd[c];
      if (!((mk >> c) & 1)) v[4] += ps[c] * ps[c];
    }
    if (dd[0] == 0.0 && dd[1] == 0.0 && dd[2] == 0.0) {
      out[0] = ps[0]; out[1] = ps[1]; out[2] = ps[2];
    } else {
      double R[9], dR[9], Rn[9], rv[3];
      pg_rodrigues(ps, R);
      pg_rodrigues(dd, dR);
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) Rn[3 * a + b] = dR[3 * a] * R[b] + dR[3 * a + 1] * R[3 + b] + dR[3 * a + 2] * R[6 + b];
      sim_log_map(Rn, rv);
      out[0] = rv[0]; out[1] = rv[1]; out[2] = rv[2];
    }
#pragma unroll
    for (int c = 3; c < 6; ++c) out[c] = dd[c] == 0.0 ? ps[c] : ps[c] + dd[c];      // (-0.0 + 0.0 is +0.0: a held t keeps its bits)
    out[6] = dd[6] == 0.0 ? ps[6] : ps[6] * exp(dd[6]);
  }
  pg_block_sums<5>(v, lds, G.part_step + 5 * (size_t)blockIdx.x);
}

// every partial row in index order into the record (one wave): the cost rows always; max |g| when n_g > 0; the step's sums when
// n_step > 0; the PCG verdict a k_pg_pcg_edge of iteration k would take when k >= 0 (the state itself is left alone)
__global__ void __launch_bounds__(64)
k_pg_fold(const PgGraph G, const int n_cost, const int n_g, const int n_step, const int k, const int n_rz, const double tol2, const int min_iters) {
  __shared__ double sh;
  PgRec* rec = G.rec;
  const double sse = pg_fold(G.part_cost, n_cost, 2, &sh);
  const double rho = pg_fold(G.part_cost + 1, n_cost, 2, &sh);
  if (threadIdx.x == 0) { rec->sse = sse; rec->rho = rho; rec->bad = *G.bad; }
  if (n_g > 0 && threadIdx.x == 0) {
    double m = 0.0;
    for (int b = 0; b < n_g; ++b) m = fmax(m, G.part_g[b]);
    rec->gmax = m;
  }
  if (n_step > 0) {
    double s[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) s[j] = pg_fold(G.part_step + j, n_step, 5, &sh);
    if (threadIdx.x == 0) { rec->gTd = s[0]; rec->dDd = s[1]; rec->dr = s[2]; rec->step2 = s[3]; rec->x2 = s[4]; }
  }
  if (k >= 0) {
    const double rz_new = pg_fold(G.part_rz, n_rz, 1, &sh);
    const PgPcg S = pg_verdict(G.st[k & 1], rz_new, k, tol2, min_iters);
    if (threadIdx.x == 0) rec->pcg = S;
  }
}

// ---- inspection: the dense (7 n)^2 H + lambda D (ba_pose_graph_system) ------------------------------------------------
// a thread per entry of the upper triangle, written to both places.  Diagonal blocks are the node pass's; an off-diagonal
// entry ((k, r), (l, c)) is sum over k's list of the edges whose other end is l of sum_a J_k[a][r] (w info J_l)[a][c].
__global__ void __launch_bounds__(PG_THREADS) k_pg_dense(const PgGraph G, const double lambda, double* __restrict__ Hout) {
  const size_t N = 7 * (size_t)G.n;
  const size_t idx = blockIdx.x * (size_t)PG_THREADS + threadIdx.x;
  if (idx >= N * N) return;
  const int I = (int)(idx / N), J = (int)(idx % N);
  if (I > J) return;
  const int k = I / 7, r = I % 7, l = J / 7, c = J % 7;
  double v = 0.0;
  if (k == l) {
    v = G.Hd[49 * (size_t)k + 7 * r + c] + (r == c ? lambda * G.D[8 * (size_t)k + r] : 0.0);
  } else if (!((G.mask[k] >> r) & 1) && !((G.mask[l] >> c) & 1)) {
    for (int t = G.inc_off[k]; t < G.inc_off[k + 1]; ++t) {
      const int code = G.inc[t], e = code >> 1, side = code & 1;
      if ((side ? G.ei[e] : G.ej[e]) != l) continue;
      const double* Jt = (side ? G.Bt : G.At) + 49 * (size_t)e + 7 * r;
      const double* WJ = (side ? G.WA : G.WB) + 49 * (size_t)e;
      for (int a = 0; a < 7; ++a) v += Jt[a] * WJ[7 * a + c];
    }
  }
  Hout[(size_t)I * N + J] = v;
  Hout[(size_t)J * N + I] = v;
}

}  // namespace ba
