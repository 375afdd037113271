// RANSAC resection (ba_resect_ransac): the pose of every selected camera from raw matches -- minimal P3P samples scored on all
// of the camera's observations, then ba_resect's refinement on the consensus set (cv2.solvePnPRansac of the reference's
// estimate_pose_pnp; the image registration of COLMAP, OpenMVG and ORB-SLAM).  Stand-alone kernels next to ba_resect.hpp: they
// read the handle's camera-ordered observation list, point table and camera state; k_resect and its passes are unchanged.
//
// Three launches per call:
//   k_ransac_prep<CM>   one workgroup per camera: the camera's usable observations (point known, bearing exists) compacted, in
//                       camera order, into records X | u v | j | bx by at the head of the camera's segment; their count n.
//   k_ransac_score<CM>  grid (cameras, ceil(n_hyp / 256)): lane = hypothesis.  Sample -> P3P (Lambda Twist) -> up to four poses
//                       R | t held in registers (slot = 2 * sign + root, fixed, so no register is indexed dynamically); then
//                       the camera's records stream through LDS in tiles of RN_TILE and every lane reads the same address (a
//                       broadcast) and adds to its own four MSAC costs.  No cross-lane traffic until the arg-min of
//                       (cost, 4 h + slot) (ba_hypothesis.hpp).
//   k_ransac_lo<CM>     one workgroup per camera: the lowest (cost, 4 h + slot) of the score blocks, then lo_rounds times
//                       {consensus bytes at the frozen pose; ba_resect's refinement (rs_refine<CM, true>) on them}, then
//                       ba_resect's measures and status (rs_finish), and obs_inlier through c_orig in the caller's order.
//
// Sample (step 2): hy_sample<3> of (seed, camera, h, n) -- three distinct indices into the camera's usable observations in
// camera order.
//
// P3P (step 3), Lambda Twist (Persson & Nordberg, ECCV 2018): with unit rays y_i and depths L_i the three cosine-law equations
// L_i^2 + L_j^2 + b_ij L_i L_j = a_ij are L^T M_ij L = a_ij; D1 = a23 M12 - a12 M23 and D2 = a23 M13 - a13 M23 are homogeneous,
// det(D1 + g D2) = 0 is a cubic (closed form, four Newton steps); the 3 x 3 eigen-decomposition (cyclic Jacobi) of the singular
// D0 = D1 + g D2 splits it into two planes w.L = 0, each leaving a quadratic in tau = L3 / L2.  Every root is polished by three
// Newton steps on the three equations; R = [Y1 - Y2, Y1 - Y3, x] [X1 - X2, X1 - X3, x]^-1, t = Y1 - R X1, Y_i = L_i y_i.  No
// quartic: the cubic always has a real root and the eigenvalue problem is symmetric.
#pragma once
#include "ba_hypothesis.hpp"
#include "ba_resect.hpp"

namespace ba {

constexpr int RN_THREADS = HY_THREADS;
constexpr int RN_TILE = 256;          // records per LDS tile of the scoring loop
constexpr int RN_REC = 8;             // doubles per usable observation: X0 X1 | X2 u | v j | bx by (j: its place in the camera-ordered list)
constexpr int RN_LDS = 6;             // doubles per record in LDS: X0 X1 | X2 u | v -
constexpr int RN_BEST = 16;           // doubles per (camera, score block): cost | 4 h + slot | R[9] | t[3] | - -

struct RansacArgs {
  ResectArgs r;            // as ba_resect: t.max_px is the threshold (> 0), t.loss / t.iters / t.fscale the refinement's, r.out the results
  int n_hyp, lo_rounds, n_blk;
  unsigned long long seed;
  double* rec;             // RN_REC doubles per camera-ordered observation; a camera's usable ones lead its segment
  int* cnt;                // per camera: usable observations (0 for a camera that is not selected)
  double* best;            // RN_BEST doubles per (camera, score block)
  unsigned char* cons;     // per camera-ordered observation: in the consensus set of the round
  const int* c_orig;       // camera order -> the caller's observation
  unsigned char* inl;      // obs_inlier, the caller's order (zeroed before the launch)
};

// packed symmetric 3 x 3: 00 01 02 11 12 22
__device__ __forceinline__ double rn_dot6(const double (&A)[6], const double (&B)[6]) {
  return A[0] * B[0] + A[3] * B[3] + A[5] * B[5] + 2.0 * (A[1] * B[1] + A[2] * B[2] + A[4] * B[4]);
}
// a real root of c3 g^3 + c2 g^2 + c1 g + c0 (c3 != 0): closed form, four Newton steps
__device__ inline double rn_cubic_root(const double c3, const double c2, const double c1, const double c0) {
  const double p2 = c2 / c3, p1 = c1 / c3, p0 = c0 / c3;
  const double P = p1 - p2 * p2 / 3.0;
  const double Q = p2 * (2.0 * p2 * p2 / 27.0 - p1 / 3.0) + p0;
  const double D = 0.25 * Q * Q + P * P * P / 27.0;
  double t;
  if (D > 0.0) {
    const double A = -copysign(1.0, Q) * cbrt(fabs(Q) * 0.5 + sqrt(D));
    t = A - (A != 0.0 ? P / (3.0 * A) : 0.0);
  } else {
    const double m = sqrt(-P / 3.0);
    double arg = m > 0.0 ? 3.0 * Q / (2.0 * P * m) : 0.0;
    arg = fmax(-1.0, fmin(1.0, arg));
    t = 2.0 * m * cos(acos(arg) / 3.0);
  }
  double g = t - p2 / 3.0;
#pragma unroll 1
  for (int it = 0; it < 4; ++it) {
    const double f = ((g + p2) * g + p1) * g + p0, df = (3.0 * g + 2.0 * p2) * g + p1;
    if (df != 0.0) g -= f / df;
  }
  return g;
}

struct RnTriple {          // what the roots of one hypothesis share
  double y[3][3];          // unit rays
  double X0[3];            // the first point
  double Xi[3][3];         // [d12 d13 d12 x d13]^-1
  double a12, a13, a23, b12, b13, b23;
};

// One root: depths from (w0, w1, tau), three Newton steps, the pose.  false: not a solution in front of the camera.
template <class CM>
__device__ __forceinline__ bool rn_root(const RnTriple& T, const double w0, const double w1, const double tau, const double min_depth,
                                        double (&R)[9], double (&t)[3]) {
  if (!(tau > 0.0)) return false;
  const double den = tau * (T.b23 + tau) + 1.0;
  if (!(den > 0.0)) return false;
  double L1 = sqrt(T.a23 / den), L2 = tau * L1;
  double L0 = w0 * L1 + w1 * L2;
  if (!(L0 > 0.0)) return false;
#pragma unroll 1
  for (int it = 0; it < 3; ++it) {
    const double f0 = L0 * L0 + L1 * L1 + T.b12 * L0 * L1 - T.a12;
    const double f1 = L0 * L0 + L2 * L2 + T.b13 * L0 * L2 - T.a13;
    const double f2 = L1 * L1 + L2 * L2 + T.b23 * L1 * L2 - T.a23;
    const double j00 = 2.0 * L0 + T.b12 * L1, j01 = 2.0 * L1 + T.b12 * L0;
    const double j10 = 2.0 * L0 + T.b13 * L2, j12 = 2.0 * L2 + T.b13 * L0;
    const double j21 = 2.0 * L1 + T.b23 * L2, j22 = 2.0 * L2 + T.b23 * L1;
    const double det = -j00 * j12 * j21 - j01 * j10 * j22;
    if (det == 0.0) break;
    const double id = 1.0 / det;
    L0 -= (-j12 * j21 * f0 - j01 * j22 * f1 + j01 * j12 * f2) * id;
    L1 -= (-j10 * j22 * f0 + j00 * j22 * f1 - j00 * j12 * f2) * id;
    L2 -= (j10 * j21 * f0 - j00 * j21 * f1 - j01 * j10 * f2) * id;
  }
  if (!(L0 > 0.0 && L1 > 0.0 && L2 > 0.0)) return false;
  double e1[3], e2[3], Y0[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    Y0[k] = L0 * T.y[0][k];
    e1[k] = Y0[k] - L1 * T.y[1][k];
    e2[k] = Y0[k] - L2 * T.y[2][k];
  }
  const double e3[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      R[3 * i + j] = e1[i] * T.Xi[0][j] + e2[i] * T.Xi[1][j] + e3[i] * T.Xi[2][j];
      ok = ok && sim_finite(R[3 * i + j]);
    }
    t[i] = Y0[i] - (R[3 * i] * T.X0[0] + R[3 * i + 1] * T.X0[1] + R[3 * i + 2] * T.X0[2]);
    ok = ok && sim_finite(t[i]);
  }
  // every sample point in front: its depth is L_i |y_i.z|
  const double s = CM::ID == 0 ? 1.0 : -1.0;
  return ok && s * L0 * T.y[0][2] > min_depth && s * L1 * T.y[1][2] > min_depth && s * L2 * T.y[2][2] > min_depth;
}

// The two roots of one plane w.L = 0 into the slots (Ra, ta), (Rb, tb); bit 0 / 1 of the result: slot a / b holds a pose
template <class CM>
__device__ __forceinline__ int rn_plane(const RnTriple& T, const double (&w)[3], const double min_depth, double (&Ra)[9], double (&ta)[3],
                                        double (&Rb)[9], double (&tb)[3]) {
  if (w[0] == 0.0) return 0;
  const double w0 = -w[1] / w[0], w1 = -w[2] / w[0];
  const double da = T.a13 - T.a12;
  const double qa = da * w1 * w1 - T.a12 * T.b13 * w1 - T.a12;
  const double qb = 2.0 * da * w0 * w1 + T.a13 * T.b12 * w1 - T.a12 * T.b13 * w0;
  const double qc = da * w0 * w0 + T.a13 * T.b12 * w0 + T.a13;
  const double disc = qb * qb - 4.0 * qa * qc;
  if (!(disc >= 0.0) || qa == 0.0) return 0;
  const double q = -0.5 * (qb + copysign(sqrt(disc), qb));
  int m = 0;
  if (rn_root<CM>(T, w0, w1, q / qa, min_depth, Ra, ta)) m |= 1;
  if (q != 0.0 && rn_root<CM>(T, w0, w1, qc / q, min_depth, Rb, tb)) m |= 2;
  return m;
}

// Lambda Twist on three records: the poses into the four slots; the mask of the slots that hold one
template <class CM>
__device__ inline int rn_p3p(const double* __restrict__ r0, const double* __restrict__ r1, const double* __restrict__ r2, const double min_depth,
                             double (&R)[4][9], double (&t)[4][3]) {
  RnTriple T;
  double X[3][3];
  const double* rec[3] = {r0, r1, r2};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double2 a = *(const double2*)(rec[i]), b = *(const double2*)(rec[i] + 2), d = *(const double2*)(rec[i] + 6);
    X[i][0] = a.x; X[i][1] = a.y; X[i][2] = b.x;
    const double s = (CM::ID == 0 ? 1.0 : -1.0) / sqrt(d.x * d.x + d.y * d.y + 1.0);
    T.y[i][0] = s * d.x; T.y[i][1] = s * d.y; T.y[i][2] = s;
  }
  double d12[3], d13[3], d23[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) { d12[k] = X[0][k] - X[1][k]; d13[k] = X[0][k] - X[2][k]; d23[k] = X[1][k] - X[2][k]; T.X0[k] = X[0][k]; }
  T.a12 = d12[0] * d12[0] + d12[1] * d12[1] + d12[2] * d12[2];
  T.a13 = d13[0] * d13[0] + d13[1] * d13[1] + d13[2] * d13[2];
  T.a23 = d23[0] * d23[0] + d23[1] * d23[1] + d23[2] * d23[2];
  const double nx[3] = {d12[1] * d13[2] - d12[2] * d13[1], d12[2] * d13[0] - d12[0] * d13[2], d12[0] * d13[1] - d12[1] * d13[0]};
  const double n2 = nx[0] * nx[0] + nx[1] * nx[1] + nx[2] * nx[2];
  const double ext = fmax(T.a12, fmax(T.a13, T.a23));
  if (!(sqrt(n2) > HY_AREA_TOL * ext) || !sim_finite(ext)) return 0;
  // [d12 d13 n]^-1: rows (d13 x n, n x d12, n) / |n|^2
  {
    const double in2 = 1.0 / n2;
    T.Xi[0][0] = (d13[1] * nx[2] - d13[2] * nx[1]) * in2; T.Xi[0][1] = (d13[2] * nx[0] - d13[0] * nx[2]) * in2; T.Xi[0][2] = (d13[0] * nx[1] - d13[1] * nx[0]) * in2;
    T.Xi[1][0] = (nx[1] * d12[2] - nx[2] * d12[1]) * in2; T.Xi[1][1] = (nx[2] * d12[0] - nx[0] * d12[2]) * in2; T.Xi[1][2] = (nx[0] * d12[1] - nx[1] * d12[0]) * in2;
    T.Xi[2][0] = nx[0] * in2; T.Xi[2][1] = nx[1] * in2; T.Xi[2][2] = nx[2] * in2;
  }
  T.b12 = -2.0 * (T.y[0][0] * T.y[1][0] + T.y[0][1] * T.y[1][1] + T.y[0][2] * T.y[1][2]);
  T.b13 = -2.0 * (T.y[0][0] * T.y[2][0] + T.y[0][1] * T.y[2][1] + T.y[0][2] * T.y[2][2]);
  T.b23 = -2.0 * (T.y[1][0] * T.y[2][0] + T.y[1][1] * T.y[2][1] + T.y[1][2] * T.y[2][2]);
  const double D1[6] = {T.a23, 0.5 * T.a23 * T.b12, 0.0, T.a23 - T.a12, -0.5 * T.a12 * T.b23, -T.a12};
  const double D2[6] = {T.a23, 0.0, 0.5 * T.a23 * T.b13, -T.a13, -0.5 * T.a13 * T.b23, T.a23 - T.a13};
  double C1[6], C2[6];
  sym3_cof(D1, C1); sym3_cof(D2, C2);
  const double c0 = D1[0] * C1[0] + D1[1] * C1[1] + D1[2] * C1[2], c3 = D2[0] * C2[0] + D2[1] * C2[1] + D2[2] * C2[2];
  const double c1 = rn_dot6(C1, D2), c2 = rn_dot6(D1, C2);
  if (!(fabs(c3) > 0.0)) return 0;
  const double g = rn_cubic_root(c3, c2, c1, c0);
  if (!sim_finite(g)) return 0;
  double A[3][3], V[3][3];
  A[0][0] = D1[0] + g * D2[0]; A[0][1] = A[1][0] = D1[1] + g * D2[1]; A[0][2] = A[2][0] = D1[2] + g * D2[2];
  A[1][1] = D1[3] + g * D2[3]; A[1][2] = A[2][1] = D1[4] + g * D2[4]; A[2][2] = D1[5] + g * D2[5];
  jacobi_eig<3, 12>(A, V);
  // the eigenvalue of the smallest magnitude is the zero one; the other two must differ in sign (selection by value, not by index)
  const double l0 = A[0][0], l1 = A[1][1], l2 = A[2][2];
  const double m0 = fabs(l0), m1 = fabs(l1), m2 = fabs(l2);
  double sa, sb, ea[3], eb[3];
  if (m0 <= m1 && m0 <= m2) {
    sa = l1; sb = l2;
#pragma unroll
    for (int k = 0; k < 3; ++k) { ea[k] = V[k][1]; eb[k] = V[k][2]; }
  } else if (m1 <= m2) {
    sa = l0; sb = l2;
#pragma unroll
    for (int k = 0; k < 3; ++k) { ea[k] = V[k][0]; eb[k] = V[k][2]; }
  } else {
    sa = l0; sb = l1;
#pragma unroll
    for (int k = 0; k < 3; ++k) { ea[k] = V[k][0]; eb[k] = V[k][1]; }
  }
  if (sa < 0.0) {
    const double ts = sa; sa = sb; sb = ts;
#pragma unroll
    for (int k = 0; k < 3; ++k) { const double tv = ea[k]; ea[k] = eb[k]; eb[k] = tv; }
  }
  if (!(sa > 0.0 && sb < 0.0)) return 0;
  const double s = sqrt(-sb / sa);
  const double wp[3] = {ea[0] - s * eb[0], ea[1] - s * eb[1], ea[2] - s * eb[2]};
  const double wm[3] = {ea[0] + s * eb[0], ea[1] + s * eb[1], ea[2] + s * eb[2]};
  int mask = rn_plane<CM>(T, wp, min_depth, R[0], t[0], R[1], t[1]);
  mask |= rn_plane<CM>(T, wm, min_depth, R[2], t[2], R[3], t[3]) << 2;
  return mask;
}

// |r|^2 of a record through the model's own projection at (R | t); false: behind the camera
template <class CM>
__device__ __forceinline__ bool rn_err2(const double (&R)[9], const double (&t)[3], const double (&cam)[CM::CAM], const TrackArgs& a,
                                        const double X0, const double X1, const double X2, const double u, const double v, double& e2) {
  const double Px = R[0] * X0 + R[1] * X1 + R[2] * X2 + t[0];
  const double Py = R[3] * X0 + R[4] * X1 + R[5] * X2 + t[1];
  const double Pz = R[6] * X0 + R[7] * X1 + R[8] * X2 + t[2];
  const double iz = 1.0 / Pz;
  double ru, rv;
  if constexpr (CM::ID == 0) {
    ru = u - (Px * iz * a.fx + a.cx);
    rv = v - (Py * iz * a.fy + a.cy);
  } else {
    const double p0 = -Px * iz, p1 = -Py * iz, n2 = p0 * p0 + p1 * p1;
    const double fr = cam[12] * (1.0 + n2 * (cam[13] + cam[14] * n2));
    ru = u - fr * p0;
    rv = v - fr * p1;
  }
  e2 = ru * ru + rv * rv;
  return (CM::ID == 0 ? Pz : -Pz) > a.min_depth;
}

// ------------------------------------------------------------------------------------------------ usable observations
template <class CM>
__global__ void __launch_bounds__(RN_THREADS) k_ransac_prep(const RansacArgs a) {
  __shared__ int wcnt[RS_WAVES];
  const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (a.r.sel && !a.r.sel[c]) {
    if (tid == 0) a.cnt[c] = 0;
    return;
  }
  const int beg = a.r.offk[c * (NPART + 1)], end = a.r.offk[c * (NPART + 1) + NPART];
  double cam[CM::CAM];
  CM::load_cam_vec(a.r.t.cs, a.r.t.intr, c, cam);
  int base = 0;
  for (int j0 = beg; j0 < end; j0 += RN_THREADS) {
    const int j = j0 + tid;
    double X[3] = {0.0, 0.0, 0.0}, bx = 0.0, by = 0.0;
    double2 uv = make_double2(0.0, 0.0);
    bool ok = false;
    if (j < end) ok = rs_obs<CM>(a.r, cam, j, X, uv, bx, by);
    const unsigned long long m = __ballot(ok);
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    __syncthreads();                              // (the readers of the previous counts are done)
    if (lane == 0) wcnt[wv] = __popcll(m);
    __syncthreads();
    const int w0 = wcnt[0], w1 = wcnt[1], w2 = wcnt[2], w3 = wcnt[3];
    const int off = base + (wv > 0 ? w0 : 0) + (wv > 1 ? w1 : 0) + (wv > 2 ? w2 : 0);
    if (ok) {                                     // beg + off + before <= j: inside the camera's segment
      double2* o = (double2*)(a.rec + RN_REC * (size_t)(beg + off + before));
      o[0] = make_double2(X[0], X[1]); o[1] = make_double2(X[2], uv.x); o[2] = make_double2(uv.y, (double)j); o[3] = make_double2(bx, by);
    }
    base += w0 + w1 + w2 + w3;
  }
  if (tid == 0) a.cnt[c] = base;
}

// ------------------------------------------------------------------------------------------------ hypotheses and scores
template <class CM>
__global__ void __launch_bounds__(RN_THREADS) k_ransac_score(const RansacArgs a) {
  __shared__ double tile[RN_TILE * RN_LDS];
  __shared__ double red[2 * HY_WAVES];
  const int c = blockIdx.x, blk = blockIdx.y, tid = threadIdx.x;
  const int n = a.cnt[c];
  double* out = a.best + RN_BEST * ((size_t)c * a.n_blk + blk);
  if (n < 4) {                                    // (workgroup-uniform) FEW_POINTS, or not selected: k_ransac_lo reads no record
    hy_void_block(out);
    return;
  }
  const int beg = a.r.offk[c * (NPART + 1)];
  const double* rec = a.rec + RN_REC * (size_t)beg;
  double cam[CM::CAM];
  CM::load_cam_vec(a.r.t.cs, a.r.t.intr, c, cam);
  const int h = blk * RN_THREADS + tid;
  double R[4][9], t[4][3];
#pragma unroll
  for (int s = 0; s < 4; ++s) {                   // an empty slot projects every point to depth 0: behind, thr^2 each
#pragma unroll
    for (int q = 0; q < 9; ++q) R[s][q] = 0.0;
#pragma unroll
    for (int q = 0; q < 3; ++q) t[s][q] = 0.0;
  }
  int mask = 0;
  if (h < a.n_hyp) {
    int idx[3];
    hy_sample(a.seed, c, h, n, idx);
    mask = rn_p3p<CM>(rec + RN_REC * (size_t)idx[0], rec + RN_REC * (size_t)idx[1], rec + RN_REC * (size_t)idx[2], a.r.t.min_depth, R, t);
#pragma unroll
    for (int s = 0; s < 4; ++s)
      if (!(mask >> s & 1)) {
#pragma unroll
        for (int q = 0; q < 9; ++q) R[s][q] = 0.0;
#pragma unroll
        for (int q = 0; q < 3; ++q) t[s][q] = 0.0;
      }
  }
  const double thr2 = a.r.t.max_px * a.r.t.max_px;
  double cost[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i0 = 0; i0 < n; i0 += RN_TILE) {
    const int m = min(RN_TILE, n - i0);
    __syncthreads();                              // (the readers of the previous tile are done)
    if (tid < m) {
      const double2* s = (const double2*)(rec + RN_REC * (size_t)(i0 + tid));
      const double2 q0 = s[0], q1 = s[1], q2 = s[2];
      double2* d = (double2*)(tile + RN_LDS * tid);
      d[0] = q0; d[1] = q1; d[2] = q2;
    }
    __syncthreads();
    for (int i = 0; i < m; ++i) {                 // every lane reads the same address: an LDS broadcast
      const double2* s = (const double2*)(tile + RN_LDS * i);
      const double2 q0 = s[0], q1 = s[1];
      const double v = tile[RN_LDS * i + 4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        double e2;
        const bool front = rn_err2<CM>(R[k], t[k], cam, a.r.t, q0.x, q0.y, q1.x, q1.y, v, e2);
        cost[k] += front ? fmin(e2, thr2) : thr2;
      }
    }
  }
  // the lane's best slot, then the block's best (cost, 4 h + slot)
  double bc = HY_INF, bk = HY_INF, gc, gk;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if ((mask >> k & 1) && cost[k] < bc) { bc = cost[k]; bk = (double)(4 * h + k); }
  const bool mine = hy_block_best(bc, bk, red, gc, gk);
  if (!(gc < HY_INF)) {
    hy_void_block(out);
    return;
  }
  if (mine) {
    const int k = (int)gk & 3;
    double Rw[9], tw[3];
#pragma unroll
    for (int q = 0; q < 9; ++q) Rw[q] = k == 0 ? R[0][q] : k == 1 ? R[1][q] : k == 2 ? R[2][q] : R[3][q];
#pragma unroll
    for (int q = 0; q < 3; ++q) tw[q] = k == 0 ? t[0][q] : k == 1 ? t[1][q] : k == 2 ? t[2][q] : t[3][q];
    out[0] = gc; out[1] = gk;
#pragma unroll
    for (int q = 0; q < 9; ++q) out[2 + q] = Rw[q];
#pragma unroll
    for (int q = 0; q < 3; ++q) out[11 + q] = tw[q];
  }
}

// ------------------------------------------------------------------------------------------------ local optimisation, measures
template <class CM>
__global__ void __launch_bounds__(RS_THREADS) k_ransac_lo(const RansacArgs a) {
  __shared__ double lds[RS_WAVES * RS_NSUM];
  const ResectArgs& ra = a.r;
  const int c = blockIdx.x, tid = threadIdx.x;
  double* o = ra.out + RS_OUT * (size_t)c;
  double x[6];
#pragma unroll
  for (int q = 0; q < 6; ++q) x[q] = ra.cams[6 * (size_t)c + q];
  if (ra.sel && !ra.sel[c]) { rs_write_unrefined(o, x, RS_OK); return; }   // (workgroup-uniform, like every branch below)
  const int beg = ra.offk[c * (NPART + 1)], end = ra.offk[c * (NPART + 1) + NPART];
  const double n = (double)a.cnt[c];
  int status = RS_OK;
  if (n < 4.0) status = RS_FEW_POINTS;
  else {
    // the lowest (cost, 4 h + slot) over the score blocks, in block order: the same in every lane
    const double* b = a.best + RN_BEST * (size_t)c * a.n_blk;
    double gc, gk;
    const int win = hy_winner<RN_BEST>(b, a.n_blk, gc, gk);
    if (!(gc < HY_INF)) status = RS_DEGENERATE;   // every hypothesis void
    else {
      double R[9];
#pragma unroll
      for (int q = 0; q < 9; ++q) R[q] = b[RN_BEST * win + 2 + q];
      sim_log_map(R, x);
#pragma unroll
      for (int q = 0; q < 3; ++q) x[3 + q] = b[RN_BEST * win + 11 + q];
#pragma unroll
      for (int q = 0; q < 6; ++q) if (!sim_finite(x[q])) status = RS_DEGENERATE;
      if (status != RS_OK) {
#pragma unroll
        for (int q = 0; q < 6; ++q) x[q] = ra.cams[6 * (size_t)c + q];
      }
    }
  }
  if (status != RS_OK) { rs_write_unrefined(o, x, status); return; }   // the current pose
  double cam[CM::CAM], M[9];
  CM::load_cam_vec(ra.t.cs, ra.t.intr, c, cam);   // (the BAL intrinsics; rs_pose overwrites R | t)
  for (int round = 0; round < a.lo_rounds && status == RS_OK; ++round) {
    // the consensus set at the round's frozen pose: every lane writes the bytes it reads back in the passes (same stride)
    rs_pose<CM>(x, cam, M);
    double cn[1] = {0.0};
    for (int j = beg + tid; j < end; j += RS_THREADS) {
      double X[3], ru, rv;
      double2 uv;
      typename CM::template Obs<double> g;
      const bool front = rs_residual<CM>(ra, cam, j, ru, rv, uv, X, g) > 0;
      const unsigned char in = front && sqrt(ru * ru + rv * rv) <= ra.t.max_px ? 1 : 0;
      a.cons[j] = in;
      cn[0] += (double)in;
    }
    rs_block_sums<1>(cn, lds);
    if (!(cn[0] > 0.0)) break;
    rs_refine<CM, true>(ra, cam, M, beg, end, x, status, lds, a.cons);   // ba_resect's step 3 on the set
  }
  // ba_resect's steps 4 and 5; obs_inlier is the inlier test of its measures
  rs_finish<CM>(ra, cam, M, beg, end, x, n, status, lds, o, a.inl, a.c_orig);
}

}  // namespace ba
