// Dense small-matrix helpers of the stand-alone features (triangulation, tracks, similarity, resection): the two Jacobi
// iterations on register-resident N x N matrices, the damped Cholesky step of the refinements, the rotation log map, the
// finiteness test and the quiet NaN.  Every loop bound is a compile-time constant: the matrices stay in registers, no entry is
// indexed dynamically.
#pragma once
#include <hip/hip_runtime.h>
#include "ba_device.hpp"

namespace ba {

__host__ __device__ __forceinline__ bool sim_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }   // false for NaN
constexpr double HY_NAN = __builtin_nan("");   // the quiet NaN 0x7ff8000000000000: an output without a value

// (A + lam diag A) dx = -g by Cholesky: c holds A packed upper N x N row by row (UT) and g behind it.  hold_last: the last
// parameter is held, its pivot 1 and its step 0 (its row and column of c are zero).  false: a pivot <= 0
template <int N, int M>
__device__ inline bool lm_step(const double (&c)[M], const double lam, const bool hold_last, double (&dx)[N]) {
  constexpr int G = N * (N + 1) / 2;
  static_assert(M >= G + N, "c holds the packed matrix and the gradient");
  double L[N][N];
#pragma unroll
  for (int j = 0; j < N; ++j) {
    double s = (j == N - 1 && hold_last) ? 1.0 : c[UT(N, j, j)] * (1.0 + lam);
#pragma unroll
    for (int k = 0; k < N; ++k) if (k < j) s -= L[j][k] * L[j][k];
    if (!(s > 0.0)) return false;
    const double l = sqrt(s);
    L[j][j] = l;
#pragma unroll
    for (int i = 0; i < N; ++i) if (i > j) {
      double t = c[UT(N, j, i)];
#pragma unroll
      for (int k = 0; k < N; ++k) if (k < j) t -= L[i][k] * L[j][k];
      L[i][j] = t / l;
    }
  }
  double y[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    double t = -c[G + i];
#pragma unroll
    for (int k = 0; k < N; ++k) if (k < i) t -= L[i][k] * y[k];
    y[i] = t / L[i][i];
  }
#pragma unroll
  for (int i = N - 1; i >= 0; --i) {
    double t = y[i];
#pragma unroll
    for (int k = 0; k < N; ++k) if (k > i) t -= L[k][i] * dx[k];
    dx[i] = t / L[i][i];
  }
  return true;
}

// cofactors of a packed symmetric 3 x 3: 00 01 02 11 12 22
__device__ __forceinline__ void sym3_cof(const double (&A)[6], double (&C)[6]) {
  C[0] = A[3] * A[5] - A[4] * A[4]; C[1] = A[2] * A[4] - A[1] * A[5]; C[2] = A[1] * A[4] - A[2] * A[3];
  C[3] = A[0] * A[5] - A[2] * A[2]; C[4] = A[1] * A[2] - A[0] * A[4]; C[5] = A[0] * A[3] - A[1] * A[1];
}

// Cyclic Jacobi on a symmetric N x N (full storage), at most SWEEPS sweeps: A <- V^T A V diagonal, columns of V the
// eigenvectors.  A rotation is skipped once |a_pq| <= 1e-17 sqrt(|a_pp a_qq|) (the relative criterion: the small eigenvalue
// keeps its digits).
template <int N, int SWEEPS>
__device__ inline void jacobi_eig(double (&A)[N][N], double (&V)[N][N]) {
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = 0; j < N; ++j) V[i][j] = (i == j) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < SWEEPS; ++sweep) {
    bool rotated = false;
#pragma unroll
    for (int p = 0; p < N - 1; ++p) {
#pragma unroll
      for (int q = p + 1; q < N; ++q) {
        const double apq = A[p][q];
        if (!(fabs(apq) > 1e-17 * sqrt(fabs(A[p][p] * A[q][q])))) continue;
        rotated = true;
        const double zeta = (A[q][q] - A[p][p]) / (2.0 * apq);
        const double tt = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(zeta * zeta + 1.0));
        const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
#pragma unroll
        for (int k = 0; k < N; ++k) {
          const double ap = A[k][p], aq = A[k][q];
          A[k][p] = c * ap - s * aq;
          A[k][q] = s * ap + c * aq;
        }
#pragma unroll
        for (int k = 0; k < N; ++k) {
          const double ap = A[p][k], aq = A[q][k];
          A[p][k] = c * ap - s * aq;
          A[q][k] = s * ap + c * aq;
          const double vp = V[k][p], vq = V[k][q];
          V[k][p] = c * vp - s * vq;
          V[k][q] = s * vp + c * vq;
        }
      }
    }
    if (!rotated) break;
  }
}

// One-sided (Hestenes) Jacobi SVD of the N x N A itself, at most SWEEPS sweeps: plane rotations from the right make the
// columns of U = A V mutually orthogonal; their norms are then the singular values and the columns of V the right singular
// vectors.  Working on A rather than on A^T A keeps the conditioning of the problem (A^T A squares it: for a low-parallax
// pair -- a new keyframe right after the last one -- the eigenvector of the smallest eigenvalue of A^T A loses half the
// digits; measured against LAPACK's SVD at a 1 mm baseline: 7e-8 relative through A^T A, 3e-10 through A).
template <int N, int SWEEPS>
__host__ __device__ inline void jacobi_svd(double (&U)[N][N], double (&V)[N][N]) {
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = 0; j < N; ++j) V[i][j] = (i == j) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < SWEEPS; ++sweep) {
    bool rotated = false;
#pragma unroll
    for (int p = 0; p < N - 1; ++p) {
#pragma unroll
      for (int q = p + 1; q < N; ++q) {
        double al = 0.0, be = 0.0, ga = 0.0;
#pragma unroll
        for (int k = 0; k < N; ++k) { al += U[k][p] * U[k][p]; be += U[k][q] * U[k][q]; ga += U[k][p] * U[k][q]; }
        if (!(fabs(ga) > 1e-17 * sqrt(al * be))) continue;            // already orthogonal to round-off
        rotated = true;
        const double zeta = (be - al) / (2.0 * ga);
        const double tt = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(zeta * zeta + 1.0));
        const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
#pragma unroll
        for (int k = 0; k < N; ++k) {
          const double up = U[k][p], uq = U[k][q];
          U[k][p] = c * up - s * uq;
          U[k][q] = s * up + c * uq;
          const double vp = V[k][p], vq = V[k][q];
          V[k][p] = c * vp - s * vq;
          V[k][q] = s * vp + c * vq;
        }
      }
    }
    if (!rotated) break;
  }
}

template <int P, int Q>
__host__ __device__ __forceinline__ void sim_order(double (&U)[3][3], double (&V)[3][3], double (&n2)[3]) {   // larger norm first
  if (n2[P] >= n2[Q]) return;
  const double t = n2[P]; n2[P] = n2[Q]; n2[Q] = t;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double a = U[k][P]; U[k][P] = U[k][Q]; U[k][Q] = a;
    const double b = V[k][P]; V[k][P] = V[k][Q]; V[k][Q] = b;
  }
}

// rotation matrix (row-major, orthogonal to rounding) -> rotation vector, |rvec| <= pi ("log map" of ba_similarity.hpp's header)
__host__ __device__ inline void sim_log_map(const double* __restrict__ R, double* __restrict__ rvec) {
  const double tr = R[0] + R[4] + R[8];
  double w, x, y, z;
  if (tr >= R[0] && tr >= R[4] && tr >= R[8]) {
    w = 1.0 + tr; x = R[7] - R[5]; y = R[2] - R[6]; z = R[3] - R[1];
  } else if (R[0] >= R[4] && R[0] >= R[8]) {
    w = R[7] - R[5]; x = 1.0 + R[0] - R[4] - R[8]; y = R[1] + R[3]; z = R[2] + R[6];
  } else if (R[4] >= R[8]) {
    w = R[2] - R[6]; x = R[1] + R[3]; y = 1.0 + R[4] - R[0] - R[8]; z = R[5] + R[7];
  } else {
    w = R[3] - R[1]; x = R[2] + R[6]; y = R[5] + R[7]; z = 1.0 + R[8] - R[0] - R[4];
  }
  // (each case is 4 q_k q times the quaternion, q_k its largest component: the common factor goes with the normalisation)
  const double in = 1.0 / sqrt(w * w + x * x + y * y + z * z);
  w *= in; x *= in; y *= in; z *= in;
  if (w < 0.0) { w = -w; x = -x; y = -y; z = -z; }
  const double vn = sqrt(x * x + y * y + z * z);
  const double k = (vn < 1e-10) ? 2.0 / w : 2.0 * atan2(vn, w) / vn;
  rvec[0] = k * x; rvec[1] = k * y; rvec[2] = k * z;
}

}  // namespace ba
