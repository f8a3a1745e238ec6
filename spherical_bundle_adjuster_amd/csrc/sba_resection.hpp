// Host side of the spherical resection (include/sba_hip.h: sba_problem_*_resection*): a new frame's pose from landmarks
// X_i = d1_i x1_i and the frame's bearings y_i = x2_i, all six degrees of freedom, no gauge.  HIP-free; the kernels are in
// sba_resection.hip, the per-match arithmetic in sba_resection_core.hpp.
//
//   e_i(w, t, d) = d y_i - R(w) X_i + t,   c_i = -R(w) X_i + t,   d_i* = -(y_i . c_i) / (y_i . y_i)   (the minimiser over d)
//   r_i = c_i + d_i* y_i = P_i c_i,        P_i = I - y_i y_i^T / (y_i . y_i),   cost = 1/2 sum rho(|r_i|^2)
//   d r_i / d (w, t) = P_i [A_i | I]       exactly (P_i depends on the data only), A_i = [Gn_0 X_i | Gn_1 X_i | Gn_2 X_i]
//   H = sum w_i [A | I]^T P_i [A | I],     g = sum w_i [A | I]^T r_i            (P idempotent, w = rho')
//
// Here: the layout of the reduce pass's row and its expansion into normal equations, the rotation-matrix -> rotation-vector
// log map, and the finish of the linear starting point (DLT).  With N = [M | tau] (3 x 4) and X~ = (X, -1), the bearing is
// parallel to N X~, so [y]x N X~ = 0 is linear in the 12 entries of N; the moment matrix of the column-major vec(N) is
//   sum (X~ X~^T) (x) Q_i,   Q_i = (y . y) I - y y^T                              10 x 6 = 60 distinct sums
// and N is its null vector.  d y = R X - t makes M = s R and tau = s t with one s, whose sign det M > 0 fixes.
#pragma once
#include <cfloat>
#include <cmath>

#include "../../include/sba_hip.h"
#include "sba_epipolar.hpp"

#ifndef SBA_HD
#if defined(__HIPCC__)
#define SBA_HD __host__ __device__
#else
#define SBA_HD
#endif
#endif
#if defined(__clang__)
#pragma STDC FP_CONTRACT OFF
#endif

// The row the reduce pass publishes: the upper triangle of H row by row over [rot | tran], g, then the scalars.
enum {
  SBA_RESECT_H = 0,
  SBA_RESECT_G = 21,
  SBA_RESECT_COST = 27,
  SBA_RESECT_SW = 28,
  SBA_RESECT_NOUT = 29,
  SBA_RESECT_NBEHIND = 30,    // matches with d_i* <= 0: counted, otherwise treated like any other match
  SBA_RESECT_COUNT = 31,
  SBA_RESECT_SIZE = 32
};
// The moments pass: slot 6 * p + q = sum (X~ X~^T)[a][b] Q[c][d] with p the index of (a <= b) in the upper triangle of a
// 4 x 4 matrix row by row and q that of (c <= d) in a 3 x 3 one; then the number of matches.
enum { SBA_RESECT_MOMENTS = 60, SBA_RESECT_MOM_N = 60, SBA_RESECT_MOM_COUNT = 61 };

namespace sba {

SBA_HD inline void resect_expand_row(const double* row, sba_normal_eq* ne, double* n_behind) {
  *ne = sba_normal_eq{};
  int k = SBA_RESECT_H;
  for (int a = 0; a < 6; ++a)
    for (int b = a; b < 6; ++b) {
      ne->H[6 * a + b] = row[k];
      ne->H[6 * b + a] = row[k];
      ++k;
    }
  for (int a = 0; a < 6; ++a) ne->g[a] = row[SBA_RESECT_G + a];
  ne->cost = row[SBA_RESECT_COST];
  ne->sum_w = row[SBA_RESECT_SW];
  ne->n_outlier = row[SBA_RESECT_NOUT];
  if (n_behind) *n_behind = row[SBA_RESECT_NBEHIND];
}

SBA_HD inline bool resect_row_finite(const double* row) {
  for (int k = 0; k < SBA_RESECT_COUNT; ++k)
    if (!std::isfinite(row[k])) return false;
  return true;
}

// Rotation matrix (row-major, orthogonal up to rounding) -> rotation vector with angle in [0, pi].  Through the unit
// quaternion, its largest component taken from the diagonal and the others from the off-diagonal sums and differences
// (no cancellation at any angle); angle = 2 atan2(|v|, q0), so neither acos near 0 nor the vanishing antisymmetric part
// near pi is relied on.  Also exact to rounding on the small-angle form R = I + [w]x of rotation_and_derivatives.
SBA_HD inline void rotation_log(const double* R, double w[3]) {
  const double tr = R[0] + R[4] + R[8];
  double q0, q1, q2, q3;
  if (tr > 0.0) {
    const double s = 2.0 * std::sqrt(tr + 1.0);
    q0 = 0.25 * s; q1 = (R[7] - R[5]) / s; q2 = (R[2] - R[6]) / s; q3 = (R[3] - R[1]) / s;
  } else if (R[0] >= R[4] && R[0] >= R[8]) {
    const double s = 2.0 * std::sqrt(1.0 + R[0] - R[4] - R[8]);
    q0 = (R[7] - R[5]) / s; q1 = 0.25 * s; q2 = (R[1] + R[3]) / s; q3 = (R[2] + R[6]) / s;
  } else if (R[4] >= R[8]) {
    const double s = 2.0 * std::sqrt(1.0 + R[4] - R[0] - R[8]);
    q0 = (R[2] - R[6]) / s; q1 = (R[1] + R[3]) / s; q2 = 0.25 * s; q3 = (R[5] + R[7]) / s;
  } else {
    const double s = 2.0 * std::sqrt(1.0 + R[8] - R[0] - R[4]);
    q0 = (R[3] - R[1]) / s; q1 = (R[2] + R[6]) / s; q2 = (R[5] + R[7]) / s; q3 = 0.25 * s;
  }
  if (q0 < 0.0) { q0 = -q0; q1 = -q1; q2 = -q2; q3 = -q3; }
  const double n = std::sqrt(q1 * q1 + q2 * q2 + q3 * q3);
  const double k = n > 0.0 ? 2.0 * std::atan2(n, q0) / n : 2.0;
  w[0] = k * q1; w[1] = k * q2; w[2] = k * q3;
}

// Cyclic Jacobi eigen-decomposition of a symmetric 12 x 12 matrix: w ascending, V columns = eigenvectors (row-major).
// epi::jacobi_eigen keeps its work arrays at 9 x 9 for the device's sake; this one runs on the host only.
inline void resect_eigen12(const double* A_in, double* w, double* V) {
  constexpr int n = 12;
  double A[n * n];
  for (int i = 0; i < n * n; ++i) A[i] = A_in[i];
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) V[i * n + j] = (i == j) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 64; ++sweep) {
    double off = 0.0, diag = 0.0;
    for (int i = 0; i < n; ++i) {
      diag += A[i * n + i] * A[i * n + i];
      for (int j = i + 1; j < n; ++j) off += A[i * n + j] * A[i * n + j];
    }
    if (off <= 1e-34 * diag || off == 0.0) break;
    for (int p = 0; p < n - 1; ++p)
      for (int q = p + 1; q < n; ++q) {
        const double apq = A[p * n + q];
        if (apq == 0.0) continue;
        const double theta = (A[q * n + q] - A[p * n + p]) / (2.0 * apq);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < n; ++k) {
          const double akp = A[k * n + p], akq = A[k * n + q];
          A[k * n + p] = c * akp - s * akq;
          A[k * n + q] = s * akp + c * akq;
        }
        for (int k = 0; k < n; ++k) {
          const double apk = A[p * n + k], aqk = A[q * n + k];
          A[p * n + k] = c * apk - s * aqk;
          A[q * n + k] = s * apk + c * aqk;
        }
        for (int k = 0; k < n; ++k) {
          const double vkp = V[k * n + p], vkq = V[k * n + q];
          V[k * n + p] = c * vkp - s * vkq;
          V[k * n + q] = s * vkp + c * vkq;
        }
      }
  }
  int order[n];
  for (int i = 0; i < n; ++i) {
    int j = i - 1;
    for (; j >= 0 && A[i * n + i] < A[order[j] * n + order[j]]; --j) order[j + 1] = order[j];
    order[j + 1] = i;
  }
  double Vs[n * n];
  for (int k = 0; k < n; ++k) {
    w[k] = A[order[k] * n + order[k]];
    for (int i = 0; i < n; ++i) Vs[i * n + k] = V[i * n + order[k]];
  }
  for (int i = 0; i < n * n; ++i) V[i] = Vs[i];
}

// 60 moments -> the symmetric 12 x 12 matrix over the column-major vec([M | tau]): entry (3 a + c, 3 b + d).
inline void resect_expand_moments(const double* mom, double* S) {
  int p = 0;
  for (int a = 0; a < 4; ++a)
    for (int b = a; b < 4; ++b) {
      int q = 0;
      for (int c = 0; c < 3; ++c)
        for (int d = c; d < 3; ++d) {
          const double v = mom[6 * p + q];
          S[12 * (3 * a + c) + 3 * b + d] = v; S[12 * (3 * a + d) + 3 * b + c] = v;
          S[12 * (3 * b + d) + 3 * a + c] = v; S[12 * (3 * b + c) + 3 * a + d] = v;
          ++q;
        }
      ++p;
    }
}

// The DLT finish: null vector, sign (det M > 0), projection of M onto SO(3) (scale = mean singular value), tran = tau /
// scale, log map.  info: the eigenvalues lambda_1 <= lambda_2 and lambda_12, the singular values relative to their mean;
// n and n_behind are the caller's.  Returns SBA_OK or SBA_ERR_NUMERIC (*why names the reason): fewer than 6 matches, a
// null space of more than one dimension at rounding level (lambda_2 <= 12 * 64 * DBL_EPSILON * lambda_12: a planar landmark
// set has four), a non-finite result.  Anything less degenerate is the caller's call from the reported numbers.
inline int resect_dlt_finish(const double* mom, double count, double rot[3], double tran[3], sba_resection_guess_info* info,
                             const char** why) {
  *info = sba_resection_guess_info{};
  info->n = static_cast<long long>(count);
  if (!(count >= 6.0)) { *why = "the linear resection needs at least 6 matches"; return SBA_ERR_NUMERIC; }
  for (int k = 0; k < SBA_RESECT_MOMENTS; ++k)
    if (!std::isfinite(mom[k])) { *why = "non-finite moments"; return SBA_ERR_NUMERIC; }
  double S[144], lam[12], V[144];
  resect_expand_moments(mom, S);
  resect_eigen12(S, lam, V);
  info->lambda1 = lam[0]; info->lambda2 = lam[1]; info->lambda12 = lam[11];
  if (!(lam[1] > 12.0 * 64.0 * DBL_EPSILON * lam[11])) {
    *why = "the landmarks do not fix the pose: the moment matrix has a null space of more than one dimension (a planar set?)";
    return SBA_ERR_NUMERIC;
  }
  double M[9], tau[3];
  for (int c = 0; c < 3; ++c) {
    for (int a = 0; a < 3; ++a) M[3 * c + a] = V[12 * (3 * a + c)];
    tau[c] = V[12 * (9 + c)];
  }
  if (epi::det3(M) < 0.0) {
    for (int i = 0; i < 9; ++i) M[i] = -M[i];
    for (int i = 0; i < 3; ++i) tau[i] = -tau[i];
  }
  double U[9], sv[3], Vt[9], R[9];
  epi::svd3(M, U, sv, Vt);
  epi::mul3(U, Vt, R);
  const double scale = (sv[0] + sv[1] + sv[2]) / 3.0;
  info->scale = scale;
  for (int k = 0; k < 3; ++k) info->sv[k] = sv[k] / scale;
  rotation_log(R, rot);
  for (int k = 0; k < 3; ++k) tran[k] = tau[k] / scale;
  for (int k = 0; k < 3; ++k)
    if (!std::isfinite(rot[k]) || !std::isfinite(tran[k])) { *why = "non-finite linear resection"; return SBA_ERR_NUMERIC; }
  return SBA_OK;
}

}  // namespace sba

#if defined(__clang__)
#pragma STDC FP_CONTRACT DEFAULT
#endif
