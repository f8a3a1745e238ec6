// Host side of the covariance-weighted spherical resection (include/sba_hip.h: sba_problem_*_resection_weighted,
// sba_problem_resection_covariance).  HIP-free; the kernels are in sba_resection_weighted.hip, the per-match device code in
// sba_resection_weighted_core.hpp.  Notation of sba_resection.hpp, plus per match the landmark's covariance Sigma_i:
//
//   S_i = cov_scale R(w_ref) Sigma_i R(w_ref)^T + bearing_sigma^2 d_i*(ref)^2 (y . y) I        frozen at a reference pose
//   M_i = S^-1 - S^-1 y y^T S^-1 / (y^T S^-1 y) = B (B^T S B)^-1 B^T                           any 3 x 2 B spanning y-perp
//   s_i = r_i^T M_i r_i,   cost = 1/2 sum rho(s_i),   H = sum w_i [A | I]^T M_i [A | I],   g = sum w_i [A | I]^T M_i r_i
//
// The basis depends on the data only: k = the index of the smallest |y_k| (the lowest on ties), b1 = e_k x y, b2 = y x b1.
// With C = B^T S B = G G^T (Cholesky, lower) the handle stores q = (1 / g11, -g21 / (g11 g22), 1 / g22), the entries of
// G^-1; W = G^-1 B^T (2 x 3), z = W r, s = z . z, J_z = [W A | W] and M = W^T W.  A match whose Sigma row is not finite, whose
// C is not positive definite or whose d* at the reference is not finite stores q = 0: weight zero.
// Here: what host and device share of that (basis, factor, W, the M row), the option checks, the 6 x 6 inverse and the
// finish of the pose covariance.
#pragma once
#include <cmath>

#include "../../include/sba_hip.h"
#include "sba_resection.hpp"

#if defined(__clang__)
#pragma STDC FP_CONTRACT OFF
#endif

namespace sba {

// b1 = e_k x y, b2 = y x b1 with k the index of the smallest |y_k|, the lowest on ties.  No square root, no division.
SBA_HD inline void resect_weight_basis(const double y[3], double b1[3], double b2[3]) {
  const double a0 = std::fabs(y[0]), a1 = std::fabs(y[1]), a2 = std::fabs(y[2]);
  const bool k0 = a0 <= a1 && a0 <= a2, k1 = !k0 && a1 <= a2;
  b1[0] = k0 ? 0.0 : (k1 ? y[2] : -y[1]);
  b1[1] = k0 ? -y[2] : (k1 ? 0.0 : y[0]);
  b1[2] = k0 ? y[1] : (k1 ? -y[0] : 0.0);
  b2[0] = y[1] * b1[2] - y[2] * b1[1];
  b2[1] = y[2] * b1[0] - y[0] * b1[2];
  b2[2] = y[0] * b1[1] - y[1] * b1[0];
}

// S (xx, yy, zz, xy, xz, yz) -> q, the three entries of G^-1 with B^T S B = G G^T.  false (and q = 0) unless the 2 x 2 matrix is
// positive definite and every entry of q is finite and its diagonal positive.
SBA_HD inline bool resect_weight_factor(const double S[6], const double b1[3], const double b2[3], double q[3]) {
  const double u0 = S[0] * b1[0] + S[3] * b1[1] + S[4] * b1[2], u1 = S[3] * b1[0] + S[1] * b1[1] + S[5] * b1[2],
               u2 = S[4] * b1[0] + S[5] * b1[1] + S[2] * b1[2];
  const double v0 = S[0] * b2[0] + S[3] * b2[1] + S[4] * b2[2], v1 = S[3] * b2[0] + S[1] * b2[1] + S[5] * b2[2],
               v2 = S[4] * b2[0] + S[5] * b2[1] + S[2] * b2[2];
  const double c11 = b1[0] * u0 + b1[1] * u1 + b1[2] * u2, c12 = b2[0] * u0 + b2[1] * u1 + b2[2] * u2,
               c22 = b2[0] * v0 + b2[1] * v1 + b2[2] * v2;
  const double g11 = std::sqrt(c11), g21 = c12 / g11, d = c22 - g21 * g21, g22 = std::sqrt(d);
  const double q0 = 1.0 / g11, q2 = 1.0 / g22, q1 = -g21 * q0 * q2;
  const bool ok = c11 > 0.0 && d > 0.0 && q0 > 0.0 && q2 > 0.0 && std::isfinite(q0) && std::isfinite(q1) && std::isfinite(q2);
  q[0] = ok ? q0 : 0.0; q[1] = ok ? q1 : 0.0; q[2] = ok ? q2 : 0.0;
  return ok;
}

// W = G^-1 B^T: row 0 = q0 b1, row 1 = q1 b1 + q2 b2
SBA_HD inline void resect_weight_whiten(const double q[3], const double b1[3], const double b2[3], double W[2][3]) {
  for (int k = 0; k < 3; ++k) {
    W[0][k] = q[0] * b1[k];
    W[1][k] = q[1] * b1[k] + q[2] * b2[k];
  }
}

// M = W^T W as the row (xx, yy, zz, xy, xz, yz)
SBA_HD inline void resect_weight_row(const double W[2][3], double M[6]) {
  M[0] = W[0][0] * W[0][0] + W[1][0] * W[1][0];
  M[1] = W[0][1] * W[0][1] + W[1][1] * W[1][1];
  M[2] = W[0][2] * W[0][2] + W[1][2] * W[1][2];
  M[3] = W[0][0] * W[0][1] + W[1][0] * W[1][1];
  M[4] = W[0][0] * W[0][2] + W[1][0] * W[1][2];
  M[5] = W[0][1] * W[0][2] + W[1][1] * W[1][2];
}

// The stored factor of one match and its bearing -> the row of M (what resect_weight_rows_kernel writes).
SBA_HD inline void resect_weight_expand(const double q[3], const double y[3], double M[6]) {
  double b1[3], b2[3], W[2][3];
  resect_weight_basis(y, b1, b2);
  resect_weight_whiten(q, b1, b2, W);
  resect_weight_row(W, M);
}

// Option checks of the entry points: nullptr = fine, otherwise what is wrong (SBA_ERR_INVALID_ARG).
inline const char* resect_weight_check_scale(double cov_scale) {
  return std::isfinite(cov_scale) && cov_scale > 0.0 ? nullptr : "cov_scale must be finite and > 0";
}
inline const char* resect_weight_check_sigma(double bearing_sigma) {
  return std::isfinite(bearing_sigma) && bearing_sigma >= 0.0 ? nullptr : "bearing_sigma must be finite and >= 0";
}
inline const char* resect_weight_check_rounds(int reweight_rounds) {
  return reweight_rounds >= 1 && reweight_rounds <= 8 ? nullptr : "reweight_rounds must be 1 .. 8";
}

// inv = H^-1 of a symmetric positive definite 6 x 6 matrix (row-major) through H = L L^T: inv = L^-T L^-1, symmetric to the
// bit.  false (inv untouched) when a pivot is not positive or a result not finite.
inline bool resect_cov_inverse(const double* H, double* inv) {
  constexpr int n = 6;
  double L[n][n] = {}, Li[n][n] = {};
  for (int j = 0; j < n; ++j) {
    double d = H[n * j + j];
    for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
    if (!(d > 0.0) || !std::isfinite(d)) return false;
    L[j][j] = std::sqrt(d);
    for (int i = j + 1; i < n; ++i) {
      double s = H[n * i + j];
      for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
      L[i][j] = s / L[j][j];
    }
  }
  for (int j = 0; j < n; ++j) {      // column j of L^-1 by forward substitution
    Li[j][j] = 1.0 / L[j][j];
    for (int i = j + 1; i < n; ++i) {
      double s = 0.0;
      for (int k = j; k < i; ++k) s -= L[i][k] * Li[k][j];
      Li[i][j] = s / L[i][i];
    }
  }
  double out[n * n];
  for (int a = 0; a < n; ++a)
    for (int b = a; b < n; ++b) {
      double s = 0.0;
      for (int k = b; k < n; ++k) s += Li[k][a] * Li[k][b];
      if (!std::isfinite(s)) return false;
      out[n * a + b] = s;
      out[n * b + a] = s;
    }
  for (int i = 0; i < n * n; ++i) inv[i] = out[i];
  return true;
}

// The finish of sba_problem_resection_covariance: the reduce pass's row at the point, n and the freeze's n_zero_weight ->
// *out.  SBA_ERR_NUMERIC (*why names the reason, *out untouched): dof <= 0, non-finite sums or a failed factorisation.
inline int resect_cov_finish(const double* row, long long n, long long n_zero_weight, sba_resection_cov* out, const char** why) {
  const long long n_used = n - n_zero_weight, dof = 2 * n_used - 6;
  if (dof <= 0) { *why = "the pose covariance needs more than 3 matches with weight (dof = 2 n_used - 6 <= 0)"; return SBA_ERR_NUMERIC; }
  if (!resect_row_finite(row)) { *why = "non-finite weighted resection sums"; return SBA_ERR_NUMERIC; }
  sba_normal_eq ne;
  resect_expand_row(row, &ne, nullptr);
  sba_resection_cov res = sba_resection_cov{};
  if (!resect_cov_inverse(ne.H, res.cov)) { *why = "the weighted normal matrix is not positive definite: the matches do not fix the pose"; return SBA_ERR_NUMERIC; }
  res.cost = ne.cost; res.sum_w = ne.sum_w; res.n_outlier = ne.n_outlier;
  res.n_used = n_used; res.n_zero_weight = n_zero_weight; res.dof = dof;
  res.sigma2 = 2.0 * ne.cost / static_cast<double>(dof);
  *out = res;
  return SBA_OK;
}

}  // namespace sba

#if defined(__clang__)
#pragma STDC FP_CONTRACT DEFAULT
#endif
