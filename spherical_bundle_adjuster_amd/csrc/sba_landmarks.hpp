// Host and device share of the landmark map (include/sba_hip.h: sba_landmarks_*): the fusion of one bearing into one
// landmark, the wave-uniform state of a fusion pass and the option and index checks of the entry points.  HIP-free; the
// kernels are in sba_landmarks.hip, the entry points in sba_landmarks.cpp.  Notation of sba_resection.hpp and
// sba_resection_weighted.hpp, per observation of a landmark X with covariance Sigma (landmark frame) by a bearing y from a
// frame at the pose (w, t) with covariance Sigma_pose over [rot | tran]:
//
//   c = -R X + t,   d* = -(y . c) / (y . y),   r = c + d* y                                     as resect_residual forms them
//   S = R Sigma R^T + bearing_sigma^2 d*^2 (y . y) I + [A | I] Sigma_pose [A | I]^T              A = -[a]x J, a = -R X
//   b1, b2 = resect_weight_basis(y),  q = resect_weight_factor(S, b1, b2),  W = resect_weight_whiten(q, b1, b2)      (2 x 3)
//   u = W r,   chi2 = u . u,   T = Sigma R^T W^T (3 x 2),   X+ = X + T u,   Sigma+ = Sigma - T T^T
//
// W S W^T = I, so this is the Kalman update of X by the 2-vector B^T r, which is linear in X: the exact posterior.  The pose
// term is formed from three matrices the host prepares once per pass, K = J Sigma_rr J^T, L = J Sigma_rt and Sigma_tt:
//   [A | I] Sigma_pose [A | I]^T = [a]x K [a]x^T - [a]x L - ([a]x L)^T + Sigma_tt
// so the device needs neither J nor the 36 entries.  Sigma+ is symmetric by construction (six entries are formed).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/sba_hip.h"
#include "sba_resection_weighted.hpp"
#include "sba_rotation.hpp"

#if defined(__clang__)
#pragma STDC FP_CONTRACT OFF
#endif

namespace sba {

// The class of an observation, tested in this order.
enum { LANDMARK_SKIPPED = 0, LANDMARK_BEHIND = 1, LANDMARK_GATED = 2, LANDMARK_FUSED = 3, LANDMARK_CLASSES = 4 };

// The wave-uniform state of a fusion pass, a by-value kernel argument (scalar registers).
struct LandmarkFuseParams {
  double Rn[9];              // -R(w)
  double t[3];
  double K[6];               // J Sigma_rr J^T   (xx, yy, zz, xy, xz, yz)
  double L[9];               // J Sigma_rt       row-major
  double Ctt[6];             // Sigma_tt         (xx, yy, zz, xy, xz, yz)
  double bearing_sigma2;
  double chi2_gate;
  unsigned long long n;      // landmarks on the handle
  unsigned long long m;      // observations of the pass
  int small_angle;           // rot . rot <= DBL_EPSILON: a = -X (J = I is in K and L already)
  int have_pose_cov;
};

// Option checks of sba_landmarks_fuse: nullptr = fine, otherwise what is wrong (SBA_ERR_INVALID_ARG).  bearing_sigma and
// cov_scale are checked by resect_weight_check_sigma / resect_weight_check_scale.
inline const char* landmark_check_gate(double chi2_gate) {
  return chi2_gate > 0.0 ? nullptr : "chi2_gate must be > 0 (+inf: no gate)";
}
inline const char* landmark_check_pose_cov(const double* c /* 36, row-major, or null */) {
  if (!c) return nullptr;
  for (int a = 0; a < 6; ++a)
    for (int b = 0; b < 6; ++b) {
      if (!std::isfinite(c[6 * a + b])) return "pose_cov must be finite";
      if (c[6 * a + b] != c[6 * b + a]) return "pose_cov must be symmetric to the bit";
    }
  for (int a = 0; a < 6; ++a)
    if (!(c[7 * a] >= 0.0)) return "pose_cov must have a non-negative diagonal";
  return nullptr;
}
// idx == nullptr: the dense form, m == n.  Otherwise m <= n indices, strictly increasing and < n: one pass, after which no
// landmark is written twice and no index reaches the device out of range.
inline const char* landmark_check_index(const int64_t* idx, size_t m, size_t n) {
  if (m > n) return "more observations than landmarks";
  if (!idx) return m == n ? nullptr : "the dense form (idx == NULL) takes one bearing per landmark: m must equal the handle's size";
  int64_t prev = -1;
  for (size_t j = 0; j < m; ++j) {
    if (idx[j] <= prev) return "idx must be strictly increasing (and >= 0)";
    prev = idx[j];
  }
  if (m > 0 && static_cast<uint64_t>(prev) >= n) return "idx out of range";
  return nullptr;
}

// The state of a pass from the pose, its covariance (36, row-major over [rot | tran], or null) and the scalars.
inline void landmark_fuse_fill(unsigned long long n, unsigned long long m, const double rot[3], const double tran[3],
                               const double* pose_cov, double bearing_sigma, double chi2_gate, LandmarkFuseParams* P) {
  double R[9], B[9], J[9];
  rotation_and_derivatives(rot, R, nullptr);
  factored_frame(rot, B, J);
  for (int i = 0; i < 9; ++i) P->Rn[i] = -R[i];
  for (int i = 0; i < 3; ++i) P->t[i] = tran[i];
  for (int i = 0; i < 6; ++i) { P->K[i] = 0.0; P->Ctt[i] = 0.0; }
  for (int i = 0; i < 9; ++i) P->L[i] = 0.0;
  P->have_pose_cov = pose_cov ? 1 : 0;
  if (pose_cov) {
    double JS[9];
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b) {
        JS[3 * a + b] = J[3 * a] * pose_cov[b] + J[3 * a + 1] * pose_cov[6 + b] + J[3 * a + 2] * pose_cov[12 + b];
        P->L[3 * a + b] = J[3 * a] * pose_cov[3 + b] + J[3 * a + 1] * pose_cov[9 + b] + J[3 * a + 2] * pose_cov[15 + b];
      }
    const int ra[6] = {0, 1, 2, 0, 0, 1}, rb[6] = {0, 1, 2, 1, 2, 2};
    for (int k = 0; k < 6; ++k) {
      const int a = ra[k], b = rb[k];
      P->K[k] = JS[3 * a] * J[3 * b] + JS[3 * a + 1] * J[3 * b + 1] + JS[3 * a + 2] * J[3 * b + 2];
      P->Ctt[k] = pose_cov[6 * (3 + a) + 3 + b];
    }
  }
  P->bearing_sigma2 = bearing_sigma * bearing_sigma;
  P->chi2_gate = chi2_gate;
  P->n = n;
  P->m = m;
  P->small_angle = !(rot[0] * rot[0] + rot[1] * rot[1] + rot[2] * rot[2] > DBL_EPSILON) ? 1 : 0;
}

// [a]x M for a 3 x 3 matrix given by its rows m0, m1, m2.
SBA_HD inline void landmark_cross_rows(const double a[3], const double m0[3], const double m1[3], const double m2[3], double out[3][3]) {
  for (int k = 0; k < 3; ++k) {
    out[0][k] = a[1] * m2[k] - a[2] * m1[k];
    out[1][k] = a[2] * m0[k] - a[0] * m2[k];
    out[2][k] = a[0] * m1[k] - a[1] * m0[k];
  }
}

// One bearing into one landmark.  X, Sg (xx, yy, zz, xy, xz, yz): the prior; y: the bearing, any length.  Returns the class;
// *chi2 is NaN for LANDMARK_SKIPPED and the observation's chi^2 otherwise; Xo, So hold the posterior for LANDMARK_FUSED and
// are unspecified otherwise (the caller stores them for LANDMARK_FUSED only).
SBA_HD inline int landmark_fuse_one(const LandmarkFuseParams& P, const double X[3], const double Sg[6], const double y[3], double Xo[3],
                                    double So[6], double* chi2) {
  bool ok = std::isfinite(X[0]) && std::isfinite(X[1]) && std::isfinite(X[2]);
  for (int k = 0; k < 6; ++k) ok = ok && std::isfinite(Sg[k]);
  // c, d*, r exactly as resect_residual: (Rn X) + t summed left to right, r = fma(d*, y, c)
  double rx[3], c[3], r[3];
  for (int k = 0; k < 3; ++k) {
    rx[k] = P.Rn[3 * k] * X[0] + P.Rn[3 * k + 1] * X[1] + P.Rn[3 * k + 2] * X[2];
    c[k] = rx[k] + P.t[k];
  }
  const double yy = y[0] * y[0] + y[1] * y[1] + y[2] * y[2];
  const double inv_yy = 1.0 / yy;
  const double dstar = -(y[0] * c[0] + y[1] * c[1] + y[2] * c[2]) * inv_yy;
  for (int k = 0; k < 3; ++k) r[k] = __builtin_fma(dstar, y[k], c[k]);
  ok = ok && std::isfinite(dstar);
  // S = Rn Sigma Rn^T (Rn = -R: the signs cancel) + iso I + the pose term
  double T1[3][3];
  for (int a = 0; a < 3; ++a) {
    T1[a][0] = P.Rn[3 * a] * Sg[0] + P.Rn[3 * a + 1] * Sg[3] + P.Rn[3 * a + 2] * Sg[4];
    T1[a][1] = P.Rn[3 * a] * Sg[3] + P.Rn[3 * a + 1] * Sg[1] + P.Rn[3 * a + 2] * Sg[5];
    T1[a][2] = P.Rn[3 * a] * Sg[4] + P.Rn[3 * a + 1] * Sg[5] + P.Rn[3 * a + 2] * Sg[2];
  }
  const double iso = P.bearing_sigma2 * (dstar * dstar) * yy;
  double S[6];
  S[0] = T1[0][0] * P.Rn[0] + T1[0][1] * P.Rn[1] + T1[0][2] * P.Rn[2] + iso;
  S[1] = T1[1][0] * P.Rn[3] + T1[1][1] * P.Rn[4] + T1[1][2] * P.Rn[5] + iso;
  S[2] = T1[2][0] * P.Rn[6] + T1[2][1] * P.Rn[7] + T1[2][2] * P.Rn[8] + iso;
  S[3] = T1[0][0] * P.Rn[3] + T1[0][1] * P.Rn[4] + T1[0][2] * P.Rn[5];
  S[4] = T1[0][0] * P.Rn[6] + T1[0][1] * P.Rn[7] + T1[0][2] * P.Rn[8];
  S[5] = T1[1][0] * P.Rn[6] + T1[1][1] * P.Rn[7] + T1[1][2] * P.Rn[8];
  if (P.have_pose_cov) {
    const double a[3] = {P.small_angle ? -X[0] : rx[0], P.small_angle ? -X[1] : rx[1], P.small_angle ? -X[2] : rx[2]};
    const double k0[3] = {P.K[0], P.K[3], P.K[4]}, k1[3] = {P.K[3], P.K[1], P.K[5]}, k2[3] = {P.K[4], P.K[5], P.K[2]};
    double AK[3][3], AL[3][3];
    landmark_cross_rows(a, k0, k1, k2, AK);
    landmark_cross_rows(a, &P.L[0], &P.L[3], &P.L[6], AL);
    // ([a]x K [a]x^T)[i][j] = sum_k AK[i][k] [a]x[j][k]
    const double g00 = a[1] * AK[0][2] - a[2] * AK[0][1], g01 = a[2] * AK[0][0] - a[0] * AK[0][2], g02 = a[0] * AK[0][1] - a[1] * AK[0][0];
    const double g11 = a[2] * AK[1][0] - a[0] * AK[1][2], g12 = a[0] * AK[1][1] - a[1] * AK[1][0];
    const double g22 = a[0] * AK[2][1] - a[1] * AK[2][0];
    S[0] += g00 - (AL[0][0] + AL[0][0]) + P.Ctt[0];
    S[1] += g11 - (AL[1][1] + AL[1][1]) + P.Ctt[1];
    S[2] += g22 - (AL[2][2] + AL[2][2]) + P.Ctt[2];
    S[3] += g01 - (AL[0][1] + AL[1][0]) + P.Ctt[3];
    S[4] += g02 - (AL[0][2] + AL[2][0]) + P.Ctt[4];
    S[5] += g12 - (AL[1][2] + AL[2][1]) + P.Ctt[5];
  }
  double b1[3], b2[3], q[3], W[2][3];
  resect_weight_basis(y, b1, b2);
  ok = resect_weight_factor(S, b1, b2, q) && ok;
  resect_weight_whiten(q, b1, b2, W);
  const double u0 = W[0][0] * r[0] + W[0][1] * r[1] + W[0][2] * r[2], u1 = W[1][0] * r[0] + W[1][1] * r[1] + W[1][2] * r[2];
  const double s = u0 * u0 + u1 * u1;
  // T = Sigma R^T W^T: column k = Sigma v_k with v_k = R^T W_k^T = -(Rn^T W_k^T)
  double Tm[3][2];
  for (int k = 0; k < 2; ++k) {
    const double v0 = -(P.Rn[0] * W[k][0] + P.Rn[3] * W[k][1] + P.Rn[6] * W[k][2]), v1 = -(P.Rn[1] * W[k][0] + P.Rn[4] * W[k][1] + P.Rn[7] * W[k][2]),
                 v2 = -(P.Rn[2] * W[k][0] + P.Rn[5] * W[k][1] + P.Rn[8] * W[k][2]);
    Tm[0][k] = Sg[0] * v0 + Sg[3] * v1 + Sg[4] * v2;
    Tm[1][k] = Sg[3] * v0 + Sg[1] * v1 + Sg[5] * v2;
    Tm[2][k] = Sg[4] * v0 + Sg[5] * v1 + Sg[2] * v2;
  }
  for (int k = 0; k < 3; ++k) Xo[k] = X[k] + (Tm[k][0] * u0 + Tm[k][1] * u1);
  So[0] = Sg[0] - (Tm[0][0] * Tm[0][0] + Tm[0][1] * Tm[0][1]);
  So[1] = Sg[1] - (Tm[1][0] * Tm[1][0] + Tm[1][1] * Tm[1][1]);
  So[2] = Sg[2] - (Tm[2][0] * Tm[2][0] + Tm[2][1] * Tm[2][1]);
  So[3] = Sg[3] - (Tm[0][0] * Tm[1][0] + Tm[0][1] * Tm[1][1]);
  So[4] = Sg[4] - (Tm[0][0] * Tm[2][0] + Tm[0][1] * Tm[2][1]);
  So[5] = Sg[5] - (Tm[1][0] * Tm[2][0] + Tm[1][1] * Tm[2][1]);
  for (int k = 0; k < 3; ++k) ok = ok && std::isfinite(Xo[k]);
  for (int k = 0; k < 6; ++k) ok = ok && std::isfinite(So[k]);
  *chi2 = ok ? s : NAN;
  if (!ok) return LANDMARK_SKIPPED;
  if (dstar <= 0.0) return LANDMARK_BEHIND;
  if (s > P.chi2_gate) return LANDMARK_GATED;
  return LANDMARK_FUSED;
}

}  // namespace sba

#if defined(__clang__)
#pragma STDC FP_CONTRACT DEFAULT
#endif
