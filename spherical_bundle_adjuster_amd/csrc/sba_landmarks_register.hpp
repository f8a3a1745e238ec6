// Host and device share of the joint registration of a frame against the landmark map (include/sba_hip.h:
// sba_landmarks_register, sba_landmarks_eval_register): the pose (w, t) and every observed landmark solved together.  HIP-free;
// the kernels are in sba_landmarks_register.hip, the entry points in sba_landmarks.cpp.  Notation of sba_landmarks.hpp and
// sba_resection_weighted.hpp.  The objective, with the prior X_j ~ N(Xb_j, Sigma_j) of the map's rows and the bearing y_j
// measured with isotropic noise s_j^2 = bearing_sigma^2 d*_j^2 (y_j . y_j) across the ray, FROZEN at the start pose and Xb_j:
//
//   F = sum_j [ |B_j^T (-R X_j + t)|^2 / s_j^2 + (X_j - Xb_j)^T Sigma_j^-1 (X_j - Xb_j) ]                  no pose prior
//
// With the pose held the landmark part is linear-Gaussian, so every landmark is eliminated exactly (variable projection, the
// update landmark_fuse_one does) and a six-parameter problem remains.  Per observation at a pose:
//
//   c = -R Xb + t,   d* = -(y . c) / (y . y),   r = c + d* y,   S = R Sigma R^T + s_j^2 I
//   b1, b2 = resect_weight_basis(y),  q = resect_weight_factor(S, b1, b2),  W = resect_weight_whiten(q, b1, b2)      (2 x 3)
//   u = W r,   chi2 = u . u,   T = Sigma R^T W^T,   Xh = Xb + T u (the minimiser over X_j at this pose),   Sigma_cond = Sigma - T T^T
//   J_w = W [A(Xh) | I]   (2 x 6),   A = -[a]x J with a = -R Xh (small angles: a = -Xh), as resect_waccumulate forms it
//   H = sum J_w^T J_w (the Schur complement of the full Gauss-Newton matrix),   g = sum J_w^T u,   cost = 1/2 sum chi2
//
// By the Woodbury identity no Sigma^-1 is formed: a singular Sigma is fine.  g is the exact gradient of the reduced cost
// (dF/dX = 0 at Xh).  At the solution, with Sigma_c = H^-1 the pose covariance and G = T J_w (3 x 6):
//
//   X+ = Xh,   Sigma+ = Sigma_cond + G Sigma_c G^T = Sigma_cond + T (J_w Sigma_c J_w^T) T^T      six entries: symmetric by construction
//
// Cov(X_j, pose) = G Sigma_c is not stored.  The frozen noise is one double per observation: s_j^2 for an observation that takes
// part, -s_j^2 (the sign bit set, -0.0 included) for one that is BEHIND at the freeze, NaN for one that is SKIPPED there; neither
// of the two takes part in the solve.  An observation GATED at the solution did take part.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "sba_landmarks.hpp"

#if defined(__clang__)
#pragma STDC FP_CONTRACT OFF
#endif

namespace sba {

// The class landmark_register_noise gives an observation that takes part in the solve.
enum { LANDMARK_LIVE = LANDMARK_FUSED };

// The wave-uniform state of a pass, a by-value kernel argument (scalar registers).
struct LandmarkRegisterParams {
  double Rn[9];              // -R(w)
  double t[3];
  double J[9];               // frame of the rotation Jacobian A = -[a]x J (factored_frame)
  double cov[21];            // Sigma_c, upper triangle row by row over [rot | tran]: the write-back only
  double bearing_sigma2;
  double chi2_gate;
  unsigned long long n;      // landmarks on the handle
  unsigned long long m;      // observations of the pass
  int small_angle;           // rot . rot <= DBL_EPSILON: a = -X, J = I
  int pad_;
};

// The state of a pass at the pose; pose_cov: Sigma_c (36, row-major, symmetric) or null (zeros).
inline void landmark_register_fill(unsigned long long n, unsigned long long m, const double rot[3], const double tran[3],
                                   const double* pose_cov, double bearing_sigma, double chi2_gate, LandmarkRegisterParams* P) {
  double R[9], B[9];
  rotation_and_derivatives(rot, R, nullptr);
  factored_frame(rot, B, P->J);
  for (int i = 0; i < 9; ++i) P->Rn[i] = -R[i];
  for (int i = 0; i < 3; ++i) P->t[i] = tran[i];
  int k = 0;
  for (int a = 0; a < 6; ++a)
    for (int b = a; b < 6; ++b) P->cov[k++] = pose_cov ? pose_cov[6 * a + b] : 0.0;
  P->bearing_sigma2 = bearing_sigma * bearing_sigma;
  P->chi2_gate = chi2_gate;
  P->n = n;
  P->m = m;
  P->small_angle = !(rot[0] * rot[0] + rot[1] * rot[1] + rot[2] * rot[2] > DBL_EPSILON) ? 1 : 0;
  P->pad_ = 0;
}

// Option check of the entry points: the joint solve has no robust loss (SBA_ERR_UNSUPPORTED).
inline const char* landmark_register_check_loss(double huber_delta) {
  return huber_delta == 0.0 ? nullptr : "the joint registration has no robust loss: lm.huber_delta must be 0";
}

// What the three per-observation functions share at a pose, in the arithmetic order of landmark_fuse_one.
struct LandmarkRegisterPoint {
  double rx[3], dstar, yy, W[2][3], u0, u1, s, Tm[3][2];
  bool ok;                   // a finite d* and a factor that did not fail (else W = 0, u = 0, T = 0)
};

// *noise2: the frozen s_j^2 (>= 0, finite); derive == true forms it from d* at this pose instead and returns it (the freeze).
SBA_HD inline void landmark_register_point(const LandmarkRegisterParams& P, const double X[3], const double Sg[6], const double y[3], bool derive,
                                           double* noise2, LandmarkRegisterPoint* o) {
  // c, d*, r exactly as resect_residual: (Rn X) + t summed left to right, r = fma(d*, y, c)
  double c[3], r[3];
  for (int k = 0; k < 3; ++k) {
    o->rx[k] = P.Rn[3 * k] * X[0] + P.Rn[3 * k + 1] * X[1] + P.Rn[3 * k + 2] * X[2];
    c[k] = o->rx[k] + P.t[k];
  }
  const double yy = y[0] * y[0] + y[1] * y[1] + y[2] * y[2];
  const double inv_yy = 1.0 / yy;
  const double dstar = -(y[0] * c[0] + y[1] * c[1] + y[2] * c[2]) * inv_yy;
  for (int k = 0; k < 3; ++k) r[k] = __builtin_fma(dstar, y[k], c[k]);
  o->dstar = dstar;
  o->yy = yy;
  // S = Rn Sigma Rn^T (Rn = -R: the signs cancel) + iso I
  double T1[3][3];
  for (int a = 0; a < 3; ++a) {
    T1[a][0] = P.Rn[3 * a] * Sg[0] + P.Rn[3 * a + 1] * Sg[3] + P.Rn[3 * a + 2] * Sg[4];
    T1[a][1] = P.Rn[3 * a] * Sg[3] + P.Rn[3 * a + 1] * Sg[1] + P.Rn[3 * a + 2] * Sg[5];
    T1[a][2] = P.Rn[3 * a] * Sg[4] + P.Rn[3 * a + 1] * Sg[5] + P.Rn[3 * a + 2] * Sg[2];
  }
  if (derive) *noise2 = P.bearing_sigma2 * (dstar * dstar) * yy;
  const double iso = *noise2;
  double S[6];
  S[0] = T1[0][0] * P.Rn[0] + T1[0][1] * P.Rn[1] + T1[0][2] * P.Rn[2] + iso;
  S[1] = T1[1][0] * P.Rn[3] + T1[1][1] * P.Rn[4] + T1[1][2] * P.Rn[5] + iso;
  S[2] = T1[2][0] * P.Rn[6] + T1[2][1] * P.Rn[7] + T1[2][2] * P.Rn[8] + iso;
  S[3] = T1[0][0] * P.Rn[3] + T1[0][1] * P.Rn[4] + T1[0][2] * P.Rn[5];
  S[4] = T1[0][0] * P.Rn[6] + T1[0][1] * P.Rn[7] + T1[0][2] * P.Rn[8];
  S[5] = T1[1][0] * P.Rn[6] + T1[1][1] * P.Rn[7] + T1[1][2] * P.Rn[8];
  double b1[3], b2[3], q[3];
  resect_weight_basis(y, b1, b2);
  o->ok = resect_weight_factor(S, b1, b2, q) && std::isfinite(dstar);
  if (!o->ok) { q[0] = 0.0; q[1] = 0.0; q[2] = 0.0; }
  resect_weight_whiten(q, b1, b2, o->W);
  o->u0 = o->W[0][0] * r[0] + o->W[0][1] * r[1] + o->W[0][2] * r[2];
  o->u1 = o->W[1][0] * r[0] + o->W[1][1] * r[1] + o->W[1][2] * r[2];
  o->s = o->u0 * o->u0 + o->u1 * o->u1;
  // T = Sigma R^T W^T: column k = Sigma v_k with v_k = R^T W_k^T = -(Rn^T W_k^T)
  for (int k = 0; k < 2; ++k) {
    const double v0 = -(P.Rn[0] * o->W[k][0] + P.Rn[3] * o->W[k][1] + P.Rn[6] * o->W[k][2]),
                 v1 = -(P.Rn[1] * o->W[k][0] + P.Rn[4] * o->W[k][1] + P.Rn[7] * o->W[k][2]),
                 v2 = -(P.Rn[2] * o->W[k][0] + P.Rn[5] * o->W[k][1] + P.Rn[8] * o->W[k][2]);
    o->Tm[0][k] = Sg[0] * v0 + Sg[3] * v1 + Sg[4] * v2;
    o->Tm[1][k] = Sg[3] * v0 + Sg[1] * v1 + Sg[5] * v2;
    o->Tm[2][k] = Sg[4] * v0 + Sg[5] * v1 + Sg[2] * v2;
  }
}

// J_w = W [A(Xh) | I] with Xh = X + T u: a = Rn Xh (small angles: -Xh), A column j = J[:, j] x a as resect_waccumulate forms it.
SBA_HD inline void landmark_register_jacobian(const LandmarkRegisterParams& P, const double X[3], const LandmarkRegisterPoint& pt, double Xh[3],
                                              double Jw[2][6]) {
  for (int k = 0; k < 3; ++k) Xh[k] = X[k] + (pt.Tm[k][0] * pt.u0 + pt.Tm[k][1] * pt.u1);
  double a[3];
  for (int k = 0; k < 3; ++k) a[k] = P.small_angle ? -Xh[k] : P.Rn[3 * k] * Xh[0] + P.Rn[3 * k + 1] * Xh[1] + P.Rn[3 * k + 2] * Xh[2];
  for (int j = 0; j < 3; ++j) {
    const double j0 = P.J[j], j1 = P.J[3 + j], j2 = P.J[6 + j];
    const double A0 = j1 * a[2] - j2 * a[1], A1 = j2 * a[0] - j0 * a[2], A2 = j0 * a[1] - j1 * a[0];
    Jw[0][j] = pt.W[0][0] * A0 + pt.W[0][1] * A1 + pt.W[0][2] * A2;
    Jw[1][j] = pt.W[1][0] * A0 + pt.W[1][1] * A1 + pt.W[1][2] * A2;
    Jw[0][3 + j] = pt.W[0][j];
    Jw[1][3 + j] = pt.W[1][j];
  }
}

// The freeze of one observation at the start pose P: *noise = s_j^2 (LANDMARK_LIVE), -s_j^2 with the sign bit set
// (LANDMARK_BEHIND: d* <= 0) or NaN (LANDMARK_SKIPPED: a non-finite X or Sigma, a zero or non-finite bearing, a non-finite d* or
// s_j^2, a factor that fails).  Returns the class.
SBA_HD inline int landmark_register_noise(const LandmarkRegisterParams& P, const double X[3], const double Sg[6], const double y[3], double* noise) {
  bool ok = std::isfinite(X[0]) && std::isfinite(X[1]) && std::isfinite(X[2]);
  for (int k = 0; k < 6; ++k) ok = ok && std::isfinite(Sg[k]);
  LandmarkRegisterPoint pt;
  double s2 = 0.0;
  landmark_register_point(P, X, Sg, y, true, &s2, &pt);
  ok = ok && pt.ok && std::isfinite(s2);
  if (!ok) { *noise = NAN; return LANDMARK_SKIPPED; }
  if (pt.dstar <= 0.0) { *noise = -s2; return LANDMARK_BEHIND; }
  *noise = s2;
  return LANDMARK_LIVE;
}

// Whether a frozen noise value marks an observation that takes part in the solve.
SBA_HD inline bool landmark_register_live(double noise) { return !std::isnan(noise) && !std::signbit(noise); }

// One observation into the SBA_RESECT_COUNT lane sums, in the slots of SBA_RESECT_*: H, g, cost; SBA_RESECT_SW counts the
// observations that entered (n_used), SBA_RESECT_NBEHIND those of them with d* <= 0 at this pose; SBA_RESECT_NOUT stays 0.
// live = in range and landmark_register_live(noise); an observation that is not live is replaced by the padding one here
// (X = 0, Sigma = 0, y = (1, 0, 0), noise 0: its factor fails and it adds exact zeros), so everything stays finite.  A live
// observation whose factor fails at this pose adds zeros as well.
SBA_HD inline void landmark_register_accumulate(const LandmarkRegisterParams& P, const double X_in[3], const double Sg_in[6], const double y_in[3],
                                                double noise, bool live, double* acc) {
  double X[3], Sg[6], y[3];
  for (int k = 0; k < 3; ++k) { X[k] = live ? X_in[k] : 0.0; y[k] = live ? y_in[k] : (k == 0 ? 1.0 : 0.0); }
  for (int k = 0; k < 6; ++k) Sg[k] = live ? Sg_in[k] : 0.0;
  double s2 = live ? noise : 0.0;
  LandmarkRegisterPoint pt;
  landmark_register_point(P, X, Sg, y, false, &s2, &pt);
  const bool used = live && pt.ok;
  double Xh[3], Jw[2][6];
  landmark_register_jacobian(P, X, pt, Xh, Jw);
  int k = SBA_RESECT_H;
  for (int a = 0; a < 6; ++a) {
    for (int b = a; b < 6; ++b) {
      acc[k] = __builtin_fma(Jw[0][a], Jw[0][b], __builtin_fma(Jw[1][a], Jw[1][b], acc[k]));
      ++k;
    }
    acc[SBA_RESECT_G + a] = __builtin_fma(pt.u0, Jw[0][a], __builtin_fma(pt.u1, Jw[1][a], acc[SBA_RESECT_G + a]));
  }
  acc[SBA_RESECT_COST] = __builtin_fma(0.5, pt.s, acc[SBA_RESECT_COST]);
  acc[SBA_RESECT_SW] += used ? 1.0 : 0.0;
  acc[SBA_RESECT_NBEHIND] += (used && pt.dstar <= 0.0) ? 1.0 : 0.0;
}

// The write-back of one observation at the solution P (P.cov = Sigma_c): the class, tested in the order SKIPPED (marked so at
// the freeze, a factor that fails here, a non-finite d*, X+ or Sigma+; *chi2 = NaN), BEHIND (marked so at the freeze, or d* <= 0
// here), GATED (chi2 > chi2_gate), FUSED.  *chi2 is the observation's chi^2 at the solution otherwise; Xo, So hold the posterior
// for LANDMARK_FUSED and are unspecified otherwise (the caller stores them for LANDMARK_FUSED only).
SBA_HD inline int landmark_register_one(const LandmarkRegisterParams& P, const double X_in[3], const double Sg_in[6], const double y_in[3],
                                        double noise, double Xo[3], double So[6], double* chi2) {
  const bool marked = std::isnan(noise);
  double X[3], Sg[6], y[3];
  for (int k = 0; k < 3; ++k) { X[k] = marked ? 0.0 : X_in[k]; y[k] = marked ? (k == 0 ? 1.0 : 0.0) : y_in[k]; }
  for (int k = 0; k < 6; ++k) Sg[k] = marked ? 0.0 : Sg_in[k];
  double s2 = marked ? 0.0 : std::fabs(noise);
  LandmarkRegisterPoint pt;
  landmark_register_point(P, X, Sg, y, false, &s2, &pt);
  bool ok = !marked && pt.ok;
  double Jw[2][6];
  landmark_register_jacobian(P, X, pt, Xo, Jw);
  // Q = J_w Sigma_c J_w^T (2 x 2, symmetric): V_k = Sigma_c J_w[k]^T first
  double V[2][6];
  for (int a = 0; a < 6; ++a) {
    double v0 = 0.0, v1 = 0.0;
    for (int b = 0; b < 6; ++b) {
      const int lo = a < b ? a : b, hi = a < b ? b : a;
      const double cab = P.cov[6 * lo - lo * (lo - 1) / 2 + (hi - lo)];
      v0 += cab * Jw[0][b];
      v1 += cab * Jw[1][b];
    }
    V[0][a] = v0; V[1][a] = v1;
  }
  double q00 = 0.0, q01 = 0.0, q11 = 0.0;
  for (int a = 0; a < 6; ++a) { q00 += Jw[0][a] * V[0][a]; q01 += Jw[0][a] * V[1][a]; q11 += Jw[1][a] * V[1][a]; }
  // Sigma+ = (Sigma - T T^T) + T Q T^T with TQ = T Q (3 x 2)
  double TQ[3][2];
  for (int k = 0; k < 3; ++k) {
    TQ[k][0] = pt.Tm[k][0] * q00 + pt.Tm[k][1] * q01;
    TQ[k][1] = pt.Tm[k][0] * q01 + pt.Tm[k][1] * q11;
  }
  const int ra[6] = {0, 1, 2, 0, 0, 1}, rb[6] = {0, 1, 2, 1, 2, 2};
  for (int k = 0; k < 6; ++k) {
    const int a = ra[k], b = rb[k];
    So[k] = (Sg[k] - (pt.Tm[a][0] * pt.Tm[b][0] + pt.Tm[a][1] * pt.Tm[b][1])) + (TQ[a][0] * pt.Tm[b][0] + TQ[a][1] * pt.Tm[b][1]);
  }
  for (int k = 0; k < 3; ++k) ok = ok && std::isfinite(Xo[k]);
  for (int k = 0; k < 6; ++k) ok = ok && std::isfinite(So[k]);
  *chi2 = ok ? pt.s : NAN;
  if (!ok) return LANDMARK_SKIPPED;
  if (std::signbit(noise) || pt.dstar <= 0.0) return LANDMARK_BEHIND;
  if (pt.s > P.chi2_gate) return LANDMARK_GATED;
  return LANDMARK_FUSED;
}

}  // namespace sba

#if defined(__clang__)
#pragma STDC FP_CONTRACT DEFAULT
#endif
