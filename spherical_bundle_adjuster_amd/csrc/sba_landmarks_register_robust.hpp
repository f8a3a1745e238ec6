// Host and device share of the ROBUST joint registration of a frame against the landmark map (include/sba_hip.h:
// sba_landmarks_register_robust, sba_landmarks_eval_register_robust and their _device twins).  HIP-free; the kernel is in
// sba_landmarks_register_robust.hip, the entry points in sba_landmarks.cpp.  Everything per observation -- the point, the
// Jacobian, the freeze, the write-back -- is sba_landmarks_register.hpp's, included and not copied.  THE OBJECTIVE, with f_j the
// block of landmark j in that header's F (its bearing term plus its prior term):
//
//   F_rho = sum_j rho( min_X f_j(X, pose) )                  the loss on a residual block, as Ceres applies one
//
// rho is monotone, so the minimisation over X_j passes through it: eliminating the landmark is still exact, Xh_j is unchanged,
// and what remains is F_rho(pose) = sum_j rho(chi2_j) with chi2_j = u . u of sba_landmarks_register.hpp.
//   rho:  the project's Huber (huber of sba_sweep_core.hpp): rho(s) = s for s <= delta^2, else 2 delta sqrt(s) - delta^2
//   w = rho'(s):  1 for s <= delta^2, else delta / sqrt(s);   delta = lm.huber_delta, on the whitened, dimensionless |u|
// Per evaluation:
//   H = sum w_j J_w^T J_w        Gauss-Newton without the second-order loss term, as resect_waccumulate<true> forms it
//   g = sum w_j J_w^T u          the exact gradient of 1/2 F_rho (dF/dX = 0 at Xh)
//   cost = 1/2 sum rho(chi2_j)
//   SBA_RESECT_SW: n_used, as today;  SBA_RESECT_NOUT: n_outlier, the used observations with s > delta^2;  SBA_RESECT_NBEHIND: as
//   today.  The row stays at the 31 slots of SBA_RESECT_*: there is no sum of the weights.
// THE WRITE-BACK: Sigma_c = H_rho^-1 at the solution, then sba_landmarks_register.hpp's freeze and landmark_register_one
// unchanged, with classes by chi2_gate.  chi2_gate > delta^2 is REFUSED: an observation the loss downweights has w < 1 and its
// block's conditional covariance would be Sigma_cond / w, which inflates the landmark.  With chi2_gate <= delta^2 every fused
// observation had weight exactly 1 and its posterior X+ = Xh, Sigma+ = Sigma_cond + G Sigma_c G^T is the weighted problem's own;
// every downweighted observation is gated and its landmark stays untouched, byte for byte.
#pragma once
#include "sba_landmarks_register.hpp"

#if defined(__clang__)
#pragma STDC FP_CONTRACT OFF
#endif

namespace sba {

// The loss of a pass, a by-value kernel argument beside LandmarkRegisterParams (scalar registers).
struct LandmarkRegisterRobust {
  double delta;              // lm.huber_delta
  double delta2;             // delta * delta, rounded once on the host
};

inline void landmark_register_robust_fill(double huber_delta, LandmarkRegisterRobust* L) {
  L->delta = huber_delta;
  L->delta2 = huber_delta * huber_delta;
}

// Option check of the robust entry points (SBA_ERR_INVALID_ARG): nullptr = fine.  chi2_gate itself is checked by
// landmark_check_gate; here against delta^2, where +inf and NaN count as larger.
inline const char* landmark_register_check_robust(double huber_delta, double chi2_gate) {
  if (!(std::isfinite(huber_delta) && huber_delta > 0.0)) return "the robust registration needs a finite lm.huber_delta > 0";
  if (!(chi2_gate <= huber_delta * huber_delta))
    return "chi2_gate must not exceed lm.huber_delta^2: a downweighted observation must be gated, not fused";
  return nullptr;
}

// w = rho'(s), rho(s), is_out.  The device pass is huber of sba_sweep_core.hpp (a reciprocal square root refined by two
// Newton steps), which the kernel's file includes and names by SBA_LANDMARK_REGISTER_DEVICE_HUBER; the host pass (the g++
// harness) is 1 / sqrt.  The comparison s > delta2 is the same expression in both, so n_outlier is identical.
SBA_HD inline void landmark_register_huber(double s, double delta, double delta2, double& w, double& rho, double& is_out) {
#if defined(__HIP_DEVICE_COMPILE__) && defined(SBA_LANDMARK_REGISTER_DEVICE_HUBER)
  huber(s, delta, delta2, w, rho, is_out);
#else
  const double y = 1.0 / std::sqrt(s);
  const bool out = s > delta2;
  w = out ? delta * y : 1.0;
  rho = out ? __builtin_fma(2.0 * delta, s * y, -delta2) : s;
  is_out = out ? 1.0 : 0.0;
#endif
}

// One observation into the SBA_RESECT_COUNT lane sums, in the order of landmark_register_accumulate with w applied as
// resect_waccumulate applies it: w J_w[k][a] first, then the same fma chain.  An observation that is not used (not live, or a
// factor that fails at this pose) gets w = 0, rho = 0, is_out = 0 by SELECTION: the padding observation has s = 0, whose
// reciprocal square root is not finite, and a product with it would reach the sums.
SBA_HD inline void landmark_register_accumulate_robust(const LandmarkRegisterParams& P, double delta, double delta2, const double X_in[3],
                                                       const double Sg_in[6], const double y_in[3], double noise, bool live, double* acc) {
  double X[3], Sg[6], y[3];
  for (int k = 0; k < 3; ++k) { X[k] = live ? X_in[k] : 0.0; y[k] = live ? y_in[k] : (k == 0 ? 1.0 : 0.0); }
  for (int k = 0; k < 6; ++k) Sg[k] = live ? Sg_in[k] : 0.0;
  double s2 = live ? noise : 0.0;
  LandmarkRegisterPoint pt;
  landmark_register_point(P, X, Sg, y, false, &s2, &pt);
  const bool used = live && pt.ok;
  double Xh[3], Jw[2][6];
  landmark_register_jacobian(P, X, pt, Xh, Jw);
  double w, rho, is_out;
  landmark_register_huber(pt.s, delta, delta2, w, rho, is_out);
  if (!used) { w = 0.0; rho = 0.0; is_out = 0.0; }
  const double wu0 = w * pt.u0, wu1 = w * pt.u1;
  int k = SBA_RESECT_H;
  for (int a = 0; a < 6; ++a) {
    const double v0 = w * Jw[0][a], v1 = w * Jw[1][a];
    for (int b = a; b < 6; ++b) {
      acc[k] = __builtin_fma(v0, Jw[0][b], __builtin_fma(v1, Jw[1][b], acc[k]));
      ++k;
    }
    acc[SBA_RESECT_G + a] = __builtin_fma(wu0, Jw[0][a], __builtin_fma(wu1, Jw[1][a], acc[SBA_RESECT_G + a]));
  }
  acc[SBA_RESECT_COST] = __builtin_fma(0.5, rho, acc[SBA_RESECT_COST]);
  acc[SBA_RESECT_SW] += used ? 1.0 : 0.0;
  acc[SBA_RESECT_NOUT] += is_out;
  acc[SBA_RESECT_NBEHIND] += (used && pt.dstar <= 0.0) ? 1.0 : 0.0;
}

}  // namespace sba

#if defined(__clang__)
#pragma STDC FP_CONTRACT DEFAULT
#endif
