// Host and device share of the joint registration of a frame against the landmark map under a REDESCENDING loss
// (include/sba_hip.h: sba_landmarks_register_hampel, sba_landmarks_eval_register_hampel and their _device twins).  HIP-free; the
// kernel is in sba_landmarks_register_hampel.hip, the entry points in sba_landmarks.cpp.  Everything per observation -- the
// point, the Jacobian, the freeze, the write-back -- is sba_landmarks_register.hpp's, and the objective's form is
// sba_landmarks_register_robust.hpp's, both included and not copied:
//
//   F_rho = sum_j rho( min_X f_j(X, pose) ) = sum_j rho(chi2_j)        rho monotone: eliminating the landmark is still exact
//
// THE LOSS is Hampel's three-part one on s = chi2_j, r = sqrt(s), 0 < a < b < c:
//   s <= a^2          w = 1                           rho = s
//   a^2 < s <= b^2    w = a / r                       rho = 2 a r - a^2
//   b^2 < s <= c^2    w = a (c - r) / ((c - b) r)     rho = a (b + c) - a^2 - a (c - r)^2 / (c - b)
//   s > c^2           w = 0                           rho = a (b + c) - a^2
// with w = rho'(s); rho is C1.  (The third row's constant 2 a b - a^2 + a (c - b) is the fourth row's value.)  a = lm.huber_delta.
// b = c = +inf is accepted and IS Huber: the third and the fourth row are then never selected, and their arithmetic (inf - inf)
// reaches no sum, because every row is chosen by SELECTION, not by multiplication.
// Per evaluation, as in the robust pass: H = sum w J_w^T J_w (Gauss-Newton without the second-order loss term), g = sum w J_w^T u
// (the exact gradient of 1/2 F_rho), cost = 1/2 sum rho.  The row has SBA_HAMPEL_COUNT = 32 slots: the 31 of SBA_RESECT_* with
//   SBA_RESECT_SW: n_used;  SBA_RESECT_NOUT: n_outlier, the used observations with s > a^2;  SBA_RESECT_NBEHIND: as today;
//   SBA_HAMPEL_NREJ: n_rejected, the used observations with s > c^2 (weight exactly 0)
// THE WRITE-BACK is the robust one: Sigma_c = H_rho^-1, classes by chi2_gate, and chi2_gate > a^2 is refused.  Hampel's weight is
// exactly 1 up to a, so with chi2_gate <= a^2 every fused observation had weight 1 and its posterior is the weighted problem's own.
#pragma once
#include "sba_landmarks_register_robust.hpp"

#if defined(__clang__)
#pragma STDC FP_CONTRACT OFF
#endif

namespace sba {

enum {
  SBA_HAMPEL_NREJ = SBA_RESECT_COUNT,      // slot 31: used observations beyond c
  SBA_HAMPEL_COUNT = SBA_RESECT_COUNT + 1
};
static_assert(int(SBA_HAMPEL_COUNT) <= int(SBA_RESECT_SIZE), "the row of the Hampel pass fits the resection row's allocation");

// The loss of a pass, a by-value kernel argument beside LandmarkRegisterParams (scalar registers).  Everything derived is rounded
// once, on the host.
struct LandmarkRegisterHampel {
  double a, c;               // lm.huber_delta and the rejection point
  double a2, b2, c2;         // the squares
  double inv_cb;             // 1 / (c - b); NaN for b = c = +inf, where no observation selects it
  double rho_max;            // a (b + c) - a^2, rho beyond c
};

inline void landmark_register_hampel_fill(double a, double b, double c, LandmarkRegisterHampel* L) {
  L->a = a;
  L->c = c;
  L->a2 = a * a;
  L->b2 = b * b;
  L->c2 = c * c;
  L->inv_cb = 1.0 / (c - b);
  L->rho_max = a * (b + c) - a * a;
}

// Option check of the Hampel entry points (SBA_ERR_INVALID_ARG): nullptr = fine.  First the robust check (a finite a > 0,
// chi2_gate <= a^2), then the thresholds: finite with a < b < c, or both +inf (Huber).
inline const char* landmark_register_check_hampel(double a, double b, double c, double chi2_gate) {
  if (const char* why = landmark_register_check_robust(a, chi2_gate)) return why;
  if (std::isnan(b) || std::isnan(c)) return "the Hampel thresholds b and c must not be NaN";
  if (std::isinf(b) != std::isinf(c)) return "the Hampel thresholds b and c must both be finite or both +inf";
  if (!(b > a)) return "the Hampel threshold b must exceed a = lm.huber_delta";
  if (std::isinf(b)) return c > 0.0 ? nullptr : "the Hampel threshold c must exceed b";     // both +inf: Huber
  if (!(c > b)) return "the Hampel threshold c must exceed b";
  return nullptr;
}

// w = rho'(s), rho(s), is_out (s > a^2), is_rej (s > c^2).  1 / sqrt(s) as landmark_register_huber takes it: on the device
// (under SBA_LANDMARK_REGISTER_DEVICE_HUBER) the reciprocal square root refined by two Newton steps of huber in
// sba_sweep_core.hpp, on the host 1 / sqrt.  The comparisons are the same expressions in both, so the counts are identical.
// The second row is huber's own expressions, so that with b = c = +inf the pass is the robust one's arithmetic.  No branch:
// four candidates, three selects each.
SBA_HD inline void landmark_register_hampel(double s, const LandmarkRegisterHampel& L, double& w, double& rho, double& is_out, double& is_rej) {
#if defined(__HIP_DEVICE_COMPILE__) && defined(SBA_LANDMARK_REGISTER_DEVICE_HUBER)
  double y = __builtin_amdgcn_rsq(s);
  const double hs = 0.5 * s;
  y = y * __builtin_fma(-hs * y, y, 1.5);
  y = y * __builtin_fma(-hs * y, y, 1.5);
#else
  const double y = 1.0 / std::sqrt(s);
#endif
  const bool out = s > L.a2, mid = s > L.b2, rej = s > L.c2;
  const double r = s * y;                                   // sqrt(s)
  const double t = L.c - r;
  const double q = (L.a * t) * L.inv_cb;                    // a (c - r) / (c - b)
  const double w2 = L.a * y, rho2 = __builtin_fma(2.0 * L.a, r, -L.a2);
  const double w3 = q * y, rho3 = __builtin_fma(-q, t, L.rho_max);
  w = rej ? 0.0 : (mid ? w3 : (out ? w2 : 1.0));
  rho = rej ? L.rho_max : (mid ? rho3 : (out ? rho2 : s));
  is_out = out ? 1.0 : 0.0;
  is_rej = rej ? 1.0 : 0.0;
}

// One observation into the SBA_HAMPEL_COUNT lane sums, in landmark_register_accumulate_robust's order exactly: w J_w[k][a] first,
// then the same fma chain.  An observation that is not used gets w = 0, rho = 0 and zero counts by SELECTION (the padding
// observation has s = 0, whose reciprocal square root is not finite).
SBA_HD inline void landmark_register_accumulate_hampel(const LandmarkRegisterParams& P, const LandmarkRegisterHampel& L, const double X_in[3],
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
  double w, rho, is_out, is_rej;
  landmark_register_hampel(pt.s, L, w, rho, is_out, is_rej);
  if (!used) { w = 0.0; rho = 0.0; is_out = 0.0; is_rej = 0.0; }
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
  acc[SBA_HAMPEL_NREJ] += is_rej;
}

}  // namespace sba

#if defined(__clang__)
#pragma STDC FP_CONTRACT DEFAULT
#endif
