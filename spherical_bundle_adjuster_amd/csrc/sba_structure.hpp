// Triangulated landmarks of the joint solve with their 3 x 3 covariances -- the per-match arithmetic structure_kernel
// (sba_structure.hip) runs, with no HIP in it.  The same source is driven on the CPU by tests/test_structure_host_cpu.py.
//
// In camera 2's frame, the frame the residual is written in, with u = R(w) x1:
//   a = d1 u - t,  b = d2 x2,  e = b - a,  X = (a + b) / 2            the landmark: midpoint of the two ray ends
//   G_d = dX / d(d1, d2) = [u | x2] / 2,   G_c = dX / d(w, t) = -F / 2   (F = [A | I] of sba_joint_core.hpp)
// Over (d_i, w, t) the covariance of sba_covariance.hpp has the blocks Sigma_dd,i, Sigma_c and Sigma_dc,i = -s_i T_i Sigma_c, so
//   Sigma_X = G_d s U^-1 s G_d^T + K Sigma_c K^T,   K = G_c - G_d s T   (3 x 6)
// -- two positive semi-definite terms, no difference of large ones.  The score q = trace(Sigma_X) / (X.X) has no dimension: it
// does not depend on the scale of the gauge.  Unscaled, as the blocks it is made of.
#pragma once
#include <cmath>

#include "sba_covariance.hpp"

#if defined(__clang__)
#pragma STDC FP_CONTRACT OFF
#endif

namespace sba {

// One match.  ok: cov_block()'s verdict (false: z1, z2, Ui are not read).  nu = -u, A, s1, s2: joint_block()'s outputs; z1, z2,
// Ui: cov_block()'s; C: Sigma_c, row-major 6 x 6; x2 (unit vector), d1, d2: the match; t: the translation.
// X is written as computed either way.  cov = (xx, yy, zz, xy, xz, yz) and q; a degenerate match gets (inf, inf, inf, 0, 0, 0)
// and q = inf.  want_cov = false (a compile-time constant at every call): X alone.
SBA_HD inline void structure_block(bool ok, bool want_cov, const double nu[3], const double A[3][3], double s1, double s2,
                                   const double z1[6], const double z2[6], const double Ui[3], const double* C, double x2x,
                                   double x2y, double x2z, double d1, double d2, const double t[3], double X[3], double cov[6],
                                   double* q) {
  const double x2[3] = {x2x, x2y, x2z};
  SBA_UNROLL
  for (int r = 0; r < 3; ++r) {
    const double a = d1 * -nu[r] - t[r], b = d2 * x2[r];
    X[r] = 0.5 * (a + b);
  }
  if (!want_cov) return;
  cov[0] = __builtin_huge_val(); cov[1] = __builtin_huge_val(); cov[2] = __builtin_huge_val(); cov[3] = 0.0; cov[4] = 0.0; cov[5] = 0.0;
  *q = __builtin_huge_val();
  if (!ok) return;
  double g1[3], g2[3];               // columns of G_d
  SBA_UNROLL
  for (int r = 0; r < 3; ++r) { g1[r] = -0.5 * nu[r]; g2[r] = 0.5 * x2[r]; }
  const double m11 = s1 * Ui[0] * s1, m22 = s2 * Ui[2] * s2, m12 = s1 * Ui[1] * s2;   // s U^-1 s
  double K[3][6];
  SBA_UNROLL
  for (int a = 0; a < 6; ++a) {
    const double t1 = s1 * z1[a], t2 = s2 * z2[a];    // column a of s T
    SBA_UNROLL
    for (int r = 0; r < 3; ++r) {
      const double f = a < 3 ? A[r][a] : (a - 3 == r ? 1.0 : 0.0);
      K[r][a] = -0.5 * f - (g1[r] * t1 + g2[r] * t2);
    }
  }
  double S[3][3];                    // upper triangle of Sigma_X
  SBA_UNROLL
  for (int r = 0; r < 3; ++r) {
    double kc[6];                    // row r of K Sigma_c
    SBA_UNROLL
    for (int b = 0; b < 6; ++b) {
      double s = 0.0;
      SBA_UNROLL
      for (int a = 0; a < 6; ++a) s += K[r][a] * C[6 * a + b];
      kc[b] = s;
    }
    SBA_UNROLL
    for (int c = r; c < 3; ++c) {
      double s = 0.0;
      SBA_UNROLL
      for (int b = 0; b < 6; ++b) s += kc[b] * K[c][b];
      S[r][c] = (g1[r] * g1[c] * m11 + (g1[r] * g2[c] + g2[r] * g1[c]) * m12 + g2[r] * g2[c] * m22) + s;
    }
  }
  cov[0] = S[0][0]; cov[1] = S[1][1]; cov[2] = S[2][2]; cov[3] = S[0][1]; cov[4] = S[0][2]; cov[5] = S[1][2];
  *q = (S[0][0] + S[1][1] + S[2][2]) / (X[0] * X[0] + X[1] * X[1] + X[2] * X[2]);
}

}  // namespace sba

#if defined(__clang__)
#pragma STDC FP_CONTRACT DEFAULT
#endif
