// Covariance of the joint solve at a point (rot, tran, d) -- what ceres::Covariance gives a Ceres user -- as two pieces
// with no HIP in them: the per-match 2x2 block arithmetic both kernels of sba_covariance.hip run (cov_block, cov_depth_block)
// and the finish between the two passes (cov_finish: on the host for one problem, on the device for a batch).  The same source is driven on the CPU by
// tests/test_covariance_host_cpu.py with blocks from the dense restatement.
//
// Robustified problem (sqrt(rho')-scaled Jacobian, Ceres' apply_loss_function = true), undamped (radius = inf), depth
// columns Jacobi-scaled by s_i:  H = [U W; W^T V]  with the per-match 2x2 blocks U_i, their 2x6 couplings W_i
// (joint_block() of sba_joint_core.hpp) and S = V - sum W_i^T U_i^-1 W_i.  In the tangent space of the gauge
// (detail::Param's 6 x m projection P: m = 5 with SBA_TRAN_SPHERE, 6 with SBA_TRAN_FREE):
//
//   Sigma_c    = P (P^T S P)^-1 P^T                                            6 x 6 over [rot | tran], rank m
//   Sigma_dd,i = s_i (U_i^-1 + T_i Sigma_c T_i^T) s_i,   T_i = U_i^-1 W_i      the match's own 2x2 block
//
// Degeneracy: det(U) / (U11 U22) = sin^2 of the angle between the rays R x1 and x2 (weight and scaling cancel).  A match
// whose value is <= min_sin2_parallax or not finite, or whose 1 / det is not finite, is left out of the problem.
#pragma once
#include <cfloat>
#include <cmath>

#include "../../include/sba_hip.h"
#include "sba_lm.hpp"

#if defined(__clang__)
#pragma STDC FP_CONTRACT OFF
#endif

namespace sba {

// Row of cov_reduce_kernel: the upper triangle of S over [rot | tran] row by row, then four sums over the used matches.
enum {
  COV_OUT_S = 0,
  COV_OUT_COST = 21,
  COV_OUT_SW = 22,
  COV_OUT_NUSED = 23,
  COV_OUT_NDEG = 24,
  COV_OUT_COUNT = 25,
  COV_ROW = 32            // doubles per block-partial row (256 B: whole 128-byte lines)
};

// Elimination of one match's depth block: T = U^-1 W (rows z1, z2) and U^-1 (i11, i12, i22).  Returns false for a
// degenerate match (nothing else is then defined).  Both kernels call this very function with the same inputs.
SBA_HD inline bool cov_block(double U11, double U12, double U22, double inv_det, const double w1[6], const double w2[6],
                             double min_sin2_parallax, double z1[6], double z2[6], double Ui[3]) {
  const double sin2 = (U11 * U22 - U12 * U12) / (U11 * U22);
  if (!(sin2 > min_sin2_parallax) || !std::isfinite(sin2) || !std::isfinite(inv_det)) return false;
  Ui[0] = U22 * inv_det; Ui[1] = -(U12 * inv_det); Ui[2] = U11 * inv_det;
  SBA_UNROLL
  for (int a = 0; a < 6; ++a) {
    z1[a] = (U22 * w1[a] - U12 * w2[a]) * inv_det;
    z2[a] = (U11 * w2[a] - U12 * w1[a]) * inv_det;
  }
  return true;
}

// out = [var d1, var d2, cov(d1, d2)] of one used match, in unscaled depths; C: Sigma_c, row-major 6 x 6.
SBA_HD inline void cov_depth_block(double s1, double s2, const double Ui[3], const double z1[6], const double z2[6],
                                   const double* C, double out[3]) {
  double q11 = 0.0, q12 = 0.0, q22 = 0.0;
  SBA_UNROLL
  for (int a = 0; a < 6; ++a) {
    double c1 = 0.0, c2 = 0.0;       // (Sigma_c z1)[a], (Sigma_c z2)[a]
    SBA_UNROLL
    for (int b = 0; b < 6; ++b) { c1 += C[6 * a + b] * z1[b]; c2 += C[6 * a + b] * z2[b]; }
    q11 += z1[a] * c1; q12 += z1[a] * c2; q22 += z2[a] * c2;
  }
  out[0] = s1 * (Ui[0] + q11) * s1;
  out[1] = s2 * (Ui[2] + q22) * s2;
  out[2] = s1 * (Ui[1] + q12) * s2;
}

// The arrays of cov_finish: on the host an object on the stack, on the device the block's LDS (the loops below index them
// with run-time bounds, which registers cannot serve).
struct CovFinishWork {
  sba_normal_eq ne;
  detail::Param par;
  double Sf[detail::kDim * detail::kDim], gf[detail::kDim], sc[detail::kDim], A[detail::kDim * detail::kDim];
  double L[detail::kDim * detail::kDim], Li[detail::kDim * detail::kDim], Cf[detail::kDim * detail::kDim], PC[detail::kDim * detail::kDim];
};

// The finish between the two passes: S (upper triangle, row by row, 21 entries) -> Sigma_c (cov, row-major 6 x 6, symmetric to
// the bit) and the dimension m of the gauge's tangent space.  Project with detail::Param, Jacobi-scale to unit diagonal,
// Cholesky, invert, un-scale, lift.  Returns false -- nothing written -- when n_used < m, S is not finite, or a pivot of the
// unit-diagonal system is not above m * DBL_EPSILON (a rank-deficient gauge or scene).  Host and device (thread 0 of
// batch_cov_kernel) run this one text, unfused on either: their results agree to the bit.  wk: need not be initialised.
SBA_HD inline bool cov_finish(const double* S21, int tran_param, const double tran[3], long long n_used, double* cov, int* dim,
                              CovFinishWork* wk) {
  using namespace detail;
  sba_normal_eq& ne = wk->ne;
  for (int a = 0; a < 6; ++a) ne.g[a] = 0.0;
  ne.cost = 0.0; ne.sum_w = 0.0; ne.n_outlier = 0.0;
  int k = 0;
  for (int a = 0; a < 6; ++a)
    for (int b = a; b < 6; ++b) {
      if (!std::isfinite(S21[k])) return false;
      ne.H[6 * a + b] = S21[k];
      ne.H[6 * b + a] = S21[k];
      ++k;
    }
  Param& par = wk->par;
  par.build(SBA_MODE_RT, tran_param, tran);
  const int m = par.m;
  if (n_used < m) return false;
  double *Sf = wk->Sf, *gf = wk->gf, *sc = wk->sc, *A = wk->A;
  par.project(ne, Sf, gf);
  for (int i = 0; i < m; ++i) {
    const double d = Sf[i * kDim + i];
    if (!(d > 0.0) || !std::isfinite(d)) return false;
    sc[i] = 1.0 / std::sqrt(d);
  }
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < m; ++j) A[i * kDim + j] = i == j ? 1.0 : sc[i] * Sf[(i < j ? i : j) * kDim + (i < j ? j : i)] * sc[j];
  // A = L L^T
  double *L = wk->L, *Li = wk->Li, *Cf = wk->Cf, *PC = wk->PC;
  for (int i = 0; i < kDim * kDim; ++i) { L[i] = 0.0; Li[i] = 0.0; Cf[i] = 0.0; PC[i] = 0.0; }
  const double floor_pivot = m * DBL_EPSILON;
  for (int i = 0; i < m; ++i)
    for (int j = 0; j <= i; ++j) {
      double s = A[i * kDim + j];
      for (int q = 0; q < j; ++q) s -= L[i * kDim + q] * L[j * kDim + q];
      if (i == j) {
        if (!(s > floor_pivot) || !std::isfinite(s)) return false;
        L[i * kDim + i] = std::sqrt(s);
      } else {
        L[i * kDim + j] = s / L[j * kDim + j];
      }
    }
  // L^-1 (lower), column by column
  for (int c = 0; c < m; ++c)
    for (int i = c; i < m; ++i) {
      double s = i == c ? 1.0 : 0.0;
      for (int q = c; q < i; ++q) s -= L[i * kDim + q] * Li[q * kDim + c];
      Li[i * kDim + c] = s / L[i * kDim + i];
    }
  // A^-1 = L^-T L^-1, un-scaled: upper triangle, mirrored
  for (int i = 0; i < m; ++i)
    for (int j = i; j < m; ++j) {
      double s = 0.0;
      for (int q = j; q < m; ++q) s += Li[q * kDim + i] * Li[q * kDim + j];
      s = sc[i] * s * sc[j];
      if (!std::isfinite(s)) return false;
      Cf[i * kDim + j] = s;
      Cf[j * kDim + i] = s;
    }
  // lift: P Cf P^T
  for (int a = 0; a < 6; ++a)
    for (int j = 0; j < m; ++j) {
      double s = 0.0;
      for (int i = 0; i < m; ++i) s += par.P[a * kDim + i] * Cf[i * kDim + j];
      PC[a * kDim + j] = s;
    }
  for (int a = 0; a < 6; ++a)
    for (int b = a; b < 6; ++b) {
      double s = 0.0;
      for (int j = 0; j < m; ++j) s += PC[a * kDim + j] * par.P[b * kDim + j];
      cov[6 * a + b] = s;
      cov[6 * b + a] = s;
    }
  *dim = m;
  return true;
}

// ... with its arrays on the caller's stack: the host's form.
SBA_HD inline bool cov_finish(const double* S21, int tran_param, const double tran[3], long long n_used, double* cov, int* dim) {
  CovFinishWork wk;
  return cov_finish(S21, tran_param, tran, n_used, cov, dim, &wk);
}

}  // namespace sba

#if defined(__clang__)
#pragma STDC FP_CONTRACT DEFAULT
#endif
