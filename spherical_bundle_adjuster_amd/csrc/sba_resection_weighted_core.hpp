// Device core of the covariance-weighted resection (included by .hip files only): the per-match arithmetic of its passes on
// top of sba_resection_core.hpp's loads, match and residual.  Algebra: sba_resection_weighted.hpp, whose basis, factor and M
// row are the very functions used here.
#pragma once
#include "sba_resection_core.hpp"
#include "sba_resection_weighted.hpp"

namespace sba {
namespace {

// One 16-byte vector (two matches) or two (four, f32 planes) of each of the three weight planes.
template <typename ST>
struct ResectWeightRegs {
  static constexpr int PPT = Lanes<ST>::PPT;
  double2 q[3][PPT / 2];
  __device__ __forceinline__ void load(const ResectWeightPlanes& wp, size_t p) {
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int h = 0; h < PPT / 2; ++h)
        q[k][h] = VecRegs<ST, DEPTH_PER_MATCH>::stream_load(reinterpret_cast<const double2*>(wp.q[k]) + p * (PPT / 2) + h);
  }
  __device__ __forceinline__ double get(int k, int h) const { return (h & 1) ? q[k][h >> 1].y : q[k][h >> 1].x; }
};

// The factored weight of one match at the reference pose W.P: q = 0 and false for a match of zero weight (and for padding).
// sg: the match's Sigma row (xx, yy, zz, xy, xz, yz).
__device__ __forceinline__ bool resect_weight_freeze(const ResectWeightParams& W, const ResectMatch& m, const double sg[6], bool valid,
                                                     double q[3]) {
  double inv_yy, dstar, c[3], r[3];
  resect_residual(W.P, m, inv_yy, dstar, c, r);
  bool ok = valid && std::isfinite(dstar);
#pragma unroll
  for (int k = 0; k < 6; ++k) ok = ok && std::isfinite(sg[k]);
  // T = Rn Sigma, S = cov_scale T Rn^T + iso I   (Rn = -R: the signs cancel)
  const double* Rn = W.P.Rn;
  double T[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    T[a][0] = Rn[3 * a] * sg[0] + Rn[3 * a + 1] * sg[3] + Rn[3 * a + 2] * sg[4];
    T[a][1] = Rn[3 * a] * sg[3] + Rn[3 * a + 1] * sg[1] + Rn[3 * a + 2] * sg[5];
    T[a][2] = Rn[3 * a] * sg[4] + Rn[3 * a + 1] * sg[5] + Rn[3 * a + 2] * sg[2];
  }
  const double yy = m.y[0] * m.y[0] + m.y[1] * m.y[1] + m.y[2] * m.y[2];
  const double iso = W.bearing_sigma2 * (dstar * dstar) * yy;
  double S[6];
  S[0] = __builtin_fma(W.cov_scale, T[0][0] * Rn[0] + T[0][1] * Rn[1] + T[0][2] * Rn[2], iso);
  S[1] = __builtin_fma(W.cov_scale, T[1][0] * Rn[3] + T[1][1] * Rn[4] + T[1][2] * Rn[5], iso);
  S[2] = __builtin_fma(W.cov_scale, T[2][0] * Rn[6] + T[2][1] * Rn[7] + T[2][2] * Rn[8], iso);
  S[3] = W.cov_scale * (T[0][0] * Rn[3] + T[0][1] * Rn[4] + T[0][2] * Rn[5]);
  S[4] = W.cov_scale * (T[0][0] * Rn[6] + T[0][1] * Rn[7] + T[0][2] * Rn[8]);
  S[5] = W.cov_scale * (T[1][0] * Rn[6] + T[1][1] * Rn[7] + T[1][2] * Rn[8]);
  double b1[3], b2[3];
  resect_weight_basis(m.y, b1, b2);
  ok = resect_weight_factor(S, b1, b2, q) && ok;
  if (!ok) { q[0] = 0.0; q[1] = 0.0; q[2] = 0.0; }
  return ok;
}

// One match into the SBA_RESECT_COUNT lane sums.  live = in range and of non-zero weight; the caller has replaced a match
// that is not live by the padding match (resect_match with valid = false), so everything here stays finite.
template <bool LOSS>
__device__ __forceinline__ void resect_waccumulate(const ResectParams& P, const ResectMatch& m, const double q[3], bool live,
                                                   double* __restrict__ acc) {
  double inv_yy, dstar, c[3], r[3];
  resect_residual(P, m, inv_yy, dstar, c, r);
  double b1[3], b2[3], W[2][3];
  resect_weight_basis(m.y, b1, b2);
  resect_weight_whiten(q, b1, b2, W);
  // z = W r, s = z . z
  const double z0 = W[0][0] * r[0] + W[0][1] * r[1] + W[0][2] * r[2], z1 = W[1][0] * r[0] + W[1][1] * r[1] + W[1][2] * r[2];
  const double s = z0 * z0 + z1 * z1;
  double w = 1.0, rho = s, is_out = 0.0;
  if (LOSS) huber(s, P.delta, P.delta2, w, rho, is_out);
  double behind = dstar <= 0.0 ? 1.0 : 0.0;
  if (!live) { w = 0.0; rho = 0.0; is_out = 0.0; behind = 0.0; }
  // J_z = [W A | W], A column j = J[:, j] x a as in resect_accumulate; no P: W y = 0
  const double a0 = P.small_angle ? -m.X[0] : c[0] - P.t[0], a1 = P.small_angle ? -m.X[1] : c[1] - P.t[1],
               a2 = P.small_angle ? -m.X[2] : c[2] - P.t[2];
  double Jz[2][6];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double j0 = P.J[j], j1 = P.J[3 + j], j2 = P.J[6 + j];
    const double A0 = j1 * a2 - j2 * a1, A1 = j2 * a0 - j0 * a2, A2 = j0 * a1 - j1 * a0;
    Jz[0][j] = W[0][0] * A0 + W[0][1] * A1 + W[0][2] * A2;
    Jz[1][j] = W[1][0] * A0 + W[1][1] * A1 + W[1][2] * A2;
    Jz[0][3 + j] = W[0][j];
    Jz[1][3 + j] = W[1][j];
  }
  const double wz0 = w * z0, wz1 = w * z1;
  int k = SBA_RESECT_H;
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    const double u0 = w * Jz[0][a], u1 = w * Jz[1][a];
#pragma unroll
    for (int b = a; b < 6; ++b) {
      acc[k] = __builtin_fma(u0, Jz[0][b], __builtin_fma(u1, Jz[1][b], acc[k]));
      ++k;
    }
    acc[SBA_RESECT_G + a] = __builtin_fma(wz0, Jz[0][a], __builtin_fma(wz1, Jz[1][a], acc[SBA_RESECT_G + a]));
  }
  acc[SBA_RESECT_COST] = __builtin_fma(0.5, rho, acc[SBA_RESECT_COST]);
  acc[SBA_RESECT_SW] += w;
  acc[SBA_RESECT_NOUT] += is_out;
  acc[SBA_RESECT_NBEHIND] += behind;
}

}  // namespace
}  // namespace sba
