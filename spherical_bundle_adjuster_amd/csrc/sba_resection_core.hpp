// Device core of the spherical resection (included by .hip files only): the per-match arithmetic of its three passes.
// Algebra and row layout: sba_resection.hpp.  What a lane streams: the three x1 planes, the three x2 planes and d1 -- never d2.
#pragma once
#include "sba_device.hpp"
#include "sba_resection.hpp"
#include "sba_sweep_core.hpp"

namespace sba {
namespace {

// One 16-byte vector of every plane a resection pass reads, loaded one grid-stride step ahead of its use (the sweep's
// VecRegs without the d2 plane).
template <typename ST>
struct ResectRegs {
  static constexpr int PPT = Lanes<ST>::PPT;
  typename Lanes<ST>::vec c[6];        // x1.x x1.y x1.z x2.x x2.y x2.z
  double2 d1[PPT / 2];
  __device__ __forceinline__ void load(const Planes& pl, size_t p) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      c[k] = VecRegs<ST, DEPTH_PER_MATCH>::stream_load(reinterpret_cast<const typename Lanes<ST>::vec*>(pl.x1[k]) + p);
      c[3 + k] = VecRegs<ST, DEPTH_PER_MATCH>::stream_load(reinterpret_cast<const typename Lanes<ST>::vec*>(pl.x2[k]) + p);
    }
#pragma unroll
    for (int h = 0; h < PPT / 2; ++h)
      d1[h] = VecRegs<ST, DEPTH_PER_MATCH>::stream_load(reinterpret_cast<const double2*>(pl.d1) + p * (PPT / 2) + h);
  }
  __device__ __forceinline__ double coord(int k, int h) const {
    if (PPT == 2) return h == 0 ? static_cast<double>(c[k].x) : static_cast<double>(c[k].y);
    const float4& q = reinterpret_cast<const float4&>(c[k]);
    return h == 0 ? q.x : (h == 1 ? q.y : (h == 2 ? q.z : q.w));
  }
  __device__ __forceinline__ double depth1(int h) const { return (h & 1) ? d1[h >> 1].y : d1[h >> 1].x; }
};

// The landmark as the sweep forms it (the rounded product) and the bearing.  A padding slot (zeros in the planes) gets the
// bearing (1, 0, 0): everything downstream stays finite and its weight is zero.
struct ResectMatch {
  double X[3], y[3];
};
template <typename ST>
__device__ __forceinline__ void resect_match(const ResectRegs<ST>& r, int h, bool valid, ResectMatch& m) {
  const double d1 = r.depth1(h);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    m.X[k] = mul_rounded(d1, r.coord(k, h));
    m.y[k] = r.coord(3 + k, h);
  }
  if (!valid) { m.X[0] = 0.0; m.X[1] = 0.0; m.X[2] = 0.0; m.y[0] = 1.0; m.y[1] = 0.0; m.y[2] = 0.0; }
}

// c = Rn X + t, d* = -(y . c) / (y . y), r = c + d* y
__device__ __forceinline__ void resect_residual(const ResectParams& P, const ResectMatch& m, double& inv_yy, double& dstar, double c[3], double r[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) c[k] = P.Rn[3 * k] * m.X[0] + P.Rn[3 * k + 1] * m.X[1] + P.Rn[3 * k + 2] * m.X[2] + P.t[k];
  inv_yy = 1.0 / (m.y[0] * m.y[0] + m.y[1] * m.y[1] + m.y[2] * m.y[2]);
  dstar = -(m.y[0] * c[0] + m.y[1] * c[1] + m.y[2] * c[2]) * inv_yy;
#pragma unroll
  for (int k = 0; k < 3; ++k) r[k] = __builtin_fma(dstar, m.y[k], c[k]);
}

// One match into the SBA_RESECT_COUNT lane sums.
template <bool LOSS>
__device__ __forceinline__ void resect_accumulate(const ResectParams& P, const ResectMatch& m, bool valid, double* __restrict__ acc) {
  double inv_yy, dstar, c[3], r[3];
  resect_residual(P, m, inv_yy, dstar, c, r);
  const double s = sq_norm(r[0], r[1], r[2]);
  double w = 1.0, rho = s, is_out = 0.0;
  if (LOSS) huber(s, P.delta, P.delta2, w, rho, is_out);
  double behind = dstar <= 0.0 ? 1.0 : 0.0;
  if (!valid) { w = 0.0; rho = 0.0; is_out = 0.0; behind = 0.0; }
  // A = -[a]x J, column j = J[:, j] x a, with a = -R X = c - t (small angles: a = -X, J = I): the frame of sba_rotation.hpp, as
  // the joint solve's per-match block forms it.  PA = P A = A - y (y . A_j) / (y . y)
  const double a0 = P.small_angle ? -m.X[0] : c[0] - P.t[0], a1 = P.small_angle ? -m.X[1] : c[1] - P.t[1],
               a2 = P.small_angle ? -m.X[2] : c[2] - P.t[2];
  // Column by column, so that only PA stays live: g_a = w A_a . r goes out as soon as column a exists.
  double PA[3][3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double j0 = P.J[j], j1 = P.J[3 + j], j2 = P.J[6 + j];
    const double A0 = j1 * a2 - j2 * a1, A1 = j2 * a0 - j0 * a2, A2 = j0 * a1 - j1 * a0;
    acc[SBA_RESECT_G + j] = __builtin_fma(w, A0 * r[0] + A1 * r[1] + A2 * r[2], acc[SBA_RESECT_G + j]);
    const double ya = (m.y[0] * A0 + m.y[1] * A1 + m.y[2] * A2) * inv_yy;
    PA[0][j] = __builtin_fma(-ya, m.y[0], A0);
    PA[1][j] = __builtin_fma(-ya, m.y[1], A1);
    PA[2][j] = __builtin_fma(-ya, m.y[2], A2);
  }
  // upper triangle of H row by row: rows 0..2 = w [A^T P A | A^T P], rows 3..5 = w P
  int k = SBA_RESECT_H;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int b = a; b < 3; ++b) {
      acc[k] = __builtin_fma(w, PA[0][a] * PA[0][b] + PA[1][a] * PA[1][b] + PA[2][a] * PA[2][b], acc[k]);
      ++k;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) { acc[k] = __builtin_fma(w, PA[c][a], acc[k]); ++k; }
  }
  const double wi = w * inv_yy;
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = a; b < 3; ++b) {
      acc[k] += (a == b ? w : 0.0) - wi * m.y[a] * m.y[b];
      ++k;
    }
  // g_t = w r
#pragma unroll
  for (int a = 0; a < 3; ++a) acc[SBA_RESECT_G + 3 + a] = __builtin_fma(w, r[a], acc[SBA_RESECT_G + 3 + a]);
  acc[SBA_RESECT_COST] = __builtin_fma(0.5, rho, acc[SBA_RESECT_COST]);
  acc[SBA_RESECT_SW] += w;
  acc[SBA_RESECT_NOUT] += is_out;
  acc[SBA_RESECT_NBEHIND] += behind;
}

// One match into the SBA_RESECT_MOM_COUNT lane sums of the DLT: (X~ X~^T)[a][b] Q[c][d], X~ = (X, -1), Q = (y . y) I - y y^T.
__device__ __forceinline__ void resect_moments(const ResectMatch& m, bool valid, double* __restrict__ acc) {
  const double v = valid ? 1.0 : 0.0;
  const double yy = m.y[0] * m.y[0] + m.y[1] * m.y[1] + m.y[2] * m.y[2];
  double Q[6];
  int q = 0;
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int d = c; d < 3; ++d) Q[q++] = v * ((c == d ? yy : 0.0) - m.y[c] * m.y[d]);
  const double Xt[4] = {m.X[0], m.X[1], m.X[2], -1.0};
  int p = 0;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = a; b < 4; ++b) {
      const double xx = Xt[a] * Xt[b];
#pragma unroll
      for (int k = 0; k < 6; ++k) acc[6 * p + k] = __builtin_fma(xx, Q[k], acc[6 * p + k]);
      ++p;
    }
  acc[SBA_RESECT_MOM_N] += v;
}

// Lane sums -> one row per block: DPP wave sums (total in lane 63), the four waves added in wave order.
template <int COUNT>
__device__ __forceinline__ void resect_block_fold(const double* r, double (*red)[COUNT], double* __restrict__ row) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < COUNT; ++k) {
    const double v = wave_sum_to_lane63(r[k]);
    if (lane == 63) red[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < COUNT) {
    const int k = threadIdx.x;
    row[k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
  }
}

}  // namespace
}  // namespace sba
