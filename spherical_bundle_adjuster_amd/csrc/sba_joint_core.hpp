// Device core of the joint solve's two passes (included by .hip files only): what sba_joint.hip (one problem, a grid of blocks)
// and sba_batch_joint.hip (a batch, one block per pair) compile from ONE source -- the per-match block, the per-match
// accumulation of either pass inside a lane's stream over its pairs of matches, and the fold of a block's lane partials to one row.
// The stream functions serve the batched kernels; sba_joint.hip keeps the same two loops written out in its kernels (see there:
// routed through a function they compile to other last bits, and those kernels' results are pinned).
//
//   e_i = d2_i x2_i - d1_i R(w) x1_i + t,   E_i = d e / d d_i = [-u | x2]  (u = R x1),   F_i = d e / d (w, t) = [A_i | I],
//   A_i = -[a]x J  with a = v = -d1 u and J = J_l(w)  (small angles: a = -d1 x1, J = I -- the frame of sba_rotation.hpp).
#pragma once
#include "sba_device.hpp"
#include "sba_pair_map.hpp"
#include "sba_sweep_core.hpp"

namespace sba {
namespace {

__device__ __forceinline__ double joint_wave_max(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off));
  return v;
}

template <typename ST> struct JPair;
template <> struct JPair<double> {
  static __device__ __forceinline__ void load(const void* plane, size_t pair, double out[2]) {
    typedef float f4 __attribute__((ext_vector_type(4)));
    const f4 r = __builtin_nontemporal_load(reinterpret_cast<const f4*>(plane) + pair);
    const double2 q = *reinterpret_cast<const double2*>(&r);
    out[0] = q.x; out[1] = q.y;
  }
};
template <> struct JPair<float> {
  static __device__ __forceinline__ void load(const void* plane, size_t pair, double out[2]) {
    const float2 q = reinterpret_cast<const float2*>(plane)[pair];
    out[0] = q.x; out[1] = q.y;
  }
};
__device__ __forceinline__ void joint_store_pair(double* plane, size_t pair, double a, double b) {
  reinterpret_cast<double2*>(plane)[pair] = make_double2(a, b);
}

// What one lane reads for its two matches of one stride step, loaded one step ahead of its use.
template <typename ST>
struct JointRegs {
  double X[2], Y[2], Z[2], U[2], V[2], W[2], A[2], B[2], S1[2], S2[2];
  __device__ __forceinline__ void load(const Planes& pl, const double* d1, const double* d2, const double* sc1,
                                       const double* sc2, bool load_scale, size_t pr) {
    JPair<ST>::load(pl.x1[0], pr, X); JPair<ST>::load(pl.x1[1], pr, Y); JPair<ST>::load(pl.x1[2], pr, Z);
    JPair<ST>::load(pl.x2[0], pr, U); JPair<ST>::load(pl.x2[1], pr, V); JPair<ST>::load(pl.x2[2], pr, W);
    JPair<double>::load(d1, pr, A); JPair<double>::load(d2, pr, B);
    if (load_scale) { JPair<double>::load(sc1, pr, S1); JPair<double>::load(sc2, pr, S2); }
  }
};

// The per-match block at the current point: residual, Huber weight, Jacobian pieces, the scaled damped 2x2 depth block.
// Both passes call this very function with the same inputs, so U, W and g_d agree to the bit between the passes.
struct JointBlock {
  double e[3], w, rho, is_out;
  double nu[3];         // -u = first column of E
  double A[3][3];       // A[r][j] = d e_r / d w_j
  double s1, s2;        // depth Jacobi scaling
  double U11, U12, U22, inv_det;
  double G1, G2;        // scaled depth gradient
  double gd1, gd2;      // unscaled depth gradient
  double w1[6], w2[6];  // rows of W = w E_s^T F
};

__device__ __forceinline__ void joint_block(const JointParams& P, double x, double y, double z, double u, double v, double q,
                                            double d1, double d2, double sc1, double sc2, bool valid, JointBlock& b) {
  double X = x, Y = y, Z = z, Uc = u, Vc = v, Qc = q, r0, r1, r2;
  residual<DEPTH_PER_MATCH>(&P.cur, X, Y, Z, Uc, Vc, Qc, d1, d2, r0, r1, r2, b.e[0], b.e[1], b.e[2]);
  const double s = sq_norm(b.e[0], b.e[1], b.e[2]);
  b.w = 1.0; b.rho = s; b.is_out = 0.0;
  if (P.cur.delta > 0.0) huber(s, P.cur.delta, P.cur.delta2, b.w, b.rho, b.is_out);
  if (!valid) { b.w = 0.0; b.rho = 0.0; b.is_out = 0.0; }
  const double* Rn = P.cur.Rn;
  b.nu[0] = Rn[0] * x + Rn[1] * y + Rn[2] * z;
  b.nu[1] = Rn[3] * x + Rn[4] * y + Rn[5] * z;
  b.nu[2] = Rn[6] * x + Rn[7] * y + Rn[8] * z;
  const double a0 = P.small_angle ? -X : r0, a1 = P.small_angle ? -Y : r1, a2 = P.small_angle ? -Z : r2;
#pragma unroll
  for (int j = 0; j < 3; ++j) {          // A = -[a]x J: column j = J[:, j] x a
    const double j0 = P.J[j], j1 = P.J[3 + j], j2 = P.J[6 + j];
    b.A[0][j] = j1 * a2 - j2 * a1;
    b.A[1][j] = j2 * a0 - j0 * a2;
    b.A[2][j] = j0 * a1 - j1 * a0;
  }
  const double nn = b.nu[0] * b.nu[0] + b.nu[1] * b.nu[1] + b.nu[2] * b.nu[2];
  const double nx = b.nu[0] * u + b.nu[1] * v + b.nu[2] * q, xx = u * u + v * v + q * q;
  const double h11 = b.w * nn, h12 = b.w * nx, h22 = b.w * xx;
  b.gd1 = b.w * (b.nu[0] * b.e[0] + b.nu[1] * b.e[1] + b.nu[2] * b.e[2]);
  b.gd2 = b.w * (u * b.e[0] + v * b.e[1] + q * b.e[2]);
  if (P.first) {
    b.s1 = P.jacobi_scaling ? 1.0 / (1.0 + sqrt(h11)) : 1.0;
    b.s2 = P.jacobi_scaling ? 1.0 / (1.0 + sqrt(h22)) : 1.0;
  } else {
    b.s1 = sc1; b.s2 = sc2;
  }
  const double H11 = b.s1 * h11 * b.s1, H22 = b.s2 * h22 * b.s2;
  // The LM diagonal is recomputed at the point it belongs to (rejected steps re-run the pass there): same bits, no plane.
  const double D1 = fmin(fmax(H11, P.min_diagonal), P.max_diagonal), D2 = fmin(fmax(H22, P.min_diagonal), P.max_diagonal);
  b.U11 = __builtin_fma(D1, P.inv_radius, H11);
  b.U22 = __builtin_fma(D2, P.inv_radius, H22);
  b.U12 = b.s1 * h12 * b.s2;
  if (!valid) { b.U11 = 1.0; b.U22 = 1.0; b.U12 = 0.0; }     // the padding match of an odd-sized problem: weight 0, any regular block
  b.inv_det = 1.0 / (b.U11 * b.U22 - b.U12 * b.U12);
  b.G1 = b.s1 * b.gd1; b.G2 = b.s2 * b.gd2;
  const double k1 = b.s1 * b.w, k2 = b.s2 * b.w;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    b.w1[j] = k1 * (b.nu[0] * b.A[0][j] + b.nu[1] * b.A[1][j] + b.nu[2] * b.A[2][j]);
    b.w2[j] = k2 * (u * b.A[0][j] + v * b.A[1][j] + q * b.A[2][j]);
    b.w1[3 + j] = k1 * b.nu[j];
  }
  b.w2[3] = k2 * u; b.w2[4] = k2 * v; b.w2[5] = k2 * q;
}

static_assert(SBA_PACK_GT == SBA_PACK_GA + 3 && SBA_PACK_SIZE == JOINT_OUT_S, "joint row layout");

// One lane's share of a reduce pass: its pairs of matches pr, pr + stride, ... of a problem of P.cur.n matches, the next
// step's loads in registers.  MAP: logical pair-of-matches index -> index into the planes (sba_pair_map.hpp).
template <typename ST, typename MAP = IdentityMap>
__device__ __forceinline__ void joint_reduce_stream(const Planes& pl, const double* __restrict__ d1, const double* __restrict__ d2,
                                                    double* __restrict__ sc1, double* __restrict__ sc2, const JointParams& P,
                                                    size_t pr, size_t stride, double acc[JOINT_OUT_COUNT], const MAP map = MAP()) {
  const size_t n = P.cur.n, npairs = (n + 1) / 2;
  const bool load_scale = !P.first;
#pragma unroll
  for (int k = 0; k < JOINT_OUT_COUNT; ++k) acc[k] = 0.0;
  JointRegs<ST> cur, nxt;
  if (pr < npairs) cur.load(pl, d1, d2, sc1, sc2, load_scale, map(pr));
  while (pr < npairs) {
    const size_t pn = pr + stride, q = map(pr);
    if (pn < npairs) nxt.load(pl, d1, d2, sc1, sc2, load_scale, map(pn));
    double NS1[2], NS2[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const bool valid = 2 * pr + h < n;
      JointBlock b;
      joint_block(P, cur.X[h], cur.Y[h], cur.Z[h], cur.U[h], cur.V[h], cur.W[h], cur.A[h], cur.B[h], cur.S1[h], cur.S2[h], valid, b);
      NS1[h] = b.s1; NS2[h] = b.s2;
      const double w = b.w;
      // unreduced camera block, SBA_PACK_* layout (as the explicit sweep kernel accumulates it)
      double wA[3][3];
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int j = 0; j < 3; ++j) wA[r][j] = w * b.A[r][j];
      double ff[21], fe[6];      // w F^T F (upper, row by row) and w F^T e of this match
      int k = 0;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int c = a; c < 3; ++c) ff[k++] = wA[0][a] * b.A[0][c] + wA[1][a] * b.A[1][c] + wA[2][a] * b.A[2][c];
#pragma unroll
        for (int c = 0; c < 3; ++c) ff[k++] = wA[c][a];
        fe[a] = wA[0][a] * b.e[0] + wA[1][a] * b.e[1] + wA[2][a] * b.e[2];
      }
      ff[15] = w; ff[16] = 0.0; ff[17] = 0.0; ff[18] = w; ff[19] = 0.0; ff[20] = w;
      fe[3] = w * b.e[0]; fe[4] = w * b.e[1]; fe[5] = w * b.e[2];
      // pack slots: HAA = ff[0..2], ff[6..7], ff[11]; HAT[3 a + c] = ff rows a, columns 3..5
      acc[0] += ff[0]; acc[1] += ff[1]; acc[2] += ff[2]; acc[3] += ff[6]; acc[4] += ff[7]; acc[5] += ff[11];
      acc[6] += ff[3]; acc[7] += ff[4]; acc[8] += ff[5]; acc[9] += ff[8]; acc[10] += ff[9]; acc[11] += ff[10];
      acc[12] += ff[12]; acc[13] += ff[13]; acc[14] += ff[14];
      acc[SBA_PACK_SW] += w;
#pragma unroll
      for (int a = 0; a < 6; ++a) acc[SBA_PACK_GA + a] += fe[a];          // GA[3], GT[3] are consecutive slots
      acc[SBA_PACK_COST] = __builtin_fma(0.5, b.rho, acc[SBA_PACK_COST]);
      acc[SBA_PACK_NOUT] += b.is_out;
      // Schur complement of the depth block: z = U^-1 W (two rows), T = W^T z
      double z1[6], z2[6];
#pragma unroll
      for (int a = 0; a < 6; ++a) {
        z1[a] = (b.U22 * b.w1[a] - b.U12 * b.w2[a]) * b.inv_det;
        z2[a] = (b.U11 * b.w2[a] - b.U12 * b.w1[a]) * b.inv_det;
      }
      k = 0;
#pragma unroll
      for (int a = 0; a < 6; ++a) {
#pragma unroll
        for (int c = a; c < 6; ++c) {
          acc[JOINT_OUT_S + k] += ff[k] - (b.w1[a] * z1[c] + b.w2[a] * z2[c]);
          ++k;
        }
        acc[JOINT_OUT_GS + a] += fe[a] - (z1[a] * b.G1 + z2[a] * b.G2);
      }
      if (valid) acc[JOINT_OUT_GDMAX] = fmax(acc[JOINT_OUT_GDMAX], fmax(fabs(b.gd1), fabs(b.gd2)));
    }
    if (P.first) { joint_store_pair(sc1, q, NS1[0], NS1[1]); joint_store_pair(sc2, q, NS2[0], NS2[1]); }
    cur = nxt;
    pr = pn;
  }
}

// ... and of a step pass: candidates to (c1, c2).
template <typename ST, typename MAP = IdentityMap>
__device__ __forceinline__ void joint_step_stream(const Planes& pl, const double* __restrict__ d1, const double* __restrict__ d2,
                                                  double* __restrict__ c1, double* __restrict__ c2, const double* __restrict__ sc1,
                                                  const double* __restrict__ sc2, const JointParams& P, size_t pr, size_t stride,
                                                  double acc[JOINT_STEP_COUNT], const MAP map = MAP()) {
  const size_t n = P.cur.n, npairs = (n + 1) / 2;
#pragma unroll
  for (int k = 0; k < JOINT_STEP_COUNT; ++k) acc[k] = 0.0;
  JointRegs<ST> cur, nxt;
  if (pr < npairs) cur.load(pl, d1, d2, sc1, sc2, true, map(pr));
  while (pr < npairs) {
    const size_t pn = pr + stride, q = map(pr);
    if (pn < npairs) nxt.load(pl, d1, d2, sc1, sc2, true, map(pn));
    double NA[2], NB[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const bool valid = 2 * pr + h < n;
      const double x = cur.X[h], y = cur.Y[h], z = cur.Z[h], u = cur.U[h], v = cur.V[h], q = cur.W[h];
      const double a = cur.A[h], bd = cur.B[h];
      JointBlock b;
      joint_block(P, x, y, z, u, v, q, a, bd, cur.S1[h], cur.S2[h], valid, b);
      // delta d = -U^-1 (g_d + W delta c), in scaled coordinates, then unscaled
      double t1 = b.G1, t2 = b.G2;
#pragma unroll
      for (int k = 0; k < 6; ++k) { t1 += b.w1[k] * P.delta_c[k]; t2 += b.w2[k] * P.delta_c[k]; }
      const double y1 = (b.U12 * t2 - b.U22 * t1) * b.inv_det, y2 = (b.U12 * t1 - b.U11 * t2) * b.inv_det;
      const double dl1 = b.s1 * y1, dl2 = b.s2 * y2;
      const double na = a + dl1, nb = bd + dl2;
      NA[h] = valid ? na : 0.0; NB[h] = valid ? nb : 0.0;     // the padding stays zero
      // J delta = E delta d + A delta w + delta t
      double jd[3];
#pragma unroll
      for (int r = 0; r < 3; ++r)
        jd[r] = b.nu[r] * dl1 + (r == 0 ? u : (r == 1 ? v : q)) * dl2 + b.A[r][0] * P.delta_c[0] + b.A[r][1] * P.delta_c[1] +
                b.A[r][2] * P.delta_c[2] + P.delta_c[3 + r];
      // the residual at the candidate (w', t', d'), formed as every residual of the library
      double X = x, Y = y, Z = z, Uc = u, Vc = v, Qc = q, r0, r1, r2, f0, f1, f2;
      residual<DEPTH_PER_MATCH>(&P.cand, X, Y, Z, Uc, Vc, Qc, na, nb, r0, r1, r2, f0, f1, f2);
      const double sc = sq_norm(f0, f1, f2);
      double wc = 1.0, rhoc = sc, outc = 0.0;
      if (P.cur.delta > 0.0) huber(sc, P.cur.delta, P.cur.delta2, wc, rhoc, outc);
      if (valid) {
        acc[JOINT_STEP_CAND_COST] = __builtin_fma(0.5, rhoc, acc[JOINT_STEP_CAND_COST]);
        acc[JOINT_STEP_MODEL] -= b.w * (jd[0] * (b.e[0] + 0.5 * jd[0]) + jd[1] * (b.e[1] + 0.5 * jd[1]) + jd[2] * (b.e[2] + 0.5 * jd[2]));
        acc[JOINT_STEP_DSTEP2] += dl1 * dl1 + dl2 * dl2;
        acc[JOINT_STEP_D2] += a * a + bd * bd;
      }
    }
    joint_store_pair(c1, q, NA[0], NA[1]);
    joint_store_pair(c2, q, NB[0], NB[1]);
    cur = nxt;
    pr = pn;
  }
}

// Lane partials -> one row per block: sums by DPP (total in lane 63), maxima by butterfly, the four waves in wave order.
template <int COUNT, int MAX_SLOT>
__device__ __forceinline__ void joint_block_fold(const double* r, double (*red)[COUNT], double* __restrict__ row) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < COUNT; ++k) {
    if (k == MAX_SLOT) {
      const double v = joint_wave_max(r[k]);
      if (lane == 63) red[wave][k] = v;
    } else {
      const double v = wave_sum_to_lane63(r[k]);
      if (lane == 63) red[wave][k] = v;
    }
  }
  __syncthreads();
  if (threadIdx.x < COUNT) {
    const int k = threadIdx.x;
    double s = red[0][k];
    for (int wv = 1; wv < 4; ++wv) s = k == MAX_SLOT ? fmax(s, red[wv][k]) : s + red[wv][k];
    row[k] = s;
  }
}

}  // namespace
}  // namespace sba
