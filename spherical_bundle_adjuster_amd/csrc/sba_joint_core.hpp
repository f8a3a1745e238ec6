// Device core of the joint solve's two passes (included by .hip files only): what sba_joint.hip (one problem, a grid of blocks)
// and sba_batch_joint.hip (a batch, one block per pair) compile from ONE source -- the per-match block, the per-match
// accumulation of either pass inside a lane's stream over its pairs of matches, and the fold of a block's lane partials to one row.
// Each loop is written once, in sba_joint_reduce_loop.inc / sba_joint_step_loop.inc.  The stream functions below expand them
// for the batched kernels; joint_reduce_kernel / joint_step_kernel (sba_joint.hip) expand the same two files in their own
// bodies instead of calling the stream functions (see there for why a call does not do).
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

// The same without the scaling planes, which a first pass never reads: what the covariance's two loops load
// (sba_cov_reduce_loop.inc / sba_cov_depth_loop.inc).
template <typename ST>
struct CovRegs {
  double X[2], Y[2], Z[2], U[2], V[2], W[2], A[2], B[2];
  __device__ __forceinline__ void load(const Planes& pl, const double* d1, const double* d2, size_t pr) {
    JPair<ST>::load(pl.x1[0], pr, X); JPair<ST>::load(pl.x1[1], pr, Y); JPair<ST>::load(pl.x1[2], pr, Z);
    JPair<ST>::load(pl.x2[0], pr, U); JPair<ST>::load(pl.x2[1], pr, V); JPair<ST>::load(pl.x2[2], pr, W);
    JPair<double>::load(d1, pr, A); JPair<double>::load(d2, pr, B);
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
  b.inv_det = 1.0 / depth_block_det(b.U11, b.U22, b.U12);
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
// step's loads in registers.  MAP: logical pair-of-matches index -> index into the planes (sba_pair_map.hpp).  The loop itself
// is sba_joint_reduce_loop.inc.
template <typename ST, typename MAP = IdentityMap>
__device__ __forceinline__ void joint_reduce_stream(const Planes& pl, const double* __restrict__ d1, const double* __restrict__ d2,
                                                    double* __restrict__ sc1, double* __restrict__ sc2, const JointParams& P,
                                                    size_t pr, size_t stride, double acc[JOINT_OUT_COUNT], const MAP map = MAP()) {
  const size_t n = P.cur.n, npairs = (n + 1) / 2;
  const bool load_scale = !P.first;
#pragma unroll
  for (int k = 0; k < JOINT_OUT_COUNT; ++k) acc[k] = 0.0;
#include "sba_joint_reduce_loop.inc"
}

// ... and of a step pass: candidates to (c1, c2).  The loop itself is sba_joint_step_loop.inc.
template <typename ST, typename MAP = IdentityMap>
__device__ __forceinline__ void joint_step_stream(const Planes& pl, const double* __restrict__ d1, const double* __restrict__ d2,
                                                  double* __restrict__ c1, double* __restrict__ c2, const double* __restrict__ sc1,
                                                  const double* __restrict__ sc2, const JointParams& P, size_t pr, size_t stride,
                                                  double acc[JOINT_STEP_COUNT], const MAP map = MAP()) {
  const size_t n = P.cur.n, npairs = (n + 1) / 2;
#pragma unroll
  for (int k = 0; k < JOINT_STEP_COUNT; ++k) acc[k] = 0.0;
#include "sba_joint_step_loop.inc"
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
