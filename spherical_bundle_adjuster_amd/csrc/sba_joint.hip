// Joint solve on the device: depths, rotation and translation free together (the reference's ba_spherical_costfunctor,
// spherical_bundle_adjuster.cpp:843-889: one 3-residual Huber block per match over (d_i[2], rot[3], tran[3])).
//
//   e_i = d2_i x2_i - d1_i R(w) x1_i + t,   E_i = d e / d d_i = [-u | x2]  (u = R x1),   F_i = d e / d (w, t) = [A_i | I],
//   A_i = -[a]x J  with a = v = -d1 u and J = J_l(w)  (small angles: a = -d1 x1, J = I -- the frame of sba_rotation.hpp).
//
// The depth blocks are private to a match, so they are eliminated per match (a damped 2x2 block U) and what crosses
// lanes is a fixed-size reduction.  One LM iteration is two streaming passes (step logic: sba_joint_solver.hpp):
//   joint_reduce_kernel  the reduced camera system S = sum (w F^T F - W^T U^-1 W), its gradient, the unreduced camera
//                        block in SBA_PACK_* layout, cost, outliers, max |g_d|; the first pass stores the depth scaling
//   joint_step_kernel    given the camera step: the same per-match block (same code, same bits), back-substitution
//                        delta d = -U^-1 (g_d + W delta c), candidate depths stored, cost at the candidate, model cost change
// Both: 256-thread blocks, grid-stride over 16-byte vectors (two matches per lane), the next step's loads in registers,
// DPP wave sums + LDS fold to one row per block, joint_finalize_kernel folds the rows in a fixed order and publishes to
// mapped host memory.  No atomics: bit-identical run to run.
// Bytes per match (f64 planes): reduce reads 64 (+16 scaling after the first pass, which writes 16), step reads 80 and writes 16.
#include <cstdlib>

#include "sba_device.hpp"
#include "sba_joint_core.hpp"
#include "sba_publish.hpp"

namespace sba {
namespace {

// The per-match block (JointBlock / joint_block), the plane accesses (JPair, JointRegs) and the block fold come from
// sba_joint_core.hpp, which the batched kernels (sba_batch_joint.hip) share.  The two loops below are ALSO in that header, as
// joint_reduce_stream / joint_step_stream over an address map, and the batched kernels use them from there.  These kernels
// keep their loops written out: routed through the stream functions the same lines compile to the same instruction counts
// but other last bits (which product of a sum is contracted into an FMA depends on the order the compiler meets them in) --
// S of a 4 097-match case moved from 2e-13 to 5e-12 off the long-double reference.  As they stand these three kernels are,
// instruction for instruction, the ones from before the header was split off.

// Pass 1.  ONE resident block per CU (one wave per SIMD): the 52 accumulators (104 registers), the register double buffer
// (80) and a match's temporaries need ~350 registers; held to 256 (two blocks per CU) the kernel spills 340-396 B of
// scratch into the hot loop, with the 512-register budget the overflow lives in accumulation registers instead.
template <typename ST>
__global__ __launch_bounds__(256, 1) void joint_reduce_kernel(Planes pl, const double* __restrict__ d1, const double* __restrict__ d2,
                                                             double* __restrict__ sc1, double* __restrict__ sc2, JointParams P,
                                                             double* __restrict__ partials) {
  __shared__ double red[4][JOINT_OUT_COUNT];
  const size_t n = P.cur.n, npairs = (n + 1) / 2, stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  size_t pr = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  const bool load_scale = !P.first;
  double acc[JOINT_OUT_COUNT];
#pragma unroll
  for (int k = 0; k < JOINT_OUT_COUNT; ++k) acc[k] = 0.0;
  JointRegs<ST> cur, nxt;
  if (pr < npairs) cur.load(pl, d1, d2, sc1, sc2, load_scale, pr);
  while (pr < npairs) {
    const size_t pn = pr + stride;
    if (pn < npairs) nxt.load(pl, d1, d2, sc1, sc2, load_scale, pn);
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
    if (P.first) { joint_store_pair(sc1, pr, NS1[0], NS1[1]); joint_store_pair(sc2, pr, NS2[0], NS2[1]); }
    cur = nxt;
    pr = pn;
  }
  joint_block_fold<JOINT_OUT_COUNT, JOINT_OUT_GDMAX>(acc, red, partials + static_cast<size_t>(blockIdx.x) * JOINT_ROW);
}

// Pass 2.
template <typename ST>
__global__ __launch_bounds__(256, 2) void joint_step_kernel(Planes pl, const double* __restrict__ d1, const double* __restrict__ d2,
                                                           double* __restrict__ c1, double* __restrict__ c2,
                                                           const double* __restrict__ sc1, const double* __restrict__ sc2,
                                                           JointParams P, double* __restrict__ partials) {
  __shared__ double red[4][JOINT_STEP_COUNT];
  const size_t n = P.cur.n, npairs = (n + 1) / 2, stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  size_t pr = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  double acc[JOINT_STEP_COUNT] = {0.0, 0.0, 0.0, 0.0};
  JointRegs<ST> cur, nxt;
  if (pr < npairs) cur.load(pl, d1, d2, sc1, sc2, true, pr);
  while (pr < npairs) {
    const size_t pn = pr + stride;
    if (pn < npairs) nxt.load(pl, d1, d2, sc1, sc2, true, pn);
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
    joint_store_pair(c1, pr, NA[0], NA[1]);
    joint_store_pair(c2, pr, NB[0], NB[1]);
    cur = nxt;
    pr = pn;
  }
  joint_block_fold<JOINT_STEP_COUNT, -1>(acc, red, partials + static_cast<size_t>(blockIdx.x) * JOINT_ROW);
}

// [nblocks][JOINT_ROW] -> out[count]: every slot folded in a fixed order (one wave per slot at a time: lane l takes rows l,
// l + 64, ..., then a butterfly), slot max_slot as a maximum.  With host_out (mapped pinned memory, JOINT_ROW + 1 words)
// the results are published to the host: stores, system-scope release, then the sequence number in host_out[JOINT_ROW].
__global__ __launch_bounds__(1024) void joint_finalize_kernel(const double* __restrict__ partials, int nblocks, int count, int max_slot,
                                                              double* __restrict__ out, double* __restrict__ host_out,
                                                              unsigned long long seq) {
  __shared__ double res[JOINT_ROW];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int slot = wave; slot < count; slot += 16) {
    const bool is_max = slot == max_slot;
    double v = 0.0;
    for (int b = lane; b < nblocks; b += 64) {
      const double a = partials[static_cast<size_t>(b) * JOINT_ROW + slot];
      v = is_max ? fmax(v, a) : v + a;
    }
    if (is_max) {
      v = joint_wave_max(v);
    } else {
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    }
    if (lane == 0) res[slot] = v;
  }
  __syncthreads();
  if (static_cast<int>(threadIdx.x) < count) {
    out[threadIdx.x] = res[threadIdx.x];
    if (host_out) host_store(host_out + threadIdx.x, res[threadIdx.x]);
  }
  if (host_out && threadIdx.x < 64) {     // count <= 64: wave 0 holds every host store
    host_release();
    if (threadIdx.x == 0)
      __hip_atomic_store(reinterpret_cast<unsigned long long*>(host_out + JOINT_ROW), seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}
static_assert(JOINT_OUT_COUNT <= 64 && JOINT_OUT_COUNT <= JOINT_ROW, "one wave publishes a row");

}  // namespace

hipError_t joint_blocks_per_cu(int store, int* blocks) {
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(
      blocks, reinterpret_cast<const void*>(store == 0 ? joint_reduce_kernel<double> : joint_reduce_kernel<float>), 256, 0);
}

hipError_t launch_joint_reduce(int store, const Planes& pl, const double* d1, const double* d2, double* sc1, double* sc2,
                               const JointParams& prm, double* partials, int grid, double* out, double* host_out,
                               unsigned long long seq, hipStream_t stream) {
  if (grid > 0) {
    if (store == 0) hipLaunchKernelGGL(joint_reduce_kernel<double>, dim3(grid), dim3(256), 0, stream, pl, d1, d2, sc1, sc2, prm, partials);
    else hipLaunchKernelGGL(joint_reduce_kernel<float>, dim3(grid), dim3(256), 0, stream, pl, d1, d2, sc1, sc2, prm, partials);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(joint_finalize_kernel, dim3(1), dim3(1024), 0, stream, partials, grid, static_cast<int>(JOINT_OUT_COUNT),
                     static_cast<int>(JOINT_OUT_GDMAX), out, host_out, seq);
  return hipGetLastError();
}

hipError_t launch_joint_step(int store, const Planes& pl, const double* d1, const double* d2, double* c1, double* c2,
                             const double* sc1, const double* sc2, const JointParams& prm, double* partials, int grid,
                             double* out, double* host_out, unsigned long long seq, hipStream_t stream) {
  if (grid > 0) {
    if (store == 0) hipLaunchKernelGGL(joint_step_kernel<double>, dim3(grid), dim3(256), 0, stream, pl, d1, d2, c1, c2, sc1, sc2, prm, partials);
    else hipLaunchKernelGGL(joint_step_kernel<float>, dim3(grid), dim3(256), 0, stream, pl, d1, d2, c1, c2, sc1, sc2, prm, partials);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(joint_finalize_kernel, dim3(1), dim3(1024), 0, stream, partials, grid, static_cast<int>(JOINT_STEP_COUNT), -1,
                     out, host_out, seq);
  return hipGetLastError();
}

}  // namespace sba
