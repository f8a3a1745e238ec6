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
// sba_joint_core.hpp, which the batched kernels (sba_batch_joint.hip) share.  The two per-match loops are written once, in
// sba_joint_reduce_loop.inc / sba_joint_step_loop.inc.  The kernels below expand those files in their own bodies (over the
// identity map); the batched kernels get them through the header's joint_reduce_stream / joint_step_stream.  A call of the
// stream functions here would not do: a function is unrolled and simplified on its own before it is inlined, the kernel then
// takes its parameters apart in another order, and the same lines come out with the same instruction counts but other last
// bits -- S of a 4 097-match case moved from 2e-13 to 5e-12 off the long-double reference.  Expanded in
// place, the kernels are instruction for instruction the ones from before the header was split off.

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
  const IdentityMap map;
#include "sba_joint_reduce_loop.inc"
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
  const IdentityMap map;
#include "sba_joint_step_loop.inc"
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

hipError_t launch_joint_finalize(const double* partials, int nblocks, int count, int max_slot, double* out, double* host_out,
                                 unsigned long long seq, hipStream_t stream) {
  hipLaunchKernelGGL(joint_finalize_kernel, dim3(1), dim3(1024), 0, stream, partials, nblocks, count, max_slot, out, host_out, seq);
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
