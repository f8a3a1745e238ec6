// The Hampel joint registration's reduce pass on the device (objective, loss and per-observation code:
// sba_landmarks_register_hampel.hpp, whose landmark_register_accumulate_hampel is the very function the kernel calls; the freeze
// and the write-back are sba_landmarks_register.hip's kernels, unchanged):
//   landmarks_register_hampel_reduce_kernel<INDEXED>  the nine planes + the bearing + the noise (104 B per observation) -> the 32
//                                                     sums of the Hampel row: the SBA_RESECT_* row with Hampel's weight of every
//                                                     observation's chi2 in H, g and the cost, n_outlier (chi2 > a^2) in
//                                                     SBA_RESECT_NOUT, and n_rejected (chi2 > c^2) in SBA_HAMPEL_NREJ;
//                                                     resect_block_fold to a block row of JOINT_ROW, then the joint solve's finalize
// The form of landmarks_register_robust_reduce_kernel: 256-thread blocks, grid-stride, plain stores, no atomics, bit-identical
// run to run at a fixed grid.
// dense:   lane p owns landmarks 2 p and 2 p + 1 through 16-byte plane vectors, keeps the next step's vectors in registers and
//          takes one landmark at a time (sched_barrier)
// indexed: lane p owns observations 2 p and 2 p + 1, the dense form's order of summation, so that idx = 0 .. n - 1 returns the
//          dense form's bits at the same grid
// The loss travels by value in LandmarkRegisterHampel beside LandmarkRegisterParams (scalar registers); its rows are chosen by
// selects, never by a branch.
#include "sba_device.hpp"
#include "sba_landmarks_device.hpp"
#include "sba_resection_core.hpp"      // resect_block_fold
#define SBA_LANDMARK_REGISTER_DEVICE_HUBER 1
#include "sba_landmarks_register_hampel.hpp"

namespace sba {
namespace {

static_assert(int(SBA_HAMPEL_COUNT) <= 64 && int(SBA_HAMPEL_COUNT) <= int(JOINT_ROW), "one wave publishes a row");

template <bool INDEXED>
__global__ __launch_bounds__(256) void landmarks_register_hampel_reduce_kernel(LandmarkRegisterParams P, LandmarkRegisterHampel L,
                                                                               double* __restrict__ base, unsigned long long elems,
                                                                               const long long* __restrict__ idx, const double* __restrict__ bearings,
                                                                               const double* __restrict__ noise, double* __restrict__ partials) {
  __shared__ double red[4][SBA_HAMPEL_COUNT];
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  double acc[SBA_HAMPEL_COUNT];
#pragma unroll
  for (int k = 0; k < SBA_HAMPEL_COUNT; ++k) acc[k] = 0.0;
  if (INDEXED) {
    const size_t m = P.m, nvec = (m + 1) / 2;
    for (size_t p = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; p < nvec; p += stride) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const bool valid = 2 * p + h < m;
        const size_t j = valid ? 2 * p + h : 0;            // an odd m: the last lane's second slot re-reads observation 0 and drops it
        const size_t i = static_cast<size_t>(idx[j]);      // < n: validated on the host
        double X[3], Sg[6], y[3];
        lm::gather(base, elems, i, bearings, j, X, Sg, y);
        const double s2 = noise[j];
        landmark_register_accumulate_hampel(P, L, X, Sg, y, s2, valid && landmark_register_live(s2), acc);
        __builtin_amdgcn_sched_barrier(0);                 // one observation at a time
      }
    }
  } else {
    const size_t n = P.n, nvec = (n + 1) / 2;
    size_t p = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    lm::PairRegs<true> cur, nxt;
    if (p < nvec) cur.load(base, elems, bearings, noise, p);
    while (p < nvec) {
      const size_t pn = p + stride;
      if (pn < nvec) nxt.load(base, elems, bearings, noise, pn);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        double X[3], Sg[6], y[3];
        cur.get(h, X, Sg, y);
        const double s2 = cur.noise(h);
        landmark_register_accumulate_hampel(P, L, X, Sg, y, s2, 2 * p + h < n && landmark_register_live(s2), acc);
        __builtin_amdgcn_sched_barrier(0);                 // one landmark at a time, as in landmarks_register_reduce_kernel
      }
      cur = nxt;
      p = pn;
    }
  }
  resect_block_fold<SBA_HAMPEL_COUNT>(acc, red, partials + static_cast<size_t>(blockIdx.x) * JOINT_ROW);
}

}  // namespace

hipError_t landmarks_register_hampel_blocks_per_cu(bool indexed, int* blocks) {
  const void* k = indexed ? reinterpret_cast<const void*>(landmarks_register_hampel_reduce_kernel<true>)
                          : reinterpret_cast<const void*>(landmarks_register_hampel_reduce_kernel<false>);
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks, k, 256, 0);
}

hipError_t launch_landmarks_register_hampel_reduce(const LandmarkPlanes& pl, const LandmarkRegisterParams& prm, const LandmarkRegisterHampel& loss,
                                                   const long long* idx, const double* bearings, const double* noise, double* partials, int grid,
                                                   double* out, hipStream_t stream) {
  if (grid <= 0) return hipErrorInvalidValue;
  const unsigned long long elems = pl.elems;
  if (idx) hipLaunchKernelGGL(landmarks_register_hampel_reduce_kernel<true>, dim3(grid), dim3(256), 0, stream, prm, loss, pl.base, elems, idx, bearings, noise, partials);
  else hipLaunchKernelGGL(landmarks_register_hampel_reduce_kernel<false>, dim3(grid), dim3(256), 0, stream, prm, loss, pl.base, elems, idx, bearings, noise, partials);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return launch_joint_finalize(partials, grid, SBA_HAMPEL_COUNT, -1, out, nullptr, 0, stream);
}

}  // namespace sba
