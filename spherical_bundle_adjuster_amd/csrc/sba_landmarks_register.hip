// The joint registration of a frame against the landmark map, on the device (algebra and per-observation code:
// sba_landmarks_register.hpp, whose landmark_register_noise / _accumulate / _one are the very functions the kernels call; the
// planes: sba_landmarks.hip).  With the pose held every landmark is eliminated exactly, so one evaluation of the six-parameter
// problem is ONE streaming reduction over the map, and nothing per landmark is stored between iterations but the frozen noise:
//   landmarks_register_freeze_kernel<INDEXED>         the nine planes + the bearing at the start pose -> the noise plane (8 B per
//                                                     observation: s_j^2, or the marker of an observation that takes no part) and
//                                                     the freeze's class counts; once per registration
//   landmarks_register_reduce_kernel<INDEXED>         the nine planes + the bearing + the noise (104 B per observation) -> the 31
//                                                     sums of the SBA_RESECT_* row; resect_block_fold to a block row of JOINT_ROW,
//                                                     then the joint solve's finalize
//   landmarks_register_apply_kernel<INDEXED, APPLY>   the write-back at the solution with Sigma_c: X+, Sigma+, the count, chi2 and
//                                                     the class counts; APPLY = false: chi2 and counts only.  The body is
//                                                     sba_landmarks_pass.inc around landmark_register_one: the fusion's, with the noise
// dense:   lane p owns landmarks 2 p and 2 p + 1 through 16-byte plane vectors; the reduce pass keeps the next step's vectors in
//          registers and every pass takes one landmark at a time (sched_barrier)
// indexed: lane j owns observation j and gathers landmark idx[j] (sorted: neighbouring lanes, neighbouring lines); in the reduce
//          pass lane p owns observations 2 p and 2 p + 1, the dense form's order of summation, so that idx = 0 .. n - 1 returns
//          the dense form's bits
// All: 256-thread blocks, grid-stride, plain stores, no floating-point atomics.  The reduce pass is bit-identical run to run at
// a fixed grid; the two passes without a reduction do not depend on the grid at all.  The register block of a dense lane
// (lm::PairRegs), the indexed gather and the class counts (lm::ClassCounts): sba_landmarks_device.hpp.
#include "sba_device.hpp"
#include "sba_landmarks_device.hpp"
#include "sba_landmarks_register.hpp"
#include "sba_resection_core.hpp"

namespace sba {
namespace {

template <bool INDEXED>
__global__ __launch_bounds__(256) void landmarks_register_freeze_kernel(LandmarkRegisterParams P, double* __restrict__ base, unsigned long long elems,
                                                                        const long long* __restrict__ idx, const double* __restrict__ bearings,
                                                                        double* __restrict__ noise, unsigned long long* __restrict__ counters) {
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  lm::ClassCounts<LANDMARK_CLASSES> cc;
  cc.init();
  if (INDEXED) {
    const size_t m = P.m;
    for (size_t j = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; j < m; j += stride) {
      const size_t i = static_cast<size_t>(idx[j]);        // < n: validated on the host
      double X[3], Sg[6], y[3], s2;
      lm::gather(base, elems, i, bearings, j, X, Sg, y);
      cc.add(true, landmark_register_noise(P, X, Sg, y, &s2));
      noise[j] = s2;
    }
  } else {
    const size_t n = P.n, nvec = (n + 1) / 2;
    for (size_t p = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; p < nvec; p += stride) {
      lm::PairRegs<false> cur;
      cur.load(base, elems, bearings, nullptr, p);
      double s2[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        double X[3], Sg[6], y[3];
        cur.get(h, X, Sg, y);
        const bool valid = 2 * p + h < n;
        cc.add(valid, landmark_register_noise(P, X, Sg, y, &s2[h]));
        if (!valid) s2[h] = NAN;                           // the padding row takes no part
        __builtin_amdgcn_sched_barrier(0);                 // one landmark at a time
      }
      reinterpret_cast<double2*>(noise)[p] = make_double2(s2[0], s2[1]);
    }
  }
  cc.flush(counters);
}

// 31 accumulators (62 registers), the dense form's double buffer of 2 x 26 and one landmark's temporaries: one resident block
// per CU rather than a spill.
template <bool INDEXED>
__global__ __launch_bounds__(256) void landmarks_register_reduce_kernel(LandmarkRegisterParams P, double* __restrict__ base, unsigned long long elems,
                                                                        const long long* __restrict__ idx, const double* __restrict__ bearings,
                                                                        const double* __restrict__ noise, double* __restrict__ partials) {
  __shared__ double red[4][SBA_RESECT_COUNT];
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  double acc[SBA_RESECT_COUNT];
#pragma unroll
  for (int k = 0; k < SBA_RESECT_COUNT; ++k) acc[k] = 0.0;
  if (INDEXED) {
    // Observations 2 p and 2 p + 1 in this order, as the dense form takes landmarks: at the same grid the sums over
    // idx = 0 .. n - 1 are the dense form's bit for bit.
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
        landmark_register_accumulate(P, X, Sg, y, s2, valid && landmark_register_live(s2), acc);
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
        landmark_register_accumulate(P, X, Sg, y, s2, 2 * p + h < n && landmark_register_live(s2), acc);
        __builtin_amdgcn_sched_barrier(0);                 // one landmark at a time, as in resect_wreduce_kernel
      }
      cur = nxt;
      p = pn;
    }
  }
  resect_block_fold<SBA_RESECT_COUNT>(acc, red, partials + static_cast<size_t>(blockIdx.x) * JOINT_ROW);
}

template <bool INDEXED, bool APPLY>
__global__ __launch_bounds__(256) void landmarks_register_apply_kernel(LandmarkRegisterParams P, double* __restrict__ base, unsigned long long elems,
                                                                       const long long* __restrict__ idx, const double* __restrict__ bearings,
                                                                       const double* __restrict__ noise, double* __restrict__ chi2,
                                                                       unsigned long long* __restrict__ counters) {
  constexpr bool NOISE = true;
#define SBA_LANDMARK_PASS_ONE(X, Sg, y, nz, Xo, So, chi2) landmark_register_one(P, X, Sg, y, nz, Xo, So, chi2)
#include "sba_landmarks_pass.inc"
#undef SBA_LANDMARK_PASS_ONE
}

const void* register_kernel_of(int which, bool indexed, bool apply) {
  if (which == LANDMARK_REGISTER_FREEZE)
    return indexed ? reinterpret_cast<const void*>(landmarks_register_freeze_kernel<true>) : reinterpret_cast<const void*>(landmarks_register_freeze_kernel<false>);
  if (which == LANDMARK_REGISTER_REDUCE)
    return indexed ? reinterpret_cast<const void*>(landmarks_register_reduce_kernel<true>) : reinterpret_cast<const void*>(landmarks_register_reduce_kernel<false>);
  if (indexed) return apply ? reinterpret_cast<const void*>(landmarks_register_apply_kernel<true, true>) : reinterpret_cast<const void*>(landmarks_register_apply_kernel<true, false>);
  return apply ? reinterpret_cast<const void*>(landmarks_register_apply_kernel<false, true>) : reinterpret_cast<const void*>(landmarks_register_apply_kernel<false, false>);
}

}  // namespace

hipError_t landmarks_register_blocks_per_cu(int which, bool indexed, bool apply, int* blocks) {
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks, register_kernel_of(which, indexed, apply), 256, 0);
}

hipError_t launch_landmarks_register_freeze(const LandmarkPlanes& pl, const LandmarkRegisterParams& prm, const long long* idx, const double* bearings,
                                            double* noise, unsigned long long* counters, int grid, hipStream_t stream) {
  const hipError_t e = hipMemsetAsync(counters, 0, LANDMARK_CLASSES * sizeof(unsigned long long), stream);
  if (e != hipSuccess || grid <= 0) return e;
  const unsigned long long elems = pl.elems;
  if (idx) hipLaunchKernelGGL(landmarks_register_freeze_kernel<true>, dim3(grid), dim3(256), 0, stream, prm, pl.base, elems, idx, bearings, noise, counters);
  else hipLaunchKernelGGL(landmarks_register_freeze_kernel<false>, dim3(grid), dim3(256), 0, stream, prm, pl.base, elems, idx, bearings, noise, counters);
  return hipGetLastError();
}

hipError_t launch_landmarks_register_reduce(const LandmarkPlanes& pl, const LandmarkRegisterParams& prm, const long long* idx, const double* bearings,
                                            const double* noise, double* partials, int grid, double* out, hipStream_t stream) {
  if (grid <= 0) return hipErrorInvalidValue;
  const unsigned long long elems = pl.elems;
  if (idx) hipLaunchKernelGGL(landmarks_register_reduce_kernel<true>, dim3(grid), dim3(256), 0, stream, prm, pl.base, elems, idx, bearings, noise, partials);
  else hipLaunchKernelGGL(landmarks_register_reduce_kernel<false>, dim3(grid), dim3(256), 0, stream, prm, pl.base, elems, idx, bearings, noise, partials);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return launch_joint_finalize(partials, grid, SBA_RESECT_COUNT, -1, out, nullptr, 0, stream);
}

hipError_t launch_landmarks_register_apply(const LandmarkPlanes& pl, const LandmarkRegisterParams& prm, const long long* idx, const double* bearings,
                                           const double* noise, double* chi2, unsigned long long* counters, bool apply, int grid, hipStream_t stream) {
  const hipError_t e = hipMemsetAsync(counters, 0, LANDMARK_CLASSES * sizeof(unsigned long long), stream);
  if (e != hipSuccess || grid <= 0) return e;
  const unsigned long long elems = pl.elems;
  if (idx && apply) hipLaunchKernelGGL((landmarks_register_apply_kernel<true, true>), dim3(grid), dim3(256), 0, stream, prm, pl.base, elems, idx, bearings, noise, chi2, counters);
  else if (idx) hipLaunchKernelGGL((landmarks_register_apply_kernel<true, false>), dim3(grid), dim3(256), 0, stream, prm, pl.base, elems, idx, bearings, noise, chi2, counters);
  else if (apply) hipLaunchKernelGGL((landmarks_register_apply_kernel<false, true>), dim3(grid), dim3(256), 0, stream, prm, pl.base, elems, idx, bearings, noise, chi2, counters);
  else hipLaunchKernelGGL((landmarks_register_apply_kernel<false, false>), dim3(grid), dim3(256), 0, stream, prm, pl.base, elems, idx, bearings, noise, chi2, counters);
  return hipGetLastError();
}

}  // namespace sba
