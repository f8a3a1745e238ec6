// Spherical resection on the device: a new frame's pose from landmarks X_i = d1_i x1_i and bearings y_i = x2_i (algebra and
// row layout: sba_resection.hpp, per-match code: sba_resection_core.hpp).  The bearing's depth is eliminated in closed form,
// so one evaluation of the six-parameter problem is ONE streaming reduction:
//   resect_reduce_kernel   H (21), g (6), cost, sum w, Huber outliers, n_behind: 31 sums per lane
//   resect_moments_kernel  the 60 sums of the linear starting point (DLT) and the match count; once per guess
//   resect_depths_kernel   d_i* into the handle's d2 plane; no reduction
// All: 256-thread blocks, grid-stride over 16-byte vectors (2 matches per lane with f64 planes, 4 with f32), the next
// step's loads in registers, non-temporal loads.  The two reductions: DPP wave sums + LDS fold to one row per block,
// joint_finalize_kernel (sba_joint.hip) folds the rows in a fixed order and publishes to mapped host memory.  No atomics:
// bit-identical run to run for a fixed grid.
// Bytes per match (f64 planes): 56 read by each pass -- the d2 plane is never read; the depth pass writes 8.
#include "sba_device.hpp"
#include "sba_resection_core.hpp"

namespace sba {
namespace {

// Two resident blocks per CU (two waves per SIMD, 256 registers each): 62 accumulator registers, the double buffer (28 with
// f64 planes) and a match's temporaries fit without scratch.
template <typename ST, bool LOSS>
__global__ __launch_bounds__(256, 2) void resect_reduce_kernel(Planes pl, ResectParams P, double* __restrict__ partials) {
  __shared__ double red[4][SBA_RESECT_COUNT];
  constexpr int PPT = Lanes<ST>::PPT;
  const size_t n = P.n, nvec = (n + PPT - 1) / PPT, stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  size_t p = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  double acc[SBA_RESECT_COUNT];
#pragma unroll
  for (int k = 0; k < SBA_RESECT_COUNT; ++k) acc[k] = 0.0;
  ResectRegs<ST> cur, nxt;
  if (p < nvec) cur.load(pl, p);
  while (p < nvec) {
    const size_t pn = p + stride;
    if (pn < nvec) nxt.load(pl, pn);
#pragma unroll
    for (int h = 0; h < PPT; ++h) {
      const bool valid = p * PPT + h < n;
      ResectMatch m;
      resect_match(cur, h, valid, m);
      resect_accumulate<LOSS>(P, m, valid, acc);
      // one match at a time: interleaved, the four matches of an f32 vector want more than the 256 registers of a wave
      __builtin_amdgcn_sched_barrier(0);
    }
    cur = nxt;
    p = pn;
  }
  resect_block_fold<SBA_RESECT_COUNT>(acc, red, partials + static_cast<size_t>(blockIdx.x) * JOINT_ROW);
}

// One block per CU: 61 sums per lane (122 registers) and the double buffer.
template <typename ST>
__global__ __launch_bounds__(256, 1) void resect_moments_kernel(Planes pl, unsigned long long n_matches, double* __restrict__ partials) {
  __shared__ double red[4][SBA_RESECT_MOM_COUNT];
  constexpr int PPT = Lanes<ST>::PPT;
  const size_t n = n_matches, nvec = (n + PPT - 1) / PPT, stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  size_t p = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  double acc[SBA_RESECT_MOM_COUNT];
#pragma unroll
  for (int k = 0; k < SBA_RESECT_MOM_COUNT; ++k) acc[k] = 0.0;
  ResectRegs<ST> cur, nxt;
  if (p < nvec) cur.load(pl, p);
  while (p < nvec) {
    const size_t pn = p + stride;
    if (pn < nvec) nxt.load(pl, pn);
#pragma unroll
    for (int h = 0; h < PPT; ++h) {
      const bool valid = p * PPT + h < n;
      ResectMatch m;
      resect_match(cur, h, valid, m);
      resect_moments(m, valid, acc);
    }
    cur = nxt;
    p = pn;
  }
  resect_block_fold<SBA_RESECT_MOM_COUNT>(acc, red, partials + static_cast<size_t>(blockIdx.x) * JOINT_ROW);
}

// d_i* of every match into d2, whole vectors (zeros in the padding of the last one, as an uploaded plane has them).
template <typename ST>
__global__ __launch_bounds__(256) void resect_depths_kernel(Planes pl, ResectParams P, double* __restrict__ d2) {
  constexpr int PPT = Lanes<ST>::PPT;
  const size_t n = P.n, nvec = (n + PPT - 1) / PPT, stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (size_t p = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; p < nvec; p += stride) {
    ResectRegs<ST> cur;
    cur.load(pl, p);
    double out[PPT];
#pragma unroll
    for (int h = 0; h < PPT; ++h) {
      const bool valid = p * PPT + h < n;
      ResectMatch m;
      resect_match(cur, h, valid, m);
      double inv_yy, dstar, c[3], r[3];
      resect_residual(P, m, inv_yy, dstar, c, r);
      out[h] = valid ? dstar : 0.0;
    }
#pragma unroll
    for (int h = 0; h < PPT / 2; ++h) reinterpret_cast<double2*>(d2)[p * (PPT / 2) + h] = make_double2(out[2 * h], out[2 * h + 1]);
  }
}

static_assert(SBA_RESECT_MOM_COUNT <= 64 && SBA_RESECT_MOM_COUNT <= JOINT_ROW && SBA_RESECT_SIZE <= JOINT_ROW, "one wave publishes a row");

template <typename ST>
const void* reduce_kernel_of(bool loss) {
  return loss ? reinterpret_cast<const void*>(resect_reduce_kernel<ST, true>) : reinterpret_cast<const void*>(resect_reduce_kernel<ST, false>);
}

}  // namespace

hipError_t resect_blocks_per_cu(int store, bool loss, int* blocks) {
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks, store == 0 ? reduce_kernel_of<double>(loss) : reduce_kernel_of<float>(loss), 256, 0);
}

hipError_t launch_resect_reduce(int store, const Planes& pl, const ResectParams& prm, double* partials, int grid, double* out,
                                double* host_out, unsigned long long seq, hipStream_t stream) {
  if (grid > 0) {
    const bool loss = prm.delta > 0.0;
    if (store == 0 && loss) hipLaunchKernelGGL((resect_reduce_kernel<double, true>), dim3(grid), dim3(256), 0, stream, pl, prm, partials);
    else if (store == 0) hipLaunchKernelGGL((resect_reduce_kernel<double, false>), dim3(grid), dim3(256), 0, stream, pl, prm, partials);
    else if (loss) hipLaunchKernelGGL((resect_reduce_kernel<float, true>), dim3(grid), dim3(256), 0, stream, pl, prm, partials);
    else hipLaunchKernelGGL((resect_reduce_kernel<float, false>), dim3(grid), dim3(256), 0, stream, pl, prm, partials);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return launch_joint_finalize(partials, grid, SBA_RESECT_COUNT, -1, out, host_out, seq, stream);
}

hipError_t launch_resect_moments(int store, const Planes& pl, size_t n, double* partials, int grid, double* out, double* host_out,
                                 unsigned long long seq, hipStream_t stream) {
  if (grid > 0) {
    const unsigned long long nn = n;
    if (store == 0) hipLaunchKernelGGL(resect_moments_kernel<double>, dim3(grid), dim3(256), 0, stream, pl, nn, partials);
    else hipLaunchKernelGGL(resect_moments_kernel<float>, dim3(grid), dim3(256), 0, stream, pl, nn, partials);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return launch_joint_finalize(partials, grid, SBA_RESECT_MOM_COUNT, -1, out, host_out, seq, stream);
}

hipError_t launch_resect_depths(int store, const Planes& pl, const ResectParams& prm, double* d2, int grid, hipStream_t stream) {
  if (grid <= 0) return hipSuccess;
  if (store == 0) hipLaunchKernelGGL(resect_depths_kernel<double>, dim3(grid), dim3(256), 0, stream, pl, prm, d2);
  else hipLaunchKernelGGL(resect_depths_kernel<float>, dim3(grid), dim3(256), 0, stream, pl, prm, d2);
  return hipGetLastError();
}

}  // namespace sba
