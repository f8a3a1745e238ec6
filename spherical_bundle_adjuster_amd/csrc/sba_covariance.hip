// Covariance of the joint solve on the device (algebra and host finish: sba_covariance.hpp).  Two streaming passes in the
// form of the joint solve's kernels (sba_joint.hip): 256-thread blocks, grid-stride over 16-byte vectors (two matches per
// lane), the next step's loads in registers, DPP wave sums + LDS fold to one row per block, rows folded in a fixed order.
// No atomics: bit-identical run to run.
//   cov_reduce_kernel  per match the undamped block of joint_block() (first pass, inv_radius = 0), the degeneracy rule,
//                      S = sum (w F^T F - W^T U^-1 W), cost, sum w, used and degenerate counts: 25 accumulators, so -- unlike
//                      joint_reduce_kernel's 52 -- two resident blocks per CU
//   cov_depth_kernel   given Sigma_c (kernel argument): the same block from the same inputs, T = U^-1 W,
//                      Sigma_dd,i = s (U^-1 + T Sigma_c T^T) s, three doubles per match
// Bytes per match (f64 planes): reduce reads 64; depth reads 64 and writes 24.
// The two per-match loops are sba_cov_reduce_loop.inc / sba_cov_depth_loop.inc, the one text this file and the batched form
// (sba_batch_covariance.hip) both expand in their kernels' bodies.
#include "sba_covariance.hpp"
#include "sba_device.hpp"
#include "sba_joint_core.hpp"

namespace sba {
namespace {

struct CovSigma { double c[36]; };

template <typename ST>
__global__ __launch_bounds__(256, 2) void cov_reduce_kernel(Planes pl, const double* __restrict__ d1, const double* __restrict__ d2,
                                                           JointParams P, double min_sin2, double* __restrict__ partials) {
  __shared__ double red[4][COV_OUT_COUNT];
  const size_t n = P.cur.n, npairs = (n + 1) / 2, stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  size_t pr = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  double acc[COV_OUT_COUNT];
#pragma unroll
  for (int k = 0; k < COV_OUT_COUNT; ++k) acc[k] = 0.0;
  const IdentityMap map;
#include "sba_cov_reduce_loop.inc"
  joint_block_fold<COV_OUT_COUNT, -1>(acc, red, partials + static_cast<size_t>(blockIdx.x) * COV_ROW);
}

// out: [npairs][6] doubles = three doubles per match, the padding match of an odd-sized problem included.
template <typename ST>
__global__ __launch_bounds__(256, 2) void cov_depth_kernel(Planes pl, const double* __restrict__ d1, const double* __restrict__ d2,
                                                          JointParams P, double min_sin2, CovSigma sigma, double* __restrict__ out) {
  const size_t n = P.cur.n, npairs = (n + 1) / 2, stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  size_t pr = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  const IdentityMap map;
  const double* sigma_c = sigma.c;
  const auto store = [out](size_t p, const double (&o)[2][3]) {
    joint_store_pair(out, 3 * p, o[0][0], o[0][1]);
    joint_store_pair(out, 3 * p + 1, o[0][2], o[1][0]);
    joint_store_pair(out, 3 * p + 2, o[1][1], o[1][2]);
  };
#include "sba_cov_depth_loop.inc"
}

// [nblocks][COV_ROW] -> out[COV_OUT_COUNT]: every slot folded in a fixed order (one wave per slot at a time: lane l takes
// rows l, l + 64, ..., then a butterfly).
__global__ __launch_bounds__(1024) void cov_finalize_kernel(const double* __restrict__ partials, int nblocks, double* __restrict__ out) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int slot = wave; slot < COV_OUT_COUNT; slot += 16) {
    double v = 0.0;
    for (int b = lane; b < nblocks; b += 64) v += partials[static_cast<size_t>(b) * COV_ROW + slot];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if (lane == 0) out[slot] = v;
  }
}
static_assert(COV_OUT_COUNT <= COV_ROW, "a block's row holds every slot");

}  // namespace

hipError_t cov_blocks_per_cu(int store, int* blocks) {
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(
      blocks, reinterpret_cast<const void*>(store == 0 ? cov_reduce_kernel<double> : cov_reduce_kernel<float>), 256, 0);
}

hipError_t launch_cov_reduce(int store, const Planes& pl, const double* d1, const double* d2, const JointParams& prm,
                             double min_sin2, double* partials, int grid, double* out, hipStream_t stream) {
  if (grid > 0) {
    if (store == 0) hipLaunchKernelGGL(cov_reduce_kernel<double>, dim3(grid), dim3(256), 0, stream, pl, d1, d2, prm, min_sin2, partials);
    else hipLaunchKernelGGL(cov_reduce_kernel<float>, dim3(grid), dim3(256), 0, stream, pl, d1, d2, prm, min_sin2, partials);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(cov_finalize_kernel, dim3(1), dim3(1024), 0, stream, partials, grid, out);
  return hipGetLastError();
}

hipError_t launch_cov_depth(int store, const Planes& pl, const double* d1, const double* d2, const JointParams& prm,
                            double min_sin2, const double sigma_c[36], double* out, int grid, hipStream_t stream) {
  if (grid <= 0) return hipSuccess;
  CovSigma sg;
  for (int k = 0; k < 36; ++k) sg.c[k] = sigma_c[k];
  if (store == 0) hipLaunchKernelGGL(cov_depth_kernel<double>, dim3(grid), dim3(256), 0, stream, pl, d1, d2, prm, min_sin2, sg, out);
  else hipLaunchKernelGGL(cov_depth_kernel<float>, dim3(grid), dim3(256), 0, stream, pl, d1, d2, prm, min_sin2, sg, out);
  return hipGetLastError();
}

}  // namespace sba
