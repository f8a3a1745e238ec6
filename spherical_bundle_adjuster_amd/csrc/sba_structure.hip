// Triangulated landmarks of the joint solve on the device (algebra: sba_structure.hpp): per match the midpoint X of the two ray
// ends, its 3 x 3 covariance and the score trace / X.X.  One streaming pass in the form of the covariance's depth pass
// (sba_covariance.hip): 256-thread blocks, grid-stride over 16-byte vectors (two matches per lane), the next step's loads in
// registers; per match the undamped block of joint_block(), the degeneracy rule of cov_block(), then structure_block().
// No reduction, no atomics: every value depends on its own match, the pose and Sigma_c alone, so the bits are the same for
// every grid.  Sigma_c and the pass parameters come from device memory and are staged in LDS by the prologue.
// Bytes per match (f64 planes): reads 64; writes 24 (xyz), 48 (cov: xx, yy, zz, xy, xz, yz), 8 (score) -- only the outputs
// the instantiation was compiled for.  The per-match loop is sba_structure_loop.inc.
#include "sba_covariance.hpp"
#include "sba_device.hpp"
#include "sba_joint_core.hpp"
#include "sba_structure.hpp"

namespace sba {
namespace {

static_assert(sizeof(StructureParams) % sizeof(double) == 0, "StructureParams is staged word by word");

// xyz [n][3], cov [n][6], score [n]: 16-byte aligned, exactly n rows are written (the padding match of an odd-sized problem
// is not stored: the destinations may be a caller's arrays).
template <typename ST, bool WANT_XYZ, bool WANT_COV, bool WANT_SCORE>
__global__ __launch_bounds__(256) void structure_kernel(Planes pl, const double* __restrict__ d1, const double* __restrict__ d2,
                                                        const StructureParams* __restrict__ params, double* __restrict__ xyz,
                                                        double* __restrict__ cov, double* __restrict__ score) {
  __shared__ StructureParams sp;
  {
    const double* src = reinterpret_cast<const double*>(params);
    double* dst = reinterpret_cast<double*>(&sp);
    for (unsigned k = threadIdx.x; k < sizeof(StructureParams) / sizeof(double); k += blockDim.x) dst[k] = src[k];
  }
  __syncthreads();
  const JointParams& P = sp.prm;
  const double min_sin2 = sp.min_sin2;
  const double* sigma_c = sp.sigma_c;
  const size_t n = P.cur.n, npairs = (n + 1) / 2, stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  size_t pr = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  const IdentityMap map;
  const auto store = [xyz, cov, score](size_t p, bool both, const double (&X)[2][3], const double (&cv)[2][6], const double (&q)[2]) {
    if (WANT_XYZ) {
      joint_store_pair(xyz, 3 * p, X[0][0], X[0][1]);
      if (both) {
        joint_store_pair(xyz, 3 * p + 1, X[0][2], X[1][0]);
        joint_store_pair(xyz, 3 * p + 2, X[1][1], X[1][2]);
      } else {
        xyz[6 * p + 2] = X[0][2];
      }
    }
    if (WANT_COV) {
#pragma unroll
      for (int k = 0; k < 3; ++k) joint_store_pair(cov, 6 * p + k, cv[0][2 * k], cv[0][2 * k + 1]);
      if (both) {
#pragma unroll
        for (int k = 0; k < 3; ++k) joint_store_pair(cov, 6 * p + 3 + k, cv[1][2 * k], cv[1][2 * k + 1]);
      }
    }
    if (WANT_SCORE) {
      if (both) joint_store_pair(score, p, q[0], q[1]);
      else score[2 * p] = q[0];
    }
  };
#include "sba_structure_loop.inc"
}

template <typename ST>
void launch_for(int which, int grid, hipStream_t stream, const Planes& pl, const double* d1, const double* d2,
                const StructureParams* params, double* xyz, double* cov, double* score) {
#define SBA_STRUCTURE_CASE(W, X, C, S)                                                                                    \
  case W: hipLaunchKernelGGL((structure_kernel<ST, X, C, S>), dim3(grid), dim3(256), 0, stream, pl, d1, d2, params, xyz, cov, score); break;
  switch (which) {
    SBA_STRUCTURE_CASE(1, true, false, false)
    SBA_STRUCTURE_CASE(2, false, true, false)
    SBA_STRUCTURE_CASE(3, true, true, false)
    SBA_STRUCTURE_CASE(4, false, false, true)
    SBA_STRUCTURE_CASE(5, true, false, true)
    SBA_STRUCTURE_CASE(6, false, true, true)
    SBA_STRUCTURE_CASE(7, true, true, true)
    default: break;
  }
#undef SBA_STRUCTURE_CASE
}

}  // namespace

hipError_t structure_blocks_per_cu(int store, int* blocks) {
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(
      blocks, reinterpret_cast<const void*>(store == 0 ? structure_kernel<double, true, true, true> : structure_kernel<float, true, true, true>),
      256, 0);
}

hipError_t launch_structure(int store, const Planes& pl, const double* d1, const double* d2, const StructureParams* params_dev,
                            double* xyz, double* cov, double* score, int grid, hipStream_t stream) {
  const int which = (xyz ? 1 : 0) | (cov ? 2 : 0) | (score ? 4 : 0);
  if (grid <= 0 || which == 0) return hipSuccess;
  if (store == 0) launch_for<double>(which, grid, stream, pl, d1, d2, params_dev, xyz, cov, score);
  else launch_for<float>(which, grid, stream, pl, d1, d2, params_dev, xyz, cov, score);
  return hipGetLastError();
}

}  // namespace sba
