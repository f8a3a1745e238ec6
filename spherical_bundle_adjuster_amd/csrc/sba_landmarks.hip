// The landmark map on the device (algebra and per-observation code: sba_landmarks.hpp, whose landmark_fuse_one is the very
// function the kernels call).  Storage: nine f64 planes X.x X.y X.z S.xx S.yy S.zz S.xy S.xz S.yz of `elems` doubles each in one
// allocation, then one u32 plane of accepted observations; elems = n rounded up to a whole 16-byte vector, zeros beyond n.
//   landmarks_pack_kernel      caller rows [n][3] + [n][6] -> the planes, cov_scale applied, counts zeroed, padding zeroed
//   landmarks_unpack_kernel    the planes -> caller rows, exactly n of each
//   landmarks_fuse_kernel<INDEXED, APPLY>   sba_landmarks_pass.inc around landmark_fuse_one: the dense and the indexed form and
//                                           what APPLY = false leaves out are described there
// All: 256-thread blocks, grid-stride, plain stores.  The pose, its covariance terms and the scalars are one by-value
// argument (scalar registers).  No floating-point reduction anywhere: the bytes do not depend on the grid.
// Bytes per landmark, dense: 72 + 4 (planes, count) + 24 (bearing) read, up to 72 + 4 + 8 written.
// The plane accessors, the non-temporal load, the register block and the class counts: sba_landmarks_device.hpp (lm::).
#include "sba_device.hpp"
#include "sba_landmarks.hpp"
#include "sba_landmarks_device.hpp"

namespace sba {
namespace {

__global__ __launch_bounds__(256) void landmarks_pack_kernel(const double* __restrict__ xyz, const double* __restrict__ cov, unsigned long long n,
                                                             double cov_scale, double* __restrict__ base, unsigned long long elems) {
  const size_t nvec = elems / 2, stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (size_t p = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; p < nvec; p += stride) {
    double v[2][9];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int k = 0; k < 9; ++k) v[h][k] = 0.0;
    if (2 * p + 1 < n) {          // both rows exist: 48 + 96 contiguous bytes, 16-byte aligned
      const double2* xv = reinterpret_cast<const double2*>(xyz) + 3 * p;
      const double2* cv = reinterpret_cast<const double2*>(cov) + 6 * p;
      const double2 x0 = lm::load_nt(xv), x1 = lm::load_nt(xv + 1), x2 = lm::load_nt(xv + 2);
      v[0][0] = x0.x; v[0][1] = x0.y; v[0][2] = x1.x; v[1][0] = x1.y; v[1][1] = x2.x; v[1][2] = x2.y;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double2 a = lm::load_nt(cv + k), b = lm::load_nt(cv + 3 + k);
        v[0][3 + 2 * k] = a.x; v[0][4 + 2 * k] = a.y; v[1][3 + 2 * k] = b.x; v[1][4 + 2 * k] = b.y;
      }
    } else if (2 * p < n) {       // the last row of an odd n: nothing is read beyond the caller's rows
#pragma unroll
      for (int k = 0; k < 3; ++k) v[0][k] = xyz[6 * p + k];
#pragma unroll
      for (int k = 0; k < 6; ++k) v[0][3 + k] = cov[12 * p + k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) lm::plane(base, elems, k)[p] = make_double2(v[0][k], v[1][k]);
#pragma unroll
    for (int k = 3; k < 9; ++k) lm::plane(base, elems, k)[p] = make_double2(cov_scale * v[0][k], cov_scale * v[1][k]);
    reinterpret_cast<uint2*>(lm::counts(base, elems))[p] = make_uint2(0u, 0u);
  }
}

__global__ __launch_bounds__(256) void landmarks_unpack_kernel(double* __restrict__ base, unsigned long long elems, unsigned long long n,
                                                               double* __restrict__ xyz, double* __restrict__ cov) {
  const size_t nvec = (n + 1) / 2, stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (size_t p = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; p < nvec; p += stride) {
    double2 v[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) v[k] = lm::plane(base, elems, k)[p];
    const bool both = 2 * p + 1 < n;
    if (xyz) {
      if (both) {
        double2* xv = reinterpret_cast<double2*>(xyz) + 3 * p;
        xv[0] = make_double2(v[0].x, v[1].x); xv[1] = make_double2(v[2].x, v[0].y); xv[2] = make_double2(v[1].y, v[2].y);
      } else {
        xyz[6 * p] = v[0].x; xyz[6 * p + 1] = v[1].x; xyz[6 * p + 2] = v[2].x;
      }
    }
    if (cov) {
      if (both) {
        double2* cv = reinterpret_cast<double2*>(cov) + 6 * p;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          cv[k] = make_double2(v[3 + 2 * k].x, v[4 + 2 * k].x);
          cv[3 + k] = make_double2(v[3 + 2 * k].y, v[4 + 2 * k].y);
        }
      } else {
#pragma unroll
        for (int k = 0; k < 6; ++k) cov[12 * p + k] = v[3 + k].x;
      }
    }
  }
}

template <bool INDEXED, bool APPLY>
__global__ __launch_bounds__(256) void landmarks_fuse_kernel(LandmarkFuseParams P, double* __restrict__ base, unsigned long long elems,
                                                             const long long* __restrict__ idx, const double* __restrict__ bearings,
                                                             double* __restrict__ chi2, unsigned long long* __restrict__ counters) {
  constexpr bool NOISE = false;
  const double* noise = nullptr;          // no noise plane: never read
#define SBA_LANDMARK_PASS_ONE(X, Sg, y, nz, Xo, So, chi2) landmark_fuse_one(P, X, Sg, y, Xo, So, chi2)
#include "sba_landmarks_pass.inc"
#undef SBA_LANDMARK_PASS_ONE
}

const void* fuse_kernel_of(bool indexed, bool apply) {
  if (indexed) return apply ? reinterpret_cast<const void*>(landmarks_fuse_kernel<true, true>) : reinterpret_cast<const void*>(landmarks_fuse_kernel<true, false>);
  return apply ? reinterpret_cast<const void*>(landmarks_fuse_kernel<false, true>) : reinterpret_cast<const void*>(landmarks_fuse_kernel<false, false>);
}

}  // namespace

hipError_t landmarks_fuse_blocks_per_cu(bool indexed, bool apply, int* blocks) {
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks, fuse_kernel_of(indexed, apply), 256, 0);
}

hipError_t landmarks_pack_blocks_per_cu(bool unpack, int* blocks) {
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(
      blocks, unpack ? reinterpret_cast<const void*>(landmarks_unpack_kernel) : reinterpret_cast<const void*>(landmarks_pack_kernel), 256, 0);
}

hipError_t launch_landmarks_pack(const double* xyz, const double* cov, size_t n, double cov_scale, const LandmarkPlanes& pl, int grid,
                                 hipStream_t stream) {
  if (grid <= 0) return hipSuccess;
  hipLaunchKernelGGL(landmarks_pack_kernel, dim3(grid), dim3(256), 0, stream, xyz, cov, static_cast<unsigned long long>(n), cov_scale, pl.base,
                     static_cast<unsigned long long>(pl.elems));
  return hipGetLastError();
}

hipError_t launch_landmarks_unpack(const LandmarkPlanes& pl, size_t n, double* xyz, double* cov, int grid, hipStream_t stream) {
  if (grid <= 0) return hipSuccess;
  hipLaunchKernelGGL(landmarks_unpack_kernel, dim3(grid), dim3(256), 0, stream, pl.base, static_cast<unsigned long long>(pl.elems),
                     static_cast<unsigned long long>(n), xyz, cov);
  return hipGetLastError();
}

hipError_t launch_landmarks_fuse(const LandmarkPlanes& pl, const LandmarkFuseParams& prm, const long long* idx, const double* bearings,
                                 double* chi2, unsigned long long* counters, bool apply, int grid, hipStream_t stream) {
  const hipError_t e = hipMemsetAsync(counters, 0, LANDMARK_CLASSES * sizeof(unsigned long long), stream);
  if (e != hipSuccess || grid <= 0) return e;
  const unsigned long long elems = pl.elems;
  if (idx && apply) hipLaunchKernelGGL((landmarks_fuse_kernel<true, true>), dim3(grid), dim3(256), 0, stream, prm, pl.base, elems, idx, bearings, chi2, counters);
  else if (idx) hipLaunchKernelGGL((landmarks_fuse_kernel<true, false>), dim3(grid), dim3(256), 0, stream, prm, pl.base, elems, idx, bearings, chi2, counters);
  else if (apply) hipLaunchKernelGGL((landmarks_fuse_kernel<false, true>), dim3(grid), dim3(256), 0, stream, prm, pl.base, elems, idx, bearings, chi2, counters);
  else hipLaunchKernelGGL((landmarks_fuse_kernel<false, false>), dim3(grid), dim3(256), 0, stream, prm, pl.base, elems, idx, bearings, chi2, counters);
  return hipGetLastError();
}

}  // namespace sba
