// Kernels either side of the sweep: AoS -> plane re-layout at upload time, pixel -> unit sphere (reference
// spherical_bundle_adjuster.cpp:271-298), and their launchers.  (The image / key-point maps live in sba_maps.hip.)
#include <algorithm>

#include "sba_device.hpp"
#include "sba_match.hpp"

namespace sba {
namespace {

// ---- layout conversion at upload time (once per problem, not per LM iteration) ---------------
template <typename ST>
__global__ void aos_to_planes_kernel(const double* __restrict__ aos, size_t n, size_t first,
                                     ST* __restrict__ px, ST* __restrict__ py, ST* __restrict__ pz, size_t tile_elems,
                                     size_t tile_stride_elems) {
  const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const size_t o = tiled_index(first, i, tile_elems, tile_stride_elems);
  px[o] = static_cast<ST>(aos[3 * i + 0]);
  py[o] = static_cast<ST>(aos[3 * i + 1]);
  pz[o] = static_cast<ST>(aos[3 * i + 2]);
}
__global__ void d12_to_planes_kernel(const double* __restrict__ d12, size_t n, size_t first,
                                     double* __restrict__ d1, double* __restrict__ d2, size_t tile_elems, size_t tile_stride_elems) {
  const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double2 d = reinterpret_cast<const double2*>(d12)[i];
  const size_t o = tiled_index(first, i, tile_elems, tile_stride_elems);
  d1[o] = d.x;
  d2[o] = d.y;
}
// The same re-layout for a whole batch in one launch: rows [first_row, first_row + m) of the caller's CONCATENATED arrays
// (pair g = rows offsets[g] .. offsets[g + 1]) sit in `stage`; every row goes to its place in the pair's tiles
// (batch_row_index, sba_device.hpp).  One launch per staged chunk instead of one per pair.
template <typename ST>
__global__ void batch_aos_to_planes_kernel(const double* __restrict__ aos, size_t m, size_t first_row,
                                           const unsigned long long* __restrict__ offsets, int num_pairs,
                                           const PairDesc* __restrict__ desc, size_t ppt, ST* __restrict__ px,
                                           ST* __restrict__ py, ST* __restrict__ pz) {
  const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const size_t o = batch_row_index(first_row + i, offsets, num_pairs, desc, ppt);
  px[o] = static_cast<ST>(aos[3 * i + 0]);
  py[o] = static_cast<ST>(aos[3 * i + 1]);
  pz[o] = static_cast<ST>(aos[3 * i + 2]);
}
__global__ void batch_d12_to_planes_kernel(const double* __restrict__ d12, size_t m, size_t first_row,
                                           const unsigned long long* __restrict__ offsets, int num_pairs,
                                           const PairDesc* __restrict__ desc, size_t ppt, double* __restrict__ d1,
                                           double* __restrict__ d2) {
  const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const double2 d = reinterpret_cast<const double2*>(d12)[i];
  const size_t o = batch_row_index(first_row + i, offsets, num_pairs, desc, ppt);
  d1[o] = d.x;
  d2[o] = d.y;
}
__global__ void planes_to_d12_kernel(const double* __restrict__ d1, const double* __restrict__ d2,
                                     size_t n, double* __restrict__ d12) {
  const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  reinterpret_cast<double2*>(d12)[i] = make_double2(d1[i], d2[i]);
}

// ---- pixel -> unit sphere (reference spherical_bundle_adjuster.cpp:271-298) ---------------------
//   lon = 2 pi (pt.x / W), colat = pi (pt.y / H);  v = (sin colat cos lon, sin colat sin lon, cos colat)
// pt.x / pt.y are the first two floats of each `stride_bytes`-byte key-point record.
__global__ void keypoints_to_sphere_kernel(const uint8_t* __restrict__ kp, size_t n, size_t stride_bytes,
                                           double im_w, double im_h, double* __restrict__ out_xyz) {
  const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* rec = reinterpret_cast<const float*>(kp + i * stride_bytes);
  const double px = static_cast<double>(rec[0]), py = static_cast<double>(rec[1]);
  const double kPi = 3.14159265358979323846;
  const double lon = 2 * kPi * (px / im_w);
  const double colat = kPi * (py / im_h);
  const double sc = sin(colat), cc = cos(colat);
  out_xyz[3 * i + 0] = sc * cos(lon);
  out_xyz[3 * i + 1] = sc * sin(lon);
  out_xyz[3 * i + 2] = cc;
}

// Same map, fused with the upload: key-point records of BOTH images -> the six coordinate planes of a problem
// (no host-side cv::Point3d arrays in between).
template <typename ST>
__global__ void keypoints_to_planes_kernel(const uint8_t* __restrict__ kp_left, const uint8_t* __restrict__ kp_right,
                                           size_t n, size_t stride_bytes, double im_w, double im_h,
                                           ST* __restrict__ x1x, ST* __restrict__ x1y, ST* __restrict__ x1z,
                                           ST* __restrict__ x2x, ST* __restrict__ x2y, ST* __restrict__ x2z) {
  const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double kPi = 3.14159265358979323846;
  const float* l = reinterpret_cast<const float*>(kp_left + i * stride_bytes);
  const float* r = reinterpret_cast<const float*>(kp_right + i * stride_bytes);
  const double lon1 = 2 * kPi * (static_cast<double>(l[0]) / im_w), col1 = kPi * (static_cast<double>(l[1]) / im_h);
  const double lon2 = 2 * kPi * (static_cast<double>(r[0]) / im_w), col2 = kPi * (static_cast<double>(r[1]) / im_h);
  const double s1 = sin(col1), s2 = sin(col2);
  x1x[i] = static_cast<ST>(s1 * cos(lon1)); x1y[i] = static_cast<ST>(s1 * sin(lon1)); x1z[i] = static_cast<ST>(cos(col1));
  x2x[i] = static_cast<ST>(s2 * cos(lon2)); x2y[i] = static_cast<ST>(s2 * sin(lon2)); x2z[i] = static_cast<ST>(cos(col2));
}

// The two maps above with an index indirection: record i is the one at absolute row rows[i] (the key-point gather of a
// descriptor match, sba_match.cpp).  The same expressions, compiled under the same flags, so the planes / points carry the
// bits of the direct maps applied to the gathered records.
template <typename ST>
__global__ void keypoints_to_planes_gather_kernel(const uint8_t* __restrict__ kp_left, const uint8_t* __restrict__ kp_right,
                                                  const unsigned long long* __restrict__ rows_left,
                                                  const unsigned long long* __restrict__ rows_right, size_t n,
                                                  size_t stride_bytes, double im_w, double im_h, ST* __restrict__ x1x,
                                                  ST* __restrict__ x1y, ST* __restrict__ x1z, ST* __restrict__ x2x,
                                                  ST* __restrict__ x2y, ST* __restrict__ x2z) {
  const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double kPi = 3.14159265358979323846;
  const float* l = reinterpret_cast<const float*>(kp_left + rows_left[i] * stride_bytes);
  const float* r = reinterpret_cast<const float*>(kp_right + rows_right[i] * stride_bytes);
  const double lon1 = 2 * kPi * (static_cast<double>(l[0]) / im_w), col1 = kPi * (static_cast<double>(l[1]) / im_h);
  const double lon2 = 2 * kPi * (static_cast<double>(r[0]) / im_w), col2 = kPi * (static_cast<double>(r[1]) / im_h);
  const double s1 = sin(col1), s2 = sin(col2);
  x1x[i] = static_cast<ST>(s1 * cos(lon1)); x1y[i] = static_cast<ST>(s1 * sin(lon1)); x1z[i] = static_cast<ST>(cos(col1));
  x2x[i] = static_cast<ST>(s2 * cos(lon2)); x2y[i] = static_cast<ST>(s2 * sin(lon2)); x2z[i] = static_cast<ST>(cos(col2));
}
__global__ void keypoints_to_sphere_gather_kernel(const uint8_t* __restrict__ kp, const unsigned long long* __restrict__ rows,
                                                  size_t n, size_t stride_bytes, double im_w, double im_h,
                                                  double* __restrict__ out_xyz) {
  const size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* rec = reinterpret_cast<const float*>(kp + rows[i] * stride_bytes);
  const double px = static_cast<double>(rec[0]), py = static_cast<double>(rec[1]);
  const double kPi = 3.14159265358979323846;
  const double lon = 2 * kPi * (px / im_w);
  const double colat = kPi * (py / im_h);
  const double sc = sin(colat), cc = cos(colat);
  out_xyz[3 * i + 0] = sc * cos(lon);
  out_xyz[3 * i + 1] = sc * sin(lon);
  out_xyz[3 * i + 2] = cc;
}

// Per-match depths folded into the coordinates: X1 = d1 x1, X2 = d2 x2 (the rounded products the per-match sweep forms,
// sba_sweep_core.hpp: accumulate), 16 B per lane per plane over the whole allocation -- the zero padding of the raw planes
// becomes the zero padding of the folded ones.
struct FoldPlanes {
  const double* x[6];
  const double* d[2];
  double* X[6];
};
__global__ __launch_bounds__(256) void fold_depths_kernel(FoldPlanes f, size_t nvec) {
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < nvec; i += stride) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const double2 d = reinterpret_cast<const double2*>(f.d[s])[i];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double2 c = reinterpret_cast<const double2*>(f.x[3 * s + k])[i];
        reinterpret_cast<double2*>(f.X[3 * s + k])[i] = make_double2(d.x * c.x, d.y * c.y);
      }
    }
  }
}

}  // namespace

hipError_t launch_fold_depths(const void* const coord[6], const double* d1, const double* d2, double* const folded[6],
                              size_t elems, int grid_cap, hipStream_t stream) {
  const size_t nvec = elems / 2;
  if (nvec == 0) return hipSuccess;
  FoldPlanes f;
  for (int k = 0; k < 6; ++k) { f.x[k] = static_cast<const double*>(coord[k]); f.X[k] = folded[k]; }
  f.d[0] = d1; f.d[1] = d2;
  const unsigned grid = static_cast<unsigned>(std::min<size_t>((nvec + 255) / 256, static_cast<size_t>(std::max(grid_cap, 1))));
  hipLaunchKernelGGL(fold_depths_kernel, dim3(grid), dim3(256), 0, stream, f, nvec);
  return hipGetLastError();
}

hipError_t launch_aos_to_planes(const double* aos, size_t n, size_t first, void* px, void* py,
                                void* pz, int store, hipStream_t stream, size_t tile_elems, size_t tile_stride_elems) {
  if (n == 0) return hipSuccess;
  const unsigned grid = static_cast<unsigned>((n + 255) / 256);
  if (store == 0)
    hipLaunchKernelGGL((aos_to_planes_kernel<double>), dim3(grid), dim3(256), 0, stream, aos, n, first,
                       static_cast<double*>(px), static_cast<double*>(py), static_cast<double*>(pz), tile_elems, tile_stride_elems);
  else
    hipLaunchKernelGGL((aos_to_planes_kernel<float>), dim3(grid), dim3(256), 0, stream, aos, n, first,
                       static_cast<float*>(px), static_cast<float*>(py), static_cast<float*>(pz), tile_elems, tile_stride_elems);
  return hipGetLastError();
}

hipError_t launch_d12_to_planes(const double* d12, size_t n, size_t first, double* d1, double* d2,
                                hipStream_t stream, size_t tile_elems, size_t tile_stride_elems) {
  if (n == 0) return hipSuccess;
  const unsigned grid = static_cast<unsigned>((n + 255) / 256);
  hipLaunchKernelGGL(d12_to_planes_kernel, dim3(grid), dim3(256), 0, stream, d12, n, first, d1, d2, tile_elems, tile_stride_elems);
  return hipGetLastError();
}

hipError_t launch_batch_aos_to_planes(const double* aos, size_t m, size_t first_row, const unsigned long long* offsets_dev,
                                      int num_pairs, const PairDesc* desc, size_t ppt, void* px, void* py, void* pz, int store,
                                      hipStream_t stream) {
  if (m == 0 || num_pairs <= 0) return hipSuccess;
  const unsigned grid = static_cast<unsigned>((m + 255) / 256);
  if (store == 0)
    hipLaunchKernelGGL((batch_aos_to_planes_kernel<double>), dim3(grid), dim3(256), 0, stream, aos, m, first_row, offsets_dev,
                       num_pairs, desc, ppt, static_cast<double*>(px), static_cast<double*>(py), static_cast<double*>(pz));
  else
    hipLaunchKernelGGL((batch_aos_to_planes_kernel<float>), dim3(grid), dim3(256), 0, stream, aos, m, first_row, offsets_dev,
                       num_pairs, desc, ppt, static_cast<float*>(px), static_cast<float*>(py), static_cast<float*>(pz));
  return hipGetLastError();
}

hipError_t launch_batch_d12_to_planes(const double* d12, size_t m, size_t first_row, const unsigned long long* offsets_dev,
                                      int num_pairs, const PairDesc* desc, size_t ppt, double* d1, double* d2,
                                      hipStream_t stream) {
  if (m == 0 || num_pairs <= 0) return hipSuccess;
  const unsigned grid = static_cast<unsigned>((m + 255) / 256);
  hipLaunchKernelGGL(batch_d12_to_planes_kernel, dim3(grid), dim3(256), 0, stream, d12, m, first_row, offsets_dev, num_pairs, desc,
                     ppt, d1, d2);
  return hipGetLastError();
}

hipError_t launch_planes_to_d12(const double* d1, const double* d2, size_t n, double* d12,
                                hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const unsigned grid = static_cast<unsigned>((n + 255) / 256);
  hipLaunchKernelGGL(planes_to_d12_kernel, dim3(grid), dim3(256), 0, stream, d1, d2, n, d12);
  return hipGetLastError();
}

hipError_t launch_keypoints_to_sphere(const uint8_t* kp, size_t n, size_t stride_bytes, double im_w,
                                      double im_h, double* out_xyz, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const unsigned grid = static_cast<unsigned>((n + 255) / 256);
  hipLaunchKernelGGL(keypoints_to_sphere_kernel, dim3(grid), dim3(256), 0, stream, kp, n, stride_bytes,
                     im_w, im_h, out_xyz);
  return hipGetLastError();
}

hipError_t launch_keypoints_to_planes(const uint8_t* kp_left, const uint8_t* kp_right, size_t n, size_t stride_bytes,
                                      double im_w, double im_h, void* const planes[6], int store, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const unsigned grid = static_cast<unsigned>((n + 255) / 256);
  if (store == 0)
    hipLaunchKernelGGL((keypoints_to_planes_kernel<double>), dim3(grid), dim3(256), 0, stream, kp_left, kp_right, n,
                       stride_bytes, im_w, im_h, static_cast<double*>(planes[0]), static_cast<double*>(planes[1]),
                       static_cast<double*>(planes[2]), static_cast<double*>(planes[3]), static_cast<double*>(planes[4]),
                       static_cast<double*>(planes[5]));
  else
    hipLaunchKernelGGL((keypoints_to_planes_kernel<float>), dim3(grid), dim3(256), 0, stream, kp_left, kp_right, n,
                       stride_bytes, im_w, im_h, static_cast<float*>(planes[0]), static_cast<float*>(planes[1]),
                       static_cast<float*>(planes[2]), static_cast<float*>(planes[3]), static_cast<float*>(planes[4]),
                       static_cast<float*>(planes[5]));
  return hipGetLastError();
}

hipError_t launch_keypoints_to_planes_gather(const uint8_t* kp_left, const uint8_t* kp_right, const unsigned long long* rows_left,
                                             const unsigned long long* rows_right, size_t n, size_t stride_bytes, double im_w,
                                             double im_h, void* const planes[6], int store, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const unsigned grid = static_cast<unsigned>((n + 255) / 256);
  if (store == 0)
    hipLaunchKernelGGL((keypoints_to_planes_gather_kernel<double>), dim3(grid), dim3(256), 0, stream, kp_left, kp_right, rows_left,
                       rows_right, n, stride_bytes, im_w, im_h, static_cast<double*>(planes[0]), static_cast<double*>(planes[1]),
                       static_cast<double*>(planes[2]), static_cast<double*>(planes[3]), static_cast<double*>(planes[4]),
                       static_cast<double*>(planes[5]));
  else
    hipLaunchKernelGGL((keypoints_to_planes_gather_kernel<float>), dim3(grid), dim3(256), 0, stream, kp_left, kp_right, rows_left,
                       rows_right, n, stride_bytes, im_w, im_h, static_cast<float*>(planes[0]), static_cast<float*>(planes[1]),
                       static_cast<float*>(planes[2]), static_cast<float*>(planes[3]), static_cast<float*>(planes[4]),
                       static_cast<float*>(planes[5]));
  return hipGetLastError();
}

hipError_t launch_keypoints_to_sphere_gather(const uint8_t* kp, const unsigned long long* rows, size_t n, size_t stride_bytes,
                                             double im_w, double im_h, double* out_xyz, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  const unsigned grid = static_cast<unsigned>((n + 255) / 256);
  hipLaunchKernelGGL(keypoints_to_sphere_gather_kernel, dim3(grid), dim3(256), 0, stream, kp, rows, n, stride_bytes, im_w, im_h,
                     out_xyz);
  return hipGetLastError();
}

}  // namespace sba
