// Edits of the landmark map on the device (the score, the classes of a prune and the checks: sba_landmarks_edit.hpp, whose
// landmark_score and landmark_prune_class are the very functions the kernels call).  Storage as in sba_landmarks.hip: nine f64
// planes of `elems` doubles in one allocation, then one u32 plane of counts; elems = n rounded up to even, zeros beyond n.
//   landmarks_scores_kernel           lane p owns landmarks 2 p and 2 p + 1: nine 16-byte plane loads, one 16-byte store
//   landmarks_keep_kernel             the same nine loads plus the two counts and two mask bytes; two keep bytes per lane, whole
//                                     tiles of kCompactTile bytes, zero beyond n; five class counts, flushed over the
//                                     kLandmarkCounterRows counter rows that the host sums
//   landmarks_compact_scatter_kernel  block b = tile b: rank within the tile by ballot and mbcnt, per-wave prefixes in LDS (as
//                                     compact_scatter_kernel of sba_select.hip); the ten planes of a kept landmark go to
//                                     tile_offset + rank of ANOTHER allocation (in place a tile's destinations lie in the source
//                                     range of earlier tiles, which may not have been read yet), its old index to kept_index
//   landmarks_append_kernel           lane p owns rows 2 p and 2 p + 1 of the new layout: an old row with its count, a caller's
//                                     row with cov_scale applied and count 0, or zero padding; 16-byte stores
//   landmarks_gather_kernel           lane j owns output row j and reads landmark idx[j] (sorted: neighbouring lanes,
//                                     neighbouring lines)
// All: 256-thread blocks, plain stores; grid-stride except the scatter (one block per tile).  No floating-point reduction
// anywhere: the bytes do not depend on the grid.
// Bytes per landmark: keep 72 + 4 (+ 1 mask) read, 1 written; scatter 1 + 76 read and 76 + 8 written per kept landmark.
// The plane accessors, the two-landmark register block and the class counts: sba_landmarks_device.hpp (lm::).
#include "sba_device.hpp"
#include "sba_landmarks_device.hpp"
#include "sba_landmarks_edit.hpp"

namespace sba {
namespace {

__global__ __launch_bounds__(256) void landmarks_scores_kernel(double* __restrict__ base, unsigned long long elems, double* __restrict__ out) {
  const size_t nvec = elems / 2, stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (size_t p = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; p < nvec; p += stride) {
    lm::PairRegs<false> cur;
    double X[2][3], S[2][6];
    cur.load_planes(base, elems, p);
    cur.landmark(0, X[0], S[0]);
    cur.landmark(1, X[1], S[1]);
    reinterpret_cast<double2*>(out)[p] = make_double2(landmark_score(X[0], S[0]), landmark_score(X[1], S[1]));
  }
}

// The loop runs over the lane pairs of whole tiles, a multiple of 64: every lane of a wave takes part in each ballot, and lane 0
// of a wave took part in every step any lane of its wave took part in.
__global__ __launch_bounds__(256) void landmarks_keep_kernel(double* __restrict__ base, unsigned long long elems, unsigned long long n,
                                                             double max_score, unsigned int min_count, const unsigned char* __restrict__ mask,
                                                             unsigned char* __restrict__ keep, unsigned long long tile_pairs,
                                                             unsigned long long* __restrict__ counters) {
  const size_t nvec = elems / 2, stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  lm::ClassCounts<LANDMARK_PRUNE_CLASSES> cc;
  cc.init();
  for (size_t p = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; p < tile_pairs; p += stride) {
    int cls[2] = {LANDMARK_INVALID, LANDMARK_INVALID};
    const bool valid[2] = {2 * p < n, 2 * p + 1 < n};
    if (p < nvec) {
      lm::PairRegs<false> cur;
      double X[2][3], S[2][6];
      cur.load_planes(base, elems, p);
      const uint2 c = reinterpret_cast<const uint2*>(lm::counts(base, elems))[p];
      const unsigned short mb = mask ? reinterpret_cast<const unsigned short*>(mask)[p] : static_cast<unsigned short>(0x0101u);
      cur.landmark(0, X[0], S[0]);
      cur.landmark(1, X[1], S[1]);
      cls[0] = landmark_prune_class(X[0], S[0], c.x, static_cast<unsigned char>(mb & 0xffu), max_score, min_count);
      cls[1] = landmark_prune_class(X[1], S[1], c.y, static_cast<unsigned char>(mb >> 8), max_score, min_count);
    }
    const unsigned k0 = valid[0] && cls[0] == LANDMARK_KEPT ? 1u : 0u, k1 = valid[1] && cls[1] == LANDMARK_KEPT ? 1u : 0u;
    reinterpret_cast<unsigned short*>(keep)[p] = static_cast<unsigned short>(k0 | (k1 << 8));
    cc.add(valid[0], cls[0]);
    cc.add(valid[1], cls[1]);
  }
  cc.flush_rows(counters);
}

// Block b = tile b.  Round r: thread t looks at landmark b * kCompactTile + r * 256 + t; a kept one goes to tile_offset[b] + (kept
// earlier in the tile) -- earlier rounds, earlier waves of this round, lower lanes of this wave.  The per-wave counts alternate
// between two LDS rows, so one barrier per round suffices.  dst == null: kept_index only (a dry run).
__global__ __launch_bounds__(256) void landmarks_compact_scatter_kernel(const unsigned char* __restrict__ keep, unsigned long long n,
                                                                        const unsigned long long* __restrict__ tile_offset,
                                                                        const double* __restrict__ src, unsigned long long src_elems,
                                                                        double* __restrict__ dst, unsigned long long dst_elems,
                                                                        unsigned long long n_kept, long long* __restrict__ kept_index) {
  __shared__ unsigned int wave_cnt[2][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t tile0 = static_cast<size_t>(blockIdx.x) * kCompactTile;
  unsigned long long pos0 = tile_offset[blockIdx.x];
  // the padding row of an odd kept count: no kept landmark lands there
  if (dst && blockIdx.x == 0 && threadIdx.x < 10 && (n_kept & 1ull)) {
    if (threadIdx.x < 9) dst[static_cast<size_t>(threadIdx.x) * dst_elems + n_kept] = 0.0;
    else lm::counts(dst, dst_elems)[n_kept] = 0u;
  }
  for (int r = 0; r < kCompactTile / 256; ++r) {
    const size_t i = tile0 + static_cast<size_t>(r) * 256 + threadIdx.x;
    const bool k = i < n && keep[i] != 0;
    const unsigned long long m = __ballot(k);
    const unsigned rank = __builtin_amdgcn_mbcnt_hi(static_cast<unsigned>(m >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<unsigned>(m), 0u));
    if (lane == 0) wave_cnt[r & 1][wave] = static_cast<unsigned>(__popcll(m));
    __syncthreads();
    unsigned before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const unsigned c = wave_cnt[r & 1][w];
      before += w < wave ? c : 0u;
      all += c;
    }
    if (k) {
      const size_t o = pos0 + before + rank;
      if (dst) {
#pragma unroll
        for (int c = 0; c < 9; ++c) dst[static_cast<size_t>(c) * dst_elems + o] = src[static_cast<size_t>(c) * src_elems + i];
        lm::counts(dst, dst_elems)[o] = lm::counts(src, src_elems)[i];
      }
      if (kept_index) kept_index[o] = static_cast<long long>(i);
    }
    pos0 += all;
  }
}

__global__ __launch_bounds__(256) void landmarks_append_kernel(const double* __restrict__ src, unsigned long long src_elems,
                                                               unsigned long long n_old, const double* __restrict__ xyz,
                                                               const double* __restrict__ cov, unsigned long long n_add, double cov_scale,
                                                               double* __restrict__ dst, unsigned long long dst_elems) {
  const size_t nvec = dst_elems / 2, n_new = n_old + n_add, stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (size_t p = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; p < nvec; p += stride) {
    double v[2][9];
    unsigned int cnt[2] = {0u, 0u};
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int k = 0; k < 9; ++k) v[h][k] = 0.0;
    if (2 * p + 1 < n_old) {                 // two old rows: p lies within the old planes
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        const double2 a = lm::plane(src, src_elems, k)[p];
        v[0][k] = a.x; v[1][k] = a.y;
      }
      const uint2 c = reinterpret_cast<const uint2*>(lm::counts(src, src_elems))[p];
      cnt[0] = c.x; cnt[1] = c.y;
    } else if (2 * p >= n_old && 2 * p + 1 < n_new && (n_old & 1ull) == 0) {
      // two new rows of an even old size: 48 + 96 contiguous bytes, 16-byte aligned as the caller's rows are
      const size_t q = p - n_old / 2;
      const double2* xv = reinterpret_cast<const double2*>(xyz) + 3 * q;
      const double2* cv = reinterpret_cast<const double2*>(cov) + 6 * q;
      const double2 x0 = lm::load_nt(xv), x1 = lm::load_nt(xv + 1), x2 = lm::load_nt(xv + 2);
      v[0][0] = x0.x; v[0][1] = x0.y; v[0][2] = x1.x; v[1][0] = x1.y; v[1][1] = x2.x; v[1][2] = x2.y;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double2 a = lm::load_nt(cv + k), b = lm::load_nt(cv + 3 + k);
        v[0][3 + 2 * k] = cov_scale * a.x; v[0][4 + 2 * k] = cov_scale * a.y;
        v[1][3 + 2 * k] = cov_scale * b.x; v[1][4 + 2 * k] = cov_scale * b.y;
      }
    } else {                                 // row by row: the seam of an odd old size, the last row, the padding
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const size_t i = 2 * p + h;
        if (i < n_old) {
#pragma unroll
          for (int k = 0; k < 9; ++k) v[h][k] = src[static_cast<size_t>(k) * src_elems + i];
          cnt[h] = lm::counts(src, src_elems)[i];
        } else if (i < n_new) {
          const size_t j = i - n_old;
#pragma unroll
          for (int k = 0; k < 3; ++k) v[h][k] = xyz[3 * j + k];
#pragma unroll
          for (int k = 0; k < 6; ++k) v[h][3 + k] = cov_scale * cov[6 * j + k];
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) lm::plane(dst, dst_elems, k)[p] = make_double2(v[0][k], v[1][k]);
    reinterpret_cast<uint2*>(lm::counts(dst, dst_elems))[p] = make_uint2(cnt[0], cnt[1]);
  }
}

__global__ __launch_bounds__(256) void landmarks_gather_kernel(const double* __restrict__ base, unsigned long long elems,
                                                               const long long* __restrict__ idx, unsigned long long m,
                                                               double* __restrict__ xyz, double* __restrict__ cov,
                                                               unsigned int* __restrict__ counts) {
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (size_t j = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; j < m; j += stride) {
    const size_t i = static_cast<size_t>(idx[j]);          // < n: validated on the host
    if (xyz) {
#pragma unroll
      for (int k = 0; k < 3; ++k) xyz[3 * j + k] = base[static_cast<size_t>(k) * elems + i];
    }
    if (cov) {
#pragma unroll
      for (int k = 0; k < 6; ++k) cov[6 * j + k] = base[static_cast<size_t>(3 + k) * elems + i];
    }
    if (counts) counts[j] = lm::counts(base, elems)[i];
  }
}

}  // namespace

hipError_t landmarks_edit_blocks_per_cu(int which, int* blocks) {
  const void* f = which == LANDMARK_EDIT_SCORES  ? reinterpret_cast<const void*>(landmarks_scores_kernel)
                  : which == LANDMARK_EDIT_KEEP  ? reinterpret_cast<const void*>(landmarks_keep_kernel)
                  : which == LANDMARK_EDIT_APPEND ? reinterpret_cast<const void*>(landmarks_append_kernel)
                                                  : reinterpret_cast<const void*>(landmarks_gather_kernel);
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks, f, 256, 0);
}

hipError_t launch_landmarks_scores(const LandmarkPlanes& pl, double* out, int grid, hipStream_t stream) {
  if (grid <= 0) return hipSuccess;
  hipLaunchKernelGGL(landmarks_scores_kernel, dim3(grid), dim3(256), 0, stream, pl.base, static_cast<unsigned long long>(pl.elems), out);
  return hipGetLastError();
}

hipError_t launch_landmarks_keep(const LandmarkPlanes& pl, size_t n, double max_score, unsigned int min_count, const unsigned char* mask,
                                 unsigned char* keep, size_t ntiles, unsigned long long* counters, int grid, hipStream_t stream) {
  static_assert(LANDMARK_PRUNE_CLASSES <= kLandmarkCounterStride, "a row holds the five class counts");
  const hipError_t e = hipMemsetAsync(counters, 0, kLandmarkCounterRows * kLandmarkCounterStride * sizeof(unsigned long long), stream);
  if (e != hipSuccess || grid <= 0) return e;
  static_assert(kCompactTile % 128 == 0, "the lane pairs of whole tiles are whole waves");
  hipLaunchKernelGGL(landmarks_keep_kernel, dim3(grid), dim3(256), 0, stream, pl.base, static_cast<unsigned long long>(pl.elems),
                     static_cast<unsigned long long>(n), max_score, min_count, mask, keep,
                     static_cast<unsigned long long>(ntiles) * (kCompactTile / 2), counters);
  return hipGetLastError();
}

hipError_t launch_landmarks_compact_scatter(const unsigned char* keep, size_t n, const unsigned long long* tile_offset, size_t ntiles,
                                            const LandmarkPlanes& src, const LandmarkPlanes& dst, size_t n_kept, long long* kept_index,
                                            hipStream_t stream) {
  if (ntiles == 0) return hipSuccess;
  hipLaunchKernelGGL(landmarks_compact_scatter_kernel, dim3(static_cast<unsigned>(ntiles)), dim3(256), 0, stream, keep,
                     static_cast<unsigned long long>(n), tile_offset, src.base, static_cast<unsigned long long>(src.elems), dst.base,
                     static_cast<unsigned long long>(dst.elems), static_cast<unsigned long long>(n_kept), kept_index);
  return hipGetLastError();
}

hipError_t launch_landmarks_append(const LandmarkPlanes& src, size_t n_old, const double* xyz, const double* cov, size_t n_add,
                                   double cov_scale, const LandmarkPlanes& dst, int grid, hipStream_t stream) {
  if (grid <= 0) return hipSuccess;
  hipLaunchKernelGGL(landmarks_append_kernel, dim3(grid), dim3(256), 0, stream, src.base, static_cast<unsigned long long>(src.elems),
                     static_cast<unsigned long long>(n_old), xyz, cov, static_cast<unsigned long long>(n_add), cov_scale, dst.base,
                     static_cast<unsigned long long>(dst.elems));
  return hipGetLastError();
}

hipError_t launch_landmarks_gather(const LandmarkPlanes& pl, const long long* idx, size_t m, double* xyz, double* cov, unsigned int* counts,
                                   int grid, hipStream_t stream) {
  if (grid <= 0) return hipSuccess;
  hipLaunchKernelGGL(landmarks_gather_kernel, dim3(grid), dim3(256), 0, stream, pl.base, static_cast<unsigned long long>(pl.elems), idx,
                     static_cast<unsigned long long>(m), xyz, cov, counts);
  return hipGetLastError();
}

}  // namespace sba
