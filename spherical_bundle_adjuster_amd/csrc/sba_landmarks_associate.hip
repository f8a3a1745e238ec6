// The landmark map's descriptor rows and the association of a frame with the map on the device (the claim key, its order and the
// checks: sba_landmarks_associate.hpp, whose associate_key / associate_within are the very functions the kernels call).  Rows are
// packed f32: row i = dim floats at desc + i * dim, next to the planes of sba_landmarks.hip.
//   landmarks_desc_compact_scatter_kernel  block b = tile b of a prune: the ranks of landmarks_compact_scatter_kernel from the same
//                                          keep bytes and tile offsets (ballot and mbcnt, per-wave prefixes in LDS), kept in LDS;
//                                          then every wave moves whole rows, a lane one 16-byte piece, 64 / (dim / 4) rows per step
//                                          (dim not a multiple of 4: one float per lane, a row per step)
//   landmarks_desc_gather_kernel           a wave per step of 64 / (dim / 4) output rows in the same shape; row j reads row idx[j]
//   landmarks_claim_kernel                 lane k owns match k of the matcher's compacted list: one 64-bit integer atomic min of its
//                                          key into its landmark's slot; the accepted rows counted by ballot and population count
//   landmarks_associate_keep_kernel        keep byte per landmark: its slot was claimed; whole tiles, zero beyond n
//   landmarks_associate_scatter_kernel     block b = tile b: rank by ballot and mbcnt as above; a claimed landmark writes its index,
//                                          the two halves of its key and the winner's bearing to output tile_offset + rank
// All: 256-thread blocks, plain stores; grid-stride except the two scatters (one block per tile).  The only atomics are integer
// ones (a minimum and a count): the bytes depend neither on the grid nor on the order in which the lanes arrive.
#include "sba_device.hpp"
#include "sba_landmarks_associate.hpp"

namespace sba {
namespace {

constexpr unsigned int kNoRow = 0xffffffffu;        // in LDS: a dropped landmark
constexpr size_t kNotMoved = ~static_cast<size_t>(0);  // what dst_row answers for it

// Rank of the kept items of a tile, round r of 256: `before` = kept in earlier waves of this round, `all` = kept in this round.
// The per-wave counts alternate between two LDS rows, so one barrier per round suffices (landmarks_compact_scatter_kernel).
__device__ __forceinline__ unsigned tile_round_rank(bool k, int r, int lane, int wave, unsigned int (*wave_cnt)[4], unsigned* all) {
  const unsigned long long m = __ballot(k);
  const unsigned rank = __builtin_amdgcn_mbcnt_hi(static_cast<unsigned>(m >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<unsigned>(m), 0u));
  if (lane == 0) wave_cnt[r & 1][wave] = static_cast<unsigned>(__popcll(m));
  __syncthreads();
  unsigned before = 0, sum = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const unsigned c = wave_cnt[r & 1][w];
    before += w < wave ? c : 0u;
    sum += c;
  }
  *all = sum;
  return before + rank;
}

// One wave moves `rows` rows, row q from src_row(q) to dst_row(q) (kNotMoved: not moved): a lane one 16-byte piece when dim is a
// multiple of 4 (the rows then start 16-byte aligned), 64 / (dim / 4) rows per step; otherwise one float per lane, a row per step.
template <typename SrcRow, typename DstRow>
__device__ __forceinline__ void wave_move_rows(const float* __restrict__ src, float* __restrict__ dst, int dim, size_t first, size_t rows,
                                               size_t step_waves, int lane, SrcRow src_row, DstRow dst_row) {
  if ((dim & 3) == 0) {
    const int vpr = dim / 4, rpp = 64 / vpr, sub = lane / vpr, v = lane - sub * vpr;
    for (size_t q0 = first * rpp; q0 < rows; q0 += step_waves * rpp) {
      const size_t q = q0 + sub;
      if (sub >= rpp || q >= rows) continue;
      const size_t d = dst_row(q);
      if (d == kNotMoved) continue;
      reinterpret_cast<float4*>(dst + d * dim)[v] = reinterpret_cast<const float4*>(src + src_row(q) * dim)[v];
    }
  } else {
    for (size_t q = first; q < rows; q += step_waves) {
      const size_t d = dst_row(q);
      if (d == kNotMoved) continue;
      const float* s = src + src_row(q) * dim;
      float* t = dst + d * dim;
      for (int k = lane; k < dim; k += 64) t[k] = s[k];
    }
  }
}

__global__ __launch_bounds__(256) void landmarks_desc_compact_scatter_kernel(const unsigned char* __restrict__ keep, unsigned long long n,
                                                                             const unsigned long long* __restrict__ tile_offset,
                                                                             const float* __restrict__ src, float* __restrict__ dst, int dim) {
  __shared__ unsigned int wave_cnt[2][4];
  __shared__ unsigned int s_dest[kCompactTile];       // rank within the tile, kNoRow for a dropped landmark
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t tile0 = static_cast<size_t>(blockIdx.x) * kCompactTile;
  unsigned pos = 0;
  for (int r = 0; r < kCompactTile / 256; ++r) {
    const size_t i = tile0 + static_cast<size_t>(r) * 256 + threadIdx.x;
    const bool k = i < n && keep[i] != 0;
    unsigned all = 0;
    const unsigned rank = tile_round_rank(k, r, lane, wave, wave_cnt, &all);
    s_dest[r * 256 + threadIdx.x] = k ? pos + rank : kNoRow;
    pos += all;
  }
  __syncthreads();
  const size_t base = tile_offset[blockIdx.x];
  wave_move_rows(src, dst, dim, static_cast<size_t>(wave), static_cast<size_t>(kCompactTile), 4, lane,
                 [&](size_t q) { return tile0 + q; },
                 [&](size_t q) { const unsigned d = s_dest[q]; return d == kNoRow ? kNotMoved : base + d; });
}

__global__ __launch_bounds__(256) void landmarks_desc_gather_kernel(const float* __restrict__ desc, int dim, const long long* __restrict__ idx,
                                                                    unsigned long long m, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const size_t wave = (static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6, waves = static_cast<size_t>(gridDim.x) * (blockDim.x >> 6);
  wave_move_rows(desc, out, dim, wave, static_cast<size_t>(m), waves, lane,
                 [&](size_t q) { return static_cast<size_t>(idx[q]); },          // < n: validated on the host
                 [&](size_t q) { return q; });
}

// The loop runs over whole waves: every lane of a wave takes part in each ballot.
__global__ __launch_bounds__(256) void landmarks_claim_kernel(const int* __restrict__ match_row, const int* __restrict__ match_landmark,
                                                              const float* __restrict__ match_dist, unsigned long long n_matches,
                                                              float max_distance, unsigned long long* __restrict__ slots,
                                                              unsigned long long* __restrict__ counters) {
  const size_t whole = (n_matches + 63) / 64 * 64, stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  unsigned long long accepted = 0;
  for (size_t k = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; k < whole; k += stride) {
    bool ok = false;
    if (k < n_matches) {
      const float d0 = match_dist[k];
      ok = associate_within(d0, max_distance);
      if (ok) atomicMin(&slots[match_landmark[k]], associate_key(d0, static_cast<unsigned int>(match_row[k])));
    }
    accepted += static_cast<unsigned long long>(__popcll(__ballot(ok)));
  }
  if ((threadIdx.x & 63) == 0 && accepted) atomicAdd(&counters[0], accepted);
}

__global__ __launch_bounds__(256) void landmarks_associate_keep_kernel(const unsigned long long* __restrict__ slots, unsigned long long n,
                                                                       unsigned char* __restrict__ keep, unsigned long long tile_items) {
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < tile_items; i += stride)
    keep[i] = i < n && slots[i] != kAssociateUnclaimed ? 1 : 0;
}

__global__ __launch_bounds__(256) void landmarks_associate_scatter_kernel(const unsigned char* __restrict__ keep, unsigned long long n,
                                                                          const unsigned long long* __restrict__ tile_offset,
                                                                          const unsigned long long* __restrict__ slots,
                                                                          const double* __restrict__ frame_bearings, long long* __restrict__ idx_out,
                                                                          int* __restrict__ row_out, float* __restrict__ dist_out,
                                                                          double* __restrict__ bearings_out) {
  __shared__ unsigned int wave_cnt[2][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t tile0 = static_cast<size_t>(blockIdx.x) * kCompactTile;
  unsigned long long pos0 = tile_offset[blockIdx.x];
  for (int r = 0; r < kCompactTile / 256; ++r) {
    const size_t i = tile0 + static_cast<size_t>(r) * 256 + threadIdx.x;
    const bool k = i < n && keep[i] != 0;
    unsigned all = 0;
    const unsigned rank = tile_round_rank(k, r, lane, wave, wave_cnt, &all);
    if (k) {
      const size_t o = pos0 + rank;
      const unsigned long long key = slots[i];
      const size_t row = associate_key_row(key);
      idx_out[o] = static_cast<long long>(i);
      row_out[o] = static_cast<int>(row);
      dist_out[o] = associate_key_distance(key);
      if (bearings_out) {
#pragma unroll
        for (int c = 0; c < 3; ++c) bearings_out[3 * o + c] = frame_bearings[3 * row + c];
      }
    }
    pos0 += all;
  }
}

}  // namespace

hipError_t landmarks_associate_blocks_per_cu(int which, int* blocks) {
  const void* f = which == LANDMARK_ASSOC_CLAIM  ? reinterpret_cast<const void*>(landmarks_claim_kernel)
                  : which == LANDMARK_ASSOC_KEEP ? reinterpret_cast<const void*>(landmarks_associate_keep_kernel)
                                                 : reinterpret_cast<const void*>(landmarks_desc_gather_kernel);
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks, f, 256, 0);
}

hipError_t launch_landmarks_desc_compact_scatter(const unsigned char* keep, size_t n, const unsigned long long* tile_offset, size_t ntiles,
                                                 const float* src, float* dst, int dim, hipStream_t stream) {
  if (ntiles == 0) return hipSuccess;
  hipLaunchKernelGGL(landmarks_desc_compact_scatter_kernel, dim3(static_cast<unsigned>(ntiles)), dim3(256), 0, stream, keep,
                     static_cast<unsigned long long>(n), tile_offset, src, dst, dim);
  return hipGetLastError();
}

hipError_t launch_landmarks_desc_gather(const float* desc, int dim, const long long* idx, size_t m, float* out, int grid, hipStream_t stream) {
  if (grid <= 0) return hipSuccess;
  hipLaunchKernelGGL(landmarks_desc_gather_kernel, dim3(grid), dim3(256), 0, stream, desc, dim, idx, static_cast<unsigned long long>(m), out);
  return hipGetLastError();
}

hipError_t launch_landmarks_claim(const int* match_row, const int* match_landmark, const float* match_dist, size_t n_matches, float max_distance,
                                  unsigned long long* slots, unsigned long long* counters, int grid, hipStream_t stream) {
  if (grid <= 0) return hipSuccess;
  hipLaunchKernelGGL(landmarks_claim_kernel, dim3(grid), dim3(256), 0, stream, match_row, match_landmark, match_dist,
                     static_cast<unsigned long long>(n_matches), max_distance, slots, counters);
  return hipGetLastError();
}

hipError_t launch_landmarks_associate_keep(const unsigned long long* slots, size_t n, unsigned char* keep, size_t ntiles, int grid,
                                           hipStream_t stream) {
  if (grid <= 0) return hipSuccess;
  hipLaunchKernelGGL(landmarks_associate_keep_kernel, dim3(grid), dim3(256), 0, stream, slots, static_cast<unsigned long long>(n), keep,
                     static_cast<unsigned long long>(ntiles) * kCompactTile);
  return hipGetLastError();
}

hipError_t launch_landmarks_associate_scatter(const unsigned char* keep, size_t n, const unsigned long long* tile_offset, size_t ntiles,
                                              const unsigned long long* slots, const double* frame_bearings, long long* idx_out, int* row_out,
                                              float* dist_out, double* bearings_out, hipStream_t stream) {
  if (ntiles == 0) return hipSuccess;
  hipLaunchKernelGGL(landmarks_associate_scatter_kernel, dim3(static_cast<unsigned>(ntiles)), dim3(256), 0, stream, keep,
                     static_cast<unsigned long long>(n), tile_offset, slots, frame_bearings, idx_out, row_out, dist_out,
                     frame_bearings ? bearings_out : nullptr);
  return hipGetLastError();
}

}  // namespace sba
