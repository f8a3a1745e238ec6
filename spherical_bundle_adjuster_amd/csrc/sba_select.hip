// Per-match residuals and stable compaction of a single problem's matches (sba_problem_residuals,
// sba_problem_compact; host side in sba_select.cpp).
//
// residual_kernel: e = d2 x2 - d1 R x1 + t for every match, formed by the sweep's own residual() (sba_sweep_core.hpp), so
// e, s = e.e and the inlier flag !(s > delta^2) carry the same bits the sweep accumulates.  Grid-stride over the same
// 16-byte VecRegs loads as the sweep (register double buffer); the outputs that were asked for (template flags) go out
// with plain vector stores; the inlier count is a per-wave __ballot + popcount, folded per block and added to one 64-bit
// word with an integer atomic (exact, order-free).
//
// Compaction, no atomics, same result on every run: compact_count_kernel counts the kept matches of each tile of
// kCompactTile matches, compact_scan_kernel turns the counts into exclusive tile offsets (one block), and
// compact_scatter_kernel moves every kept match to its tile offset plus its rank in the tile (wave __ballot +
// mbcnt, per-wave prefixes through LDS), plane by plane, and records its original index.
//
// The same for a batch (sba_batch_residuals / _compact / _keep_inliers; host side in sba_batch_select.cpp):
// batch_residual_kernel walks every pair's vectors as the batched sweep does (block group g = pair g, PairDesc) with the
// pair's SweepParams built on the device from its BatchState, and writes element by element to the pair's rows.  The
// compaction runs the tile count and scan above over the concatenated rows, batch_pair_kept_kernel reads every pair's
// kept count off the tile offsets, and batch_compact_scatter_kernel moves each kept row from its element of the old
// pair layout to its element of the new one.
#include <algorithm>

#include "sba_sweep_core.hpp"

namespace sba {
namespace {

constexpr int kOutE = 1, kOutSq = 2, kOutInlier = 4;

template <int DEPTH, typename ST, int OUT>
__global__ __launch_bounds__(kBlock) void residual_kernel(Planes pl, SweepParams prm, ResidualOut out) {
  constexpr int PPT = Lanes<ST>::PPT;
  __shared__ unsigned long long wave_count[kBlock / 64];
  const SweepParams* P = &prm;
  const bool loss = prm.delta > 0.0;
  const size_t n = prm.n;
  const size_t nvec = (n + PPT - 1) / PPT;   // the last vector may be ragged: the planes are zero-padded beyond it
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t stride = static_cast<size_t>(gridDim.x) * kBlock;
  // The loop runs per wave (base is wave-uniform), so every lane of the wave takes part in each ballot.
  size_t base = static_cast<size_t>(blockIdx.x) * kBlock + static_cast<size_t>(wave) * 64;
  unsigned long long count = 0;   // wave-uniform
  VecRegs<ST, DEPTH> cur, nxt;
  if (base + lane < nvec) cur.load(pl, base + lane);
  for (; base < nvec; base += stride) {
    const size_t p = base + lane;
    const size_t pn = p + stride;
    if (pn < nvec) nxt.load(pl, pn);
    double E[3 * PPT], S[PPT];
    unsigned char in[PPT];
#pragma unroll
    for (int h = 0; h < PPT; ++h) {
      double x = cur.coord(0, h), y = cur.coord(1, h), z = cur.coord(2, h);
      double u = cur.coord(3, h), v = cur.coord(4, h), q = cur.coord(5, h);
      double r0, r1, r2, e0, e1, e2;
      residual<DEPTH>(P, x, y, z, u, v, q, DEPTH == DEPTH_PER_MATCH ? cur.depth1(h) : 1.0,
                      DEPTH == DEPTH_PER_MATCH ? cur.depth2(h) : 0.0, r0, r1, r2, e0, e1, e2);
      const double s = sq_norm(e0, e1, e2);
      // the sweep's outlier test (huber(): s > delta2); a NaN s is no outlier there, so it is an inlier here
      const bool inl = !loss || !(s > P->delta2);
      E[3 * h] = e0; E[3 * h + 1] = e1; E[3 * h + 2] = e2;
      S[h] = s;
      in[h] = inl ? 1 : 0;
      count += __popcll(__ballot(p < nvec && p * PPT + h < n && inl));
    }
    if (p < nvec) {   // whole vectors: the scratch holds nvec * PPT elements
      if (OUT & kOutE) {
        double2* dst = reinterpret_cast<double2*>(out.e) + p * (3 * PPT / 2);
#pragma unroll
        for (int k = 0; k < 3 * PPT / 2; ++k) dst[k] = make_double2(E[2 * k], E[2 * k + 1]);
      }
      if (OUT & kOutSq) {
        double2* dst = reinterpret_cast<double2*>(out.sq) + p * (PPT / 2);
#pragma unroll
        for (int k = 0; k < PPT / 2; ++k) dst[k] = make_double2(S[2 * k], S[2 * k + 1]);
      }
      if (OUT & kOutInlier) {
        if constexpr (PPT == 2) {
          reinterpret_cast<unsigned short*>(out.inlier)[p] = static_cast<unsigned short>(in[0] | (in[1] << 8));
        } else {
          reinterpret_cast<unsigned int*>(out.inlier)[p] =
              static_cast<unsigned int>(in[0]) | (static_cast<unsigned int>(in[1]) << 8) |
              (static_cast<unsigned int>(in[2]) << 16) | (static_cast<unsigned int>(in[3]) << 24);
        }
      }
    }
    cur = nxt;
  }
  if (lane == 0) wave_count[wave] = count;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long c = 0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) c += wave_count[w];
    if (c) atomicAdd(out.n_inlier, c);
  }
}

template <int DEPTH, typename ST>
hipError_t launch_residuals_outputs(int outputs, const Planes& pl, const SweepParams& prm, const ResidualOut& out, int grid,
                                    hipStream_t stream) {
  switch (outputs & 7) {
#define SBA_RESIDUAL_CASE(F) \
    case F: hipLaunchKernelGGL((residual_kernel<DEPTH, ST, F>), dim3(grid), dim3(kBlock), 0, stream, pl, prm, out); break;
    SBA_RESIDUAL_CASE(0) SBA_RESIDUAL_CASE(1) SBA_RESIDUAL_CASE(2) SBA_RESIDUAL_CASE(3)
    SBA_RESIDUAL_CASE(4) SBA_RESIDUAL_CASE(5) SBA_RESIDUAL_CASE(6) SBA_RESIDUAL_CASE(7)
#undef SBA_RESIDUAL_CASE
  }
  return hipGetLastError();
}

// ---- compaction -------------------------------------------------------------------------------------------------------
constexpr int kCompactRounds = kCompactTile / 256;   // matches per thread and tile, one per round

__device__ __forceinline__ unsigned nonzero_bytes(unsigned w) {
  return ((w & 0xffu) != 0) + ((w & 0xff00u) != 0) + ((w & 0xff0000u) != 0) + ((w & 0xff000000u) != 0);
}

// tile_count[b] = kept matches of tile b.  keep holds whole tiles (zero beyond n): each thread reads 8 bytes.
__global__ __launch_bounds__(256) void compact_count_kernel(const unsigned char* __restrict__ keep,
                                                            unsigned int* __restrict__ tile_count) {
  static_assert(kCompactTile == 256 * 8, "one 8-byte word per thread and tile");
  __shared__ unsigned int wave_sum[4];
  const uint2 w = reinterpret_cast<const uint2*>(keep + static_cast<size_t>(blockIdx.x) * kCompactTile)[threadIdx.x];
  unsigned c = nonzero_bytes(w.x) + nonzero_bytes(w.y);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off);
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) tile_count[blockIdx.x] = wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
}

// Exclusive scan of ntiles counts in one block: every thread sums a contiguous range of tiles, the 1024 range sums are
// scanned in LDS (Hillis-Steele), then every thread writes the offsets of its own range.  total[0] = the sum.
__global__ __launch_bounds__(1024) void compact_scan_kernel(const unsigned int* __restrict__ tile_count, size_t ntiles,
                                                            unsigned long long* __restrict__ tile_offset,
                                                            unsigned long long* __restrict__ total) {
  __shared__ unsigned long long buf[2][1024];
  const int t = threadIdx.x;
  const size_t per = (ntiles + 1023) / 1024;
  const size_t lo = std::min(ntiles, per * t), hi = std::min(ntiles, lo + per);
  unsigned long long s = 0;
  for (size_t k = lo; k < hi; ++k) s += tile_count[k];
  int src = 0;
  buf[0][t] = s;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    const unsigned long long v = buf[src][t] + (t >= off ? buf[src][t - off] : 0ull);
    buf[src ^ 1][t] = v;
    src ^= 1;
    __syncthreads();
  }
  const unsigned long long incl = buf[src][t];
  unsigned long long o = incl - s;
  for (size_t k = lo; k < hi; ++k) { tile_offset[k] = o; o += tile_count[k]; }
  if (t == 1023) total[0] = incl;
}

// Block b = tile b.  Round r: thread t looks at match b * kCompactTile + r * 256 + t; a kept match goes to
// tile_offset[b] + (kept earlier in the tile) -- earlier rounds, earlier waves of this round, lower lanes of this wave.
// The per-wave counts alternate between two LDS rows, so one barrier per round suffices.
template <typename ST>
__global__ __launch_bounds__(256) void compact_scatter_kernel(CompactArgs a) {
  __shared__ unsigned int wave_cnt[2][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t tile0 = static_cast<size_t>(blockIdx.x) * kCompactTile;
  unsigned long long pos0 = a.tile_offset[blockIdx.x];
  for (int r = 0; r < kCompactRounds; ++r) {
    const size_t i = tile0 + static_cast<size_t>(r) * 256 + threadIdx.x;
    const bool k = i < a.n && a.keep[i] != 0;
    const unsigned long long m = __ballot(k);
    const unsigned rank = __builtin_amdgcn_mbcnt_hi(static_cast<unsigned>(m >> 32),
                                                    __builtin_amdgcn_mbcnt_lo(static_cast<unsigned>(m), 0u));
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
#pragma unroll
      for (int c = 0; c < 6; ++c) static_cast<ST*>(a.dst[c])[o] = static_cast<const ST*>(a.src[c])[i];
      if (a.src[6]) {
        static_cast<double*>(a.dst[6])[o] = static_cast<const double*>(a.src[6])[i];
        static_cast<double*>(a.dst[7])[o] = static_cast<const double*>(a.src[7])[i];
      }
      if (a.kept_index) a.kept_index[o] = static_cast<long long>(i);
    }
    pos0 += all;
  }
}

// ---- batches ----------------------------------------------------------------------------------------------------------
// Block group g = blockIdx.x / bpp takes pair g; block j of the group visits the pair's logical vectors j * 256 + tid,
// stepping by bpp * 256 (sweep_share_rows, sba_batch_kernels.hip).  Thread 0 builds the pair's SweepParams from its
// BatchState in LDS with the step kernels' device fill_sweep_params, so e and s carry the bits the batched sweep forms.
// Rows of consecutive pairs are adjacent and a pair's first row has any alignment: every element is stored on its own,
// only if it is one of the pair's n.  The loop bound is block-uniform, so every lane of a wave takes part in each ballot.
template <int DEPTH, typename ST, int OUT>
__global__ __launch_bounds__(kBlock) void batch_residual_kernel(Planes pl, const PairDesc* __restrict__ desc,
                                                                const unsigned long long* __restrict__ offsets,
                                                                const BatchState* __restrict__ state, double huber_delta,
                                                                int bpp, ResidualOut out) {
  constexpr int PPT = Lanes<ST>::PPT;
  __shared__ SweepParams prm_s;
  __shared__ unsigned long long wave_count[kBlock / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned pair = blockIdx.x / static_cast<unsigned>(bpp), j = blockIdx.x % static_cast<unsigned>(bpp);
  const PairDesc dsc = desc[pair];
  if (tid == 0) {
    const BatchState st = state[pair];
    fill_sweep_params(st.n, DEPTH, st.rot, st.tran, st.d1, st.d2, huber_delta, &prm_s, false);
  }
  __syncthreads();
  const SweepParams prm = prm_s;
  const SweepParams* P = &prm;
  const bool loss = prm.delta > 0.0;
  const size_t n = prm.n < dsc.n ? prm.n : dsc.n;     // never past the pair's own vectors
  const size_t nvec = (n + PPT - 1) / PPT;          // the last vector may be ragged: zero padding beyond it
  const size_t row0 = offsets[pair];
  const size_t stride = static_cast<size_t>(bpp) * kBlock, qstride = static_cast<size_t>(bpp) * dsc.tile_stride;
  size_t p = static_cast<size_t>(j) * kBlock + tid;
  size_t q = dsc.first_vec + static_cast<size_t>(j) * dsc.tile_stride + tid;
  unsigned long long count = 0;   // wave-uniform
  VecRegs<ST, DEPTH> cur, nxt;
  if (p < nvec) cur.load(pl, q);
  for (size_t t0 = static_cast<size_t>(j) * kBlock; t0 < nvec; t0 += stride) {
    const size_t pn = p + stride;
    q += qstride;
    if (pn < nvec) nxt.load(pl, q);
#pragma unroll
    for (int h = 0; h < PPT; ++h) {
      double x = cur.coord(0, h), y = cur.coord(1, h), z = cur.coord(2, h);
      double u = cur.coord(3, h), v = cur.coord(4, h), w = cur.coord(5, h);
      double r0, r1, r2, e0, e1, e2;
      residual<DEPTH>(P, x, y, z, u, v, w, DEPTH == DEPTH_PER_MATCH ? cur.depth1(h) : 1.0,
                      DEPTH == DEPTH_PER_MATCH ? cur.depth2(h) : 0.0, r0, r1, r2, e0, e1, e2);
      const double s = sq_norm(e0, e1, e2);
      const bool inl = !loss || !(s > P->delta2);   // NaN: no outlier in the sweep, an inlier here
      const size_t i = p * PPT + h;
      const bool valid = i < n;                     // implies p < nvec
      count += __popcll(__ballot(valid && inl));
      if (valid) {
        const size_t row = row0 + i;
        if (OUT & kOutE) { out.e[3 * row] = e0; out.e[3 * row + 1] = e1; out.e[3 * row + 2] = e2; }
        if (OUT & kOutSq) out.sq[row] = s;
        if (OUT & kOutInlier) out.inlier[row] = inl ? 1 : 0;
      }
    }
    cur = nxt;
    p = pn;
  }
  if (lane == 0) wave_count[wave] = count;
  __syncthreads();
  if (tid == 0) {
    unsigned long long c = 0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) c += wave_count[w];
    if (c) atomicAdd(out.n_inlier + pair, c);
  }
}

template <int DEPTH, typename ST>
hipError_t launch_batch_residuals_outputs(int outputs, const Planes& pl, const PairDesc* desc, const unsigned long long* offsets,
                                          const BatchState* state, double huber_delta, int bpp, const ResidualOut& out,
                                          unsigned grid, hipStream_t stream) {
  switch (outputs & 7) {
#define SBA_BATCH_RESIDUAL_CASE(F)                                                                                        \
    case F:                                                                                                               \
      hipLaunchKernelGGL((batch_residual_kernel<DEPTH, ST, F>), dim3(grid), dim3(kBlock), 0, stream, pl, desc, offsets,  \
                         state, huber_delta, bpp, out);                                                                   \
      break;
    SBA_BATCH_RESIDUAL_CASE(0) SBA_BATCH_RESIDUAL_CASE(1) SBA_BATCH_RESIDUAL_CASE(2) SBA_BATCH_RESIDUAL_CASE(3)
    SBA_BATCH_RESIDUAL_CASE(4) SBA_BATCH_RESIDUAL_CASE(5) SBA_BATCH_RESIDUAL_CASE(6) SBA_BATCH_RESIDUAL_CASE(7)
#undef SBA_BATCH_RESIDUAL_CASE
  }
  return hipGetLastError();
}

// One wave per pair: kept rows before row x = tile_offset[x / T] + kept in [(x / T) T, x) (at most T - 1 keep bytes, 32
// coalesced byte loads per lane); pair_kept[g] is the difference at the pair's two ends.  No atomics.
__device__ __forceinline__ unsigned long long kept_before(const unsigned char* __restrict__ keep,
                                                          const unsigned long long* __restrict__ tile_offset, size_t ntiles,
                                                          const unsigned long long* __restrict__ total, size_t x) {
  const size_t t = x / kCompactTile;
  if (t >= ntiles) return total[0];                 // x = rows = ntiles * T
  unsigned c = 0;
  for (size_t i = t * kCompactTile + threadIdx.x; i < x; i += 64) c += keep[i] != 0;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) c += __shfl_xor(c, off);
  return tile_offset[t] + c;
}
__global__ __launch_bounds__(64) void batch_pair_kept_kernel(const unsigned char* __restrict__ keep,
                                                             const unsigned long long* __restrict__ tile_offset, size_t ntiles,
                                                             const unsigned long long* __restrict__ total,
                                                             const unsigned long long* __restrict__ offsets,
                                                             unsigned long long* __restrict__ pair_kept) {
  const unsigned g = blockIdx.x;
  const unsigned long long hi = kept_before(keep, tile_offset, ntiles, total, offsets[g + 1]);
  const unsigned long long lo = kept_before(keep, tile_offset, ntiles, total, offsets[g]);
  if (threadIdx.x == 0) pair_kept[g] = hi - lo;
}

// compact_scatter_kernel over the concatenated rows; a kept row i stays in its pair g (bisection of the old offsets), so
// its new row o = tile_offset + rank is element o - new_offsets[g] of the same pair in the new layout.
template <typename ST>
__global__ __launch_bounds__(256) void batch_compact_scatter_kernel(BatchCompactArgs a) {
  __shared__ unsigned int wave_cnt[2][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t tile0 = static_cast<size_t>(blockIdx.x) * kCompactTile;
  unsigned long long pos0 = a.tile_offset[blockIdx.x];
  for (int r = 0; r < kCompactRounds; ++r) {
    const size_t i = tile0 + static_cast<size_t>(r) * 256 + threadIdx.x;
    const bool k = i < a.rows && a.keep[i] != 0;
    const unsigned long long m = __ballot(k);
    const unsigned rank = __builtin_amdgcn_mbcnt_hi(static_cast<unsigned>(m >> 32),
                                                    __builtin_amdgcn_mbcnt_lo(static_cast<unsigned>(m), 0u));
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
      constexpr size_t ppt = Lanes<ST>::PPT;      // a compile-time tile width: no 64-bit division per row
      const int g = batch_pair_of(i, a.old_offsets, a.num_pairs);
      const size_t src = pair_element(a.old_desc[g], i - a.old_offsets[g], ppt);
      const size_t dst = pair_element(a.new_desc[g], o - a.new_offsets[g], ppt);
#pragma unroll
      for (int c = 0; c < 6; ++c) static_cast<ST*>(a.dst[c])[dst] = static_cast<const ST*>(a.src[c])[src];
      if (a.src[6]) {
        static_cast<double*>(a.dst[6])[dst] = static_cast<const double*>(a.src[6])[src];
        static_cast<double*>(a.dst[7])[dst] = static_cast<const double*>(a.src[7])[src];
      }
      if (a.kept_index) a.kept_index[o] = static_cast<long long>(i);
    }
    pos0 += all;
  }
}

}  // namespace

hipError_t launch_residuals(int depth, int store, int outputs, const Planes& pl, const SweepParams& prm,
                            const ResidualOut& out, int grid, hipStream_t stream) {
  if (prm.n == 0 || grid <= 0) return hipSuccess;
  if (depth == kDepthFolded && store == 0) return launch_residuals_outputs<DEPTH_FOLDED, double>(outputs, pl, prm, out, grid, stream);
  if (depth == DEPTH_PER_MATCH)
    return store == 0 ? launch_residuals_outputs<DEPTH_PER_MATCH, double>(outputs, pl, prm, out, grid, stream)
                      : launch_residuals_outputs<DEPTH_PER_MATCH, float>(outputs, pl, prm, out, grid, stream);
  if (depth == DEPTH_UNIFORM)
    return store == 0 ? launch_residuals_outputs<DEPTH_UNIFORM, double>(outputs, pl, prm, out, grid, stream)
                      : launch_residuals_outputs<DEPTH_UNIFORM, float>(outputs, pl, prm, out, grid, stream);
  return hipErrorInvalidValue;
}

hipError_t launch_compact_count(const unsigned char* keep, size_t ntiles, unsigned int* tile_count, hipStream_t stream) {
  if (ntiles == 0) return hipSuccess;
  hipLaunchKernelGGL(compact_count_kernel, dim3(static_cast<unsigned>(ntiles)), dim3(256), 0, stream, keep, tile_count);
  return hipGetLastError();
}

hipError_t launch_compact_scan(const unsigned int* tile_count, size_t ntiles, unsigned long long* tile_offset,
                               unsigned long long* total, hipStream_t stream) {
  hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(1024), 0, stream, tile_count, ntiles, tile_offset, total);
  return hipGetLastError();
}

hipError_t launch_compact_scatter(int store, const CompactArgs& args, size_t ntiles, hipStream_t stream) {
  if (ntiles == 0) return hipSuccess;
  if (store == 0)
    hipLaunchKernelGGL(compact_scatter_kernel<double>, dim3(static_cast<unsigned>(ntiles)), dim3(256), 0, stream, args);
  else
    hipLaunchKernelGGL(compact_scatter_kernel<float>, dim3(static_cast<unsigned>(ntiles)), dim3(256), 0, stream, args);
  return hipGetLastError();
}

hipError_t launch_batch_residuals(int depth, int store, int outputs, const Planes& pl, const PairDesc* desc,
                                  const unsigned long long* offsets, const BatchState* state, double huber_delta,
                                  int num_pairs, int bpp, const ResidualOut& out, hipStream_t stream) {
  if (num_pairs <= 0 || bpp <= 0) return hipSuccess;
  const unsigned grid = static_cast<unsigned>(num_pairs) * static_cast<unsigned>(bpp);
  if (depth == DEPTH_PER_MATCH)
    return store == 0 ? launch_batch_residuals_outputs<DEPTH_PER_MATCH, double>(outputs, pl, desc, offsets, state, huber_delta, bpp, out, grid, stream)
                      : launch_batch_residuals_outputs<DEPTH_PER_MATCH, float>(outputs, pl, desc, offsets, state, huber_delta, bpp, out, grid, stream);
  if (depth == DEPTH_UNIFORM)
    return store == 0 ? launch_batch_residuals_outputs<DEPTH_UNIFORM, double>(outputs, pl, desc, offsets, state, huber_delta, bpp, out, grid, stream)
                      : launch_batch_residuals_outputs<DEPTH_UNIFORM, float>(outputs, pl, desc, offsets, state, huber_delta, bpp, out, grid, stream);
  return hipErrorInvalidValue;
}

hipError_t launch_batch_pair_kept(const unsigned char* keep, const unsigned long long* tile_offset, size_t ntiles,
                                  const unsigned long long* total, const unsigned long long* offsets, int num_pairs,
                                  unsigned long long* pair_kept, hipStream_t stream) {
  if (num_pairs <= 0) return hipSuccess;
  hipLaunchKernelGGL(batch_pair_kept_kernel, dim3(static_cast<unsigned>(num_pairs)), dim3(64), 0, stream, keep, tile_offset,
                     ntiles, total, offsets, pair_kept);
  return hipGetLastError();
}

hipError_t launch_batch_compact_scatter(int store, const BatchCompactArgs& args, size_t ntiles, hipStream_t stream) {
  if (ntiles == 0) return hipSuccess;
  if (store == 0)
    hipLaunchKernelGGL(batch_compact_scatter_kernel<double>, dim3(static_cast<unsigned>(ntiles)), dim3(256), 0, stream, args);
  else
    hipLaunchKernelGGL(batch_compact_scatter_kernel<float>, dim3(static_cast<unsigned>(ntiles)), dim3(256), 0, stream, args);
  return hipGetLastError();
}

}  // namespace sba
