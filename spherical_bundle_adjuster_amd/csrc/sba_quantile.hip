// Radix select over a plane of squared residual norms and the threshold that turns a selected value into keep bytes
// (sba_quantile.hpp; host side in sba_quantile.cpp).
//
// select_hist_kernel: block group g = blockIdx.x / bpp takes pair g and reads its rows as 8-byte keys, kSelectUnroll
// coalesced loads in flight per thread.  A key that carries one of the pair's distinct prefixes adds one to that prefix's
// histogram of the pass's digit, in LDS (8 KiB: 8 prefixes x 256 bins x 4 B, many blocks per CU).  The top digits of an f64 are
// sign and exponent, so in the first passes nearly every key of a thread falls into the same bin: a thread counts a run of
// equal bins in a register and issues one LDS atomic per run, not one per key.  At the end the block adds its non-zero bins
// to the pair's global histogram (64-bit integer atomics: exact, order-free).
// select_narrow_kernel (one block per pair): for every rank, an exclusive scan of its histogram finds the digit whose bin
// holds the rank; prefix and rank narrow, the distinct prefixes of the next pass are listed, the histogram is zeroed.  The
// last pass leaves the whole key: the value (and scale * value).  Nothing goes to the host between passes.
// keep_below_kernel: keep[row] = s[row] <= thr[pair] from the 8-byte plane alone; the kept count is a per-wave __ballot +
// popcount, folded per block and added to the pair's word with an integer atomic.
#include "sba_quantile.hpp"

namespace sba {
namespace {

constexpr int kSelectBlock = 256;
constexpr int kSelectUnroll = 4;
constexpr unsigned long long kNoPrefix = ~0ull;   // no prefix of fewer than 64 bits equals it

__global__ __launch_bounds__(64) void select_init_kernel(const unsigned long long* __restrict__ ranks, int num_pairs,
                                                         int num_ranks, SelectState* __restrict__ state) {
  const int g = blockIdx.x * 64 + threadIdx.x;
  if (g >= num_pairs) return;
  SelectState st;
#pragma unroll
  for (int j = 0; j < kSelectMaxRanks; ++j) {
    st.prefix[j] = 0;
    st.rank[j] = j < num_ranks ? ranks[static_cast<size_t>(g) * num_ranks + j] : 0;
    st.uprefix[j] = j == 0 ? 0 : kNoPrefix;
    st.slot[j] = 0;
  }
  st.nuniq = 1;
  st.pad_ = 0;
  state[g] = st;
}

__global__ __launch_bounds__(kSelectBlock) void select_hist_kernel(const double* __restrict__ s,
                                                                   const unsigned long long* __restrict__ offsets,
                                                                   const SelectState* __restrict__ state, int num_ranks,
                                                                   int bpp, int pass, unsigned long long* __restrict__ hist) {
  __shared__ unsigned int h[kSelectMaxRanks * kSelectBins];
  const int tid = threadIdx.x;
  const unsigned pair = blockIdx.x / static_cast<unsigned>(bpp), j = blockIdx.x % static_cast<unsigned>(bpp);
  const size_t row0 = offsets[pair], n = offsets[pair + 1] - row0;
  if (static_cast<size_t>(j) * kSelectBlock * kSelectUnroll >= n) return;   // block-uniform: nothing of the pair is this block's
  const SelectState* st = state + pair;
  const int nu = st->nuniq;
  unsigned long long up[kSelectMaxRanks];
#pragma unroll
  for (int u = 0; u < kSelectMaxRanks; ++u) up[u] = st->uprefix[u];
  for (int b = tid; b < nu * kSelectBins; b += kSelectBlock) h[b] = 0;
  __syncthreads();

  const unsigned long long* keys = reinterpret_cast<const unsigned long long*>(s) + row0;
  const int digit_shift = 64 - kSelectBits * (pass + 1);
  const int prefix_shift = digit_shift + kSelectBits;   // 64 in the first pass: no prefix yet, every key takes part
  const size_t stride = static_cast<size_t>(bpp) * kSelectBlock * kSelectUnroll;
  int run_bin = -1;
  unsigned run = 0;
  for (size_t base = static_cast<size_t>(j) * kSelectBlock * kSelectUnroll; base < n; base += stride) {
    unsigned long long key[kSelectUnroll];
    bool valid[kSelectUnroll];
#pragma unroll
    for (int k = 0; k < kSelectUnroll; ++k) {
      const size_t i = base + static_cast<size_t>(k) * kSelectBlock + tid;
      valid[k] = i < n;
      key[k] = valid[k] ? keys[i] : 0ull;
    }
#pragma unroll
    for (int k = 0; k < kSelectUnroll; ++k) {
      const unsigned long long hi = pass == 0 ? 0ull : key[k] >> prefix_shift;
      int slot = -1;
#pragma unroll
      for (int u = 0; u < kSelectMaxRanks; ++u) slot = hi == up[u] ? u : slot;
      if (valid[k] && slot >= 0) {
        const int bin = slot * kSelectBins + static_cast<int>((key[k] >> digit_shift) & (kSelectBins - 1));
        if (bin == run_bin) {
          ++run;
        } else {
          if (run) atomicAdd(&h[run_bin], run);
          run_bin = bin;
          run = 1;
        }
      }
    }
  }
  if (run) atomicAdd(&h[run_bin], run);
  __syncthreads();
  unsigned long long* dst = hist + static_cast<size_t>(pair) * num_ranks * kSelectBins;
  for (int b = tid; b < nu * kSelectBins; b += kSelectBlock) {
    const unsigned c = h[b];
    if (c) atomicAdd(dst + b, static_cast<unsigned long long>(c));
  }
}

__global__ __launch_bounds__(kSelectBins) void select_narrow_kernel(const unsigned long long* __restrict__ offsets,
                                                                    SelectState* __restrict__ state, int num_ranks, int pass,
                                                                    unsigned long long* __restrict__ hist,
                                                                    const double* __restrict__ scale,
                                                                    double* __restrict__ values, double* __restrict__ thr) {
  __shared__ SelectState st;
  __shared__ unsigned long long scan[2][kSelectBins];
  const int t = threadIdx.x;
  const unsigned pair = blockIdx.x;
  const bool last = pass == kSelectPasses - 1;
  const bool empty = offsets[pair + 1] == offsets[pair];
  if (empty) {   // takes no part; its histogram stayed zero
    if (last) {
      if (t < num_ranks) values[static_cast<size_t>(pair) * num_ranks + t] = __builtin_nan("");
      if (t == 0 && thr) thr[pair] = __builtin_nan("");
    }
    return;
  }
  if (t == 0) st = state[pair];
  __syncthreads();
  unsigned long long* rows = hist + static_cast<size_t>(pair) * num_ranks * kSelectBins;
  for (int j = 0; j < num_ranks; ++j) {
    const unsigned long long c = rows[st.slot[j] * kSelectBins + t];
    const unsigned long long rank = st.rank[j];
    int src = 0;
    scan[0][t] = c;
    __syncthreads();   // also orders the read of st.rank[j] before its update below
    for (int off = 1; off < kSelectBins; off <<= 1) {
      const unsigned long long v = scan[src][t] + (t >= off ? scan[src][t - off] : 0ull);
      scan[src ^ 1][t] = v;
      src ^= 1;
      __syncthreads();
    }
    const unsigned long long incl = scan[src][t], excl = incl - c;
    if (excl <= rank && rank < incl) {   // exactly one bin: the counts of the prefix sum to more than the rank
      st.prefix[j] = (st.prefix[j] << kSelectBits) | static_cast<unsigned long long>(t);
      st.rank[j] = rank - excl;
    }
    __syncthreads();
  }
  for (int b = t; b < num_ranks * kSelectBins; b += kSelectBins) rows[b] = 0;
  if (t == 0) {
    int nu = 0;
    for (int j = 0; j < num_ranks; ++j) {
      int u = 0;
      while (u < nu && st.uprefix[u] != st.prefix[j]) ++u;
      if (u == nu) st.uprefix[nu++] = st.prefix[j];
      st.slot[j] = u;
    }
    for (int u = nu; u < kSelectMaxRanks; ++u) st.uprefix[u] = kNoPrefix;
    st.nuniq = nu;
    state[pair] = st;
    if (last) {
      for (int j = 0; j < num_ranks; ++j)
        values[static_cast<size_t>(pair) * num_ranks + j] = __longlong_as_double(static_cast<long long>(st.prefix[j]));
      if (thr) thr[pair] = scale[pair] * __longlong_as_double(static_cast<long long>(st.prefix[0]));
    }
  }
}

// The loop bound is block-uniform, so every lane of a wave takes part in each ballot.
__global__ __launch_bounds__(kSelectBlock) void keep_below_kernel(const double* __restrict__ s,
                                                                  const unsigned long long* __restrict__ offsets,
                                                                  const double* __restrict__ thr, int bpp,
                                                                  unsigned char* __restrict__ keep,
                                                                  unsigned long long* __restrict__ kept) {
  __shared__ unsigned long long wave_count[kSelectBlock / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned pair = blockIdx.x / static_cast<unsigned>(bpp), j = blockIdx.x % static_cast<unsigned>(bpp);
  const size_t row0 = offsets[pair], n = offsets[pair + 1] - row0;
  const double cut = thr[pair];
  const size_t stride = static_cast<size_t>(bpp) * kSelectBlock * kSelectUnroll;
  unsigned long long count = 0;   // wave-uniform
  for (size_t base = static_cast<size_t>(j) * kSelectBlock * kSelectUnroll; base < n; base += stride) {
    double v[kSelectUnroll];
#pragma unroll
    for (int k = 0; k < kSelectUnroll; ++k) {
      const size_t i = base + static_cast<size_t>(k) * kSelectBlock + tid;
      v[k] = i < n ? s[row0 + i] : __builtin_nan("");
    }
#pragma unroll
    for (int k = 0; k < kSelectUnroll; ++k) {
      const size_t i = base + static_cast<size_t>(k) * kSelectBlock + tid;
      const bool below = v[k] <= cut;   // false for a NaN on either side
      count += __popcll(__ballot(below));
      if (i < n) keep[row0 + i] = below ? 1 : 0;
    }
  }
  if (lane == 0) wave_count[wave] = count;
  __syncthreads();
  if (tid == 0) {
    unsigned long long c = 0;
#pragma unroll
    for (int w = 0; w < kSelectBlock / 64; ++w) c += wave_count[w];
    if (c) atomicAdd(kept + pair, c);
  }
}

}  // namespace

hipError_t launch_order_stats(const double* s, const unsigned long long* offsets, int num_pairs, int bpp,
                              const unsigned long long* ranks, int num_ranks, const double* scale, SelectState* state,
                              unsigned long long* hist, double* values, double* thr, hipStream_t stream) {
  if (num_pairs <= 0 || bpp <= 0) return hipSuccess;
  if (num_ranks < 1 || num_ranks > kSelectMaxRanks) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(hist, 0, sizeof(unsigned long long) * num_pairs * num_ranks * kSelectBins, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(select_init_kernel, dim3((num_pairs + 63) / 64), dim3(64), 0, stream, ranks, num_pairs, num_ranks, state);
  const unsigned grid = static_cast<unsigned>(num_pairs) * static_cast<unsigned>(bpp);
  for (int pass = 0; pass < kSelectPasses; ++pass) {
    hipLaunchKernelGGL(select_hist_kernel, dim3(grid), dim3(kSelectBlock), 0, stream, s, offsets, state, num_ranks, bpp, pass,
                       hist);
    hipLaunchKernelGGL(select_narrow_kernel, dim3(static_cast<unsigned>(num_pairs)), dim3(kSelectBins), 0, stream, offsets,
                       state, num_ranks, pass, hist, scale, values, scale ? thr : nullptr);
  }
  return hipGetLastError();
}

hipError_t launch_keep_below(const double* s, const unsigned long long* offsets, int num_pairs, int bpp, const double* thr,
                             unsigned char* keep, unsigned long long* kept, hipStream_t stream) {
  if (num_pairs <= 0 || bpp <= 0) return hipSuccess;
  hipError_t e = hipMemsetAsync(kept, 0, sizeof(unsigned long long) * num_pairs, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(keep_below_kernel, dim3(static_cast<unsigned>(num_pairs) * static_cast<unsigned>(bpp)), dim3(kSelectBlock),
                     0, stream, s, offsets, thr, bpp, keep, kept);
  return hipGetLastError();
}

}  // namespace sba
