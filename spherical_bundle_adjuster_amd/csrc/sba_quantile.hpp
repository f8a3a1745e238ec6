// Exact order statistics of a device-resident plane of squared residual norms, and the keep-rule built on them
// (sba_quantile.hip: kernels; sba_quantile.cpp: entry points).  Internal: nothing here is exported from the library.
//
// The plane s holds, pair after pair, the rows of every pair (a single problem is one pair); offsets[g] ... offsets[g + 1]
// are pair g's rows.  The key of a row is the bit pattern of s read as an unsigned 64-bit integer: numeric order for
// s >= +0, and every NaN (either sign) sorts above +inf.  The k-th smallest key of a pair is found by a radix select from
// the top digit down: kSelectPasses passes of kSelectBits bits, each a histogram of one digit over the keys that still
// share the selected prefix, then a narrowing of prefix and rank.  All counts are integers, so the result is the same bits
// on every run and for every grid.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace sba {

constexpr int kSelectBits = 8;
constexpr int kSelectBins = 1 << kSelectBits;
constexpr int kSelectPasses = 64 / kSelectBits;
constexpr int kSelectMaxRanks = 8;

// A pair's running selection, kept on the device between passes.  Ranks whose prefixes coincide share one histogram:
// uprefix[0 .. nuniq) are the distinct prefixes, slot[j] the one rank j follows.
struct SelectState {
  unsigned long long prefix[kSelectMaxRanks];    // digits selected so far, right-aligned
  unsigned long long rank[kSelectMaxRanks];      // rank among the keys that carry prefix
  unsigned long long uprefix[kSelectMaxRanks];
  int slot[kSelectMaxRanks];
  int nuniq;
  int pad_;
};

// The device scratch of one selection, carved from the handle's select_scratch: per-pair inlier counts (the residual kernel's
// by-product) | kept counts | a single problem's two row offsets | ranks | values | scales | thresholds | selection states |
// histograms | the s plane.
struct SelectScratch {
  unsigned long long* n_inlier = nullptr;
  unsigned long long* kept = nullptr;
  unsigned long long* offsets = nullptr;
  unsigned long long* ranks = nullptr;
  double* values = nullptr;
  double* scale = nullptr;
  double* thr = nullptr;
  SelectState* state = nullptr;
  unsigned long long* hist = nullptr;
  double* sq = nullptr;
  size_t bytes = 0;
};

// values[g][j] = the ranks[g][j]-th smallest (0-based) of pair g's rows of s, NaN for a pair without rows; with scale != null
// also thr[g] = scale[g] * values[g][0] (one f64 multiplication).  bpp blocks share a pair.  state [num_pairs] and
// hist [num_pairs][num_ranks][kSelectBins] are device work space; everything is enqueued on `stream`.
hipError_t launch_order_stats(const double* s, const unsigned long long* offsets, int num_pairs, int bpp,
                              const unsigned long long* ranks, int num_ranks, const double* scale, SelectState* state,
                              unsigned long long* hist, double* values, double* thr, hipStream_t stream);
// keep[row] = s[row] <= thr[g] for every row of pair g (a NaN s is dropped: the comparison is false), kept[g] (zeroed here)
// = the number of rows kept.
hipError_t launch_keep_below(const double* s, const unsigned long long* offsets, int num_pairs, int bpp, const double* thr,
                             unsigned char* keep, unsigned long long* kept, hipStream_t stream);

}  // namespace sba
