// Host side of the robust resection guess (include/sba_hip.h: sba_problem_resection_guess_consensus): sampled minimal DLT
// trials, scored on the device.  HIP-free; the kernels are in sba_resection_consensus.hip, the entry points in
// sba_resection_consensus.cpp, the DLT finish every trial ends in is sba_resection.hpp's.
//
// Here: the sampler (which matches a trial draws), the 60 DLT moments of a short list of rows summed in list order (what
// resect_moments_kernel sums over the whole handle, for the few rows of one trial) and the pick among the scored trials.
#pragma once
#include <cmath>
#include <cstdint>

#include "sba_epipolar.hpp"
#include "sba_resection.hpp"

#if defined(__clang__)
#pragma STDC FP_CONTRACT OFF
#endif

enum {
  SBA_RESECT_MAX_TRIALS = 1024, SBA_RESECT_MAX_SAMPLE = 64, SBA_RESECT_DEFAULT_TRIALS = 128, SBA_RESECT_MIN_SAMPLE = 6,
  SBA_RESECT_ROW = 6,            // a gathered row: X (the rounded product d1 x1), then y
  SBA_RESECT_CANDIDATE = 12      // a scored candidate: Rn (9, row-major) | t (3) of fill_resect_params
};

namespace sba {

// The matches trial `trial` draws out of n >= sample_size: seeded as epi::trial_groups seeds, j = splitmix64(s) % n again
// and again, a j the trial already holds skipped, until sample_size distinct indices stand in draw order.  A longer sample
// extends a shorter one.
inline void resect_sample_trial(uint64_t seed, int trial, uint64_t n, int sample_size, long long* out) {
  uint64_t s = seed * 0x2545F4914F6CDD1Dull + static_cast<uint64_t>(trial) * 0xD6E8FEB86659FD93ull + 1;
  int held = 0;
  while (held < sample_size) {
    const long long j = static_cast<long long>(epi::splitmix64(s) % n);
    bool seen = false;
    for (int i = 0; i < held; ++i) seen = seen || out[i] == j;
    if (!seen) out[held++] = j;
  }
}

// The SBA_RESECT_MOM_COUNT sums of m rows (X | y) in list order, the arithmetic of resect_moments (sba_resection_core.hpp):
// slot 6 p + k += (X~ X~^T)[a][b] Q[k] by one fused multiply-add, X~ = (X, -1), Q = (y . y) I - y y^T; then the row count.
inline void resect_row_moments(const double* rows, int m, double* mom) {
  for (int k = 0; k < SBA_RESECT_MOM_COUNT; ++k) mom[k] = 0.0;
  for (int i = 0; i < m; ++i) {
    const double* X = rows + SBA_RESECT_ROW * i;
    const double* y = X + 3;
    const double yy = y[0] * y[0] + y[1] * y[1] + y[2] * y[2];
    double Q[6];
    int q = 0;
    for (int c = 0; c < 3; ++c)
      for (int d = c; d < 3; ++d) Q[q++] = (c == d ? yy : 0.0) - y[c] * y[d];
    const double Xt[4] = {X[0], X[1], X[2], -1.0};
    int p = 0;
    for (int a = 0; a < 4; ++a)
      for (int b = a; b < 4; ++b) {
        const double xx = Xt[a] * Xt[b];
        for (int k = 0; k < 6; ++k) mom[6 * p + k] = std::fma(xx, Q[k], mom[6 * p + k]);
        ++p;
      }
    mom[SBA_RESECT_MOM_N] += 1.0;
  }
}

// One trial: the moments of its rows, then resect_dlt_finish.  SBA_OK or SBA_ERR_NUMERIC (the trial is invalid).
inline int resect_trial_pose(const double* rows, int m, double rot[3], double tran[3], sba_resection_guess_info* info) {
  double mom[SBA_RESECT_MOM_COUNT];
  resect_row_moments(rows, m, mom);
  const char* why = "";
  return resect_dlt_finish(mom, mom[SBA_RESECT_MOM_N], rot, tran, info, &why);
}

// The trial with the largest inlier count, the lowest index among equals; entries < 0 (refused trials) never win.
// -1: no trial has a count.
inline int resect_pick(const long long* counts, int trials) {
  int best = -1;
  for (int t = 0; t < trials; ++t)
    if (counts[t] >= 0 && (best < 0 || counts[t] > counts[best])) best = t;
  return best;
}

}  // namespace sba

#if defined(__clang__)
#pragma STDC FP_CONTRACT DEFAULT
#endif
