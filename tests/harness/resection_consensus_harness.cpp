// TEST HARNESS (tests/ only): the host side of the robust resection guess (csrc/sba_resection_consensus.hpp, header-only, no
// HIP) for the CPU: the sampler, the moments of a row list, a whole trial (moments + DLT finish) and the pick.
#include "../../spherical_bundle_adjuster_amd/csrc/sba_resection_consensus.hpp"

extern "C" void consensus_harness_sample(unsigned long long seed, int trial, unsigned long long n, int sample_size, long long* out) {
  sba::resect_sample_trial(seed, trial, n, sample_size, out);
}

// rows [m][6] = (X | y) -> mom61: the 60 sums, then the row count
extern "C" void consensus_harness_row_moments(const double* rows, int m, double* mom61) { sba::resect_row_moments(rows, m, mom61); }

// info7: lambda1, lambda2, lambda12, sv[3], scale
extern "C" int consensus_harness_trial(const double* rows, int m, double* rot, double* tran, double* info7) {
  sba_resection_guess_info info;
  const int rc = sba::resect_trial_pose(rows, m, rot, tran, &info);
  info7[0] = info.lambda1; info7[1] = info.lambda2; info7[2] = info.lambda12;
  for (int k = 0; k < 3; ++k) info7[3 + k] = info.sv[k];
  info7[6] = info.scale;
  return rc;
}

extern "C" int consensus_harness_pick(const long long* counts, int trials) { return sba::resect_pick(counts, trials); }

extern "C" int consensus_harness_limit(int which) {
  const int v[] = {SBA_RESECT_MAX_TRIALS, SBA_RESECT_MAX_SAMPLE, SBA_RESECT_DEFAULT_TRIALS, SBA_RESECT_MIN_SAMPLE, SBA_RESECT_ROW,
                   SBA_RESECT_CANDIDATE};
  return which >= 0 && which < 6 ? v[which] : -1;
}
