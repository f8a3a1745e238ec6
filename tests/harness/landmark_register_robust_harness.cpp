// TEST HARNESS (tests/ only): the host and device share of the robust joint registration
// (csrc/sba_landmarks_register_robust.hpp, header-only, no HIP) compiled for the CPU: one observation into the robust sums of
// the reduce pass, and the option check of the entry points.  The freeze and the write-back are the non-robust ones
// (tests/harness/landmark_register_harness.cpp).
#include "../../spherical_bundle_adjuster_amd/csrc/sba_landmarks_register_robust.hpp"

// out: H row-major (36), g (6), cost, n_used, n_behind, n_outlier -- one set of lane sums over all rows, expanded by resect_expand_row.
extern "C" void landmark_register_robust_harness_eval(long long n, const double* X, const double* cov, const double* y, const double* noise,
                                                      const double* rot, const double* tran, double huber_delta, double* out) {
  sba::LandmarkRegisterParams P;
  sba::landmark_register_fill(static_cast<unsigned long long>(n), static_cast<unsigned long long>(n), rot, tran, nullptr, 0.0, INFINITY, &P);
  sba::LandmarkRegisterRobust L;
  sba::landmark_register_robust_fill(huber_delta, &L);
  double acc[SBA_RESECT_SIZE] = {0};
  for (long long i = 0; i < n; ++i)
    sba::landmark_register_accumulate_robust(P, L.delta, L.delta2, X + 3 * i, cov + 6 * i, y + 3 * i, noise[i], sba::landmark_register_live(noise[i]),
                                             acc);
  sba_normal_eq ne;
  double n_behind = 0.0;
  sba::resect_expand_row(acc, &ne, &n_behind);
  for (int k = 0; k < 36; ++k) out[k] = ne.H[k];
  for (int k = 0; k < 6; ++k) out[36 + k] = ne.g[k];
  out[42] = ne.cost; out[43] = ne.sum_w; out[44] = n_behind; out[45] = ne.n_outlier;
}

// returns 1 when accepted
extern "C" int landmark_register_robust_harness_check(double huber_delta, double chi2_gate) {
  return sba::landmark_register_check_robust(huber_delta, chi2_gate) == nullptr ? 1 : 0;
}
