// TEST HARNESS (tests/ only): the host side of the covariance-weighted resection (csrc/sba_resection_weighted.hpp, header-only,
// no HIP) compiled for the CPU: the basis, the factor of a projected covariance, the expansion of a stored factor to the row
// of M, the option checks, the 6 x 6 inverse and the finish of the pose covariance.
#include "../../spherical_bundle_adjuster_amd/csrc/sba_resection_weighted.hpp"

extern "C" void resection_weighted_harness_basis(const double* y3, double* b1, double* b2) { sba::resect_weight_basis(y3, b1, b2); }

// S6: (xx, yy, zz, xy, xz, yz) -> q3; returns 1 when the match has weight
extern "C" int resection_weighted_harness_factor(const double* S6, const double* y3, double* q3) {
  double b1[3], b2[3];
  sba::resect_weight_basis(y3, b1, b2);
  return sba::resect_weight_factor(S6, b1, b2, q3) ? 1 : 0;
}

extern "C" void resection_weighted_harness_rows(const double* q, const double* y, long long n, double* rows) {
  for (long long i = 0; i < n; ++i) sba::resect_weight_expand(q + 3 * i, y + 3 * i, rows + 6 * i);
}

// which: 0 cov_scale, 1 bearing_sigma, 2 reweight_rounds (value truncated); returns 1 when accepted
extern "C" int resection_weighted_harness_check(int which, double value) {
  const char* why = which == 0 ? sba::resect_weight_check_scale(value)
                               : (which == 1 ? sba::resect_weight_check_sigma(value) : sba::resect_weight_check_rounds(static_cast<int>(value)));
  return why == nullptr ? 1 : 0;
}

extern "C" int resection_weighted_harness_inverse(const double* H36, double* inv36) { return sba::resect_cov_inverse(H36, inv36) ? 1 : 0; }

// out: cov (36), cost, sum_w, n_used, n_zero_weight, n_outlier, dof, sigma2 = 43 doubles; returns the status
extern "C" int resection_weighted_harness_finish(const double* row32, long long n, long long n_zero, double* out43) {
  sba_resection_cov res;
  const char* why = "";
  const int rc = sba::resect_cov_finish(row32, n, n_zero, &res, &why);
  if (rc != SBA_OK) return rc;
  for (int i = 0; i < 36; ++i) out43[i] = res.cov[i];
  out43[36] = res.cost; out43[37] = res.sum_w; out43[38] = static_cast<double>(res.n_used);
  out43[39] = static_cast<double>(res.n_zero_weight); out43[40] = res.n_outlier; out43[41] = static_cast<double>(res.dof);
  out43[42] = res.sigma2;
  return rc;
}
