// TEST PROGRAM (tests/ only; built with g++ -fsanitize=address,undefined and run as a child process by
// tests/test_resection_weighted_host_cpu.py): the host side of the covariance-weighted resection with exact-sized heap buffers --
// the basis at every choice of axis and on ties, the factor on definite, indefinite, zero and non-finite covariances, the row
// expansion, the option checks at their limits, the 6 x 6 inverse and the finish of the pose covariance with its refusals.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../spherical_bundle_adjuster_amd/csrc/sba_resection_weighted.hpp"

namespace {

int failures = 0;
void expect(bool ok, const char* what) {
  if (!ok) { std::printf("FAILED: %s\n", what); ++failures; }
}

double dot(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

}  // namespace

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const double ys[][3] = {{0.1, 0.7, -0.7}, {0.7, -0.1, 0.7}, {0.6, 0.8, 0.0}, {1.0, 1.0, 1.0}, {0.0, 0.0, 7.5}, {-2.0, 2.0, 3.0}};
  for (const auto& yv : ys) {
    std::vector<double> y(yv, yv + 3), b1(3, nan), b2(3, nan), q(3, nan), M(6, nan);
    sba::resect_weight_basis(y.data(), b1.data(), b2.data());
    const double yy = dot(y.data(), y.data());
    expect(std::fabs(dot(b1.data(), y.data())) <= 1e-15 * yy && std::fabs(dot(b2.data(), y.data())) <= 1e-15 * yy * std::sqrt(yy), "basis across the bearing");
    expect(std::fabs(dot(b1.data(), b2.data())) <= 1e-15 * yy * std::sqrt(yy), "basis vectors orthogonal");
    expect(dot(b1.data(), b1.data()) > 0.0 && dot(b2.data(), b2.data()) > 0.0, "basis vectors non-zero");
    const std::vector<double> S = {4.0, 9.0, 1.0, 0.5, -0.25, 0.75};
    expect(sba::resect_weight_factor(S.data(), b1.data(), b2.data(), q.data()), "a definite covariance has weight");
    expect(q[0] > 0.0 && q[2] > 0.0, "positive diagonal");
    sba::resect_weight_expand(q.data(), y.data(), M.data());
    // M y = 0 and M S M = M
    const double My[3] = {M[0] * y[0] + M[3] * y[1] + M[4] * y[2], M[3] * y[0] + M[1] * y[1] + M[5] * y[2], M[4] * y[0] + M[5] * y[1] + M[2] * y[2]};
    expect(std::fabs(My[0]) + std::fabs(My[1]) + std::fabs(My[2]) <= 1e-13 * std::sqrt(yy), "M y = 0");
    const std::vector<std::vector<double>> bad = {{0, 0, 0, 0, 0, 0}, {-1, 1, 1, 0, 0, 0}, {inf, inf, inf, 0, 0, 0}, {1, nan, 1, 0, 0, 0},
                                                  {1, 1, 1, 0, 0, 2}};
    for (const auto& Sb : bad) {
      std::vector<double> qb(3, nan);
      const bool ok = sba::resect_weight_factor(Sb.data(), b1.data(), b2.data(), qb.data());
      expect(!ok || (std::isfinite(qb[0]) && std::isfinite(qb[1]) && std::isfinite(qb[2])), "a factor with weight is finite");
      if (!ok) expect(qb[0] == 0.0 && qb[1] == 0.0 && qb[2] == 0.0, "no weight: zeros");
    }
    std::vector<double> qz(3, nan);
    const std::vector<double> zero(6, 0.0);
    expect(!sba::resect_weight_factor(zero.data(), b1.data(), b2.data(), qz.data()) && qz[0] == 0.0, "a zero covariance has no weight");
  }
  expect(sba::resect_weight_check_scale(1.3) == nullptr && sba::resect_weight_check_scale(0.0) && sba::resect_weight_check_scale(-1.0) &&
             sba::resect_weight_check_scale(inf) && sba::resect_weight_check_scale(nan), "cov_scale");
  expect(sba::resect_weight_check_sigma(0.0) == nullptr && sba::resect_weight_check_sigma(1e-3) == nullptr && sba::resect_weight_check_sigma(-1e-3) &&
             sba::resect_weight_check_sigma(inf) && sba::resect_weight_check_sigma(nan), "bearing_sigma");
  expect(sba::resect_weight_check_rounds(1) == nullptr && sba::resect_weight_check_rounds(8) == nullptr && sba::resect_weight_check_rounds(0) &&
             sba::resect_weight_check_rounds(9) && sba::resect_weight_check_rounds(-1), "reweight_rounds");
  {
    // H = D + u u^T, well conditioned
    std::vector<double> H(36, 0.0), inv(36, nan);
    const double u[6] = {0.3, -0.2, 0.5, 0.1, -0.4, 0.2};
    for (int a = 0; a < 6; ++a)
      for (int b = 0; b < 6; ++b) H[6 * a + b] = (a == b ? 1.0 + a : 0.0) + u[a] * u[b];
    expect(sba::resect_cov_inverse(H.data(), inv.data()), "a definite matrix inverts");
    double worst = 0.0;
    for (int a = 0; a < 6; ++a)
      for (int b = 0; b < 6; ++b) {
        double s = 0.0;
        for (int k = 0; k < 6; ++k) s += H[6 * a + k] * inv[6 * k + b];
        worst = std::fmax(worst, std::fabs(s - (a == b ? 1.0 : 0.0)));
        expect(inv[6 * a + b] == inv[6 * b + a], "inverse symmetric to the bit");
      }
    expect(worst <= 1e-14, "H inv = I");
    std::vector<double> keep(36, 7.0);
    H[6 * 5 + 5] = -1.0;
    expect(!sba::resect_cov_inverse(H.data(), keep.data()) && keep[0] == 7.0 && keep[35] == 7.0, "an indefinite matrix is refused, nothing written");
    H[6 * 5 + 5] = nan;
    expect(!sba::resect_cov_inverse(H.data(), keep.data()) && keep[0] == 7.0, "a NaN matrix is refused");
  }
  {
    std::vector<double> row(SBA_RESECT_SIZE, 0.0);
    int k = 0;
    for (int a = 0; a < 6; ++a)
      for (int b = a; b < 6; ++b) row[k++] = a == b ? 2.0 + a : 0.1;
    row[SBA_RESECT_COST] = 10.0; row[SBA_RESECT_SW] = 9.0; row[SBA_RESECT_NOUT] = 1.0;
    sba_resection_cov res;
    const char* why = nullptr;
    expect(sba::resect_cov_finish(row.data(), 10, 2, &res, &why) == SBA_OK, "finish");
    expect(res.n_used == 8 && res.n_zero_weight == 2 && res.dof == 10 && res.sigma2 == 2.0 && res.cost == 10.0 && res.sum_w == 9.0 && res.n_outlier == 1.0,
           "finish: counts and sigma2");
    sba_resection_cov keep;
    keep.dof = -77;
    expect(sba::resect_cov_finish(row.data(), 3, 0, &keep, &why) == SBA_ERR_NUMERIC && keep.dof == -77 && why && why[0], "dof = 0 is refused, nothing written");
    expect(sba::resect_cov_finish(row.data(), 10, 7, &keep, &why) == SBA_ERR_NUMERIC && keep.dof == -77, "dof <= 0 after zero weights is refused");
    row[3] = nan;
    expect(sba::resect_cov_finish(row.data(), 10, 0, &keep, &why) == SBA_ERR_NUMERIC && keep.dof == -77, "non-finite sums are refused");
  }
  if (failures) return 1;
  std::printf("resection weighted host checks passed\n");
  return 0;
}
