// TEST PROGRAM (tests/ only; built with g++ -fsanitize=address,undefined and run as a child process by
// tests/test_landmark_register_robust_host_cpu.py): the host and device share of the robust joint registration
// (csrc/sba_landmarks_register_robust.hpp) with exact-sized heap buffers over planted rows -- NaN rows, the padding observation
// with s = 0, one row behind, inliers and outliers -- and the option check.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../spherical_bundle_adjuster_amd/csrc/sba_landmarks_register_robust.hpp"

namespace {

int failures = 0;
void expect(bool ok, const char* what) {
  if (!ok) { std::printf("FAILED: %s\n", what); ++failures; }
}

bool all_zero(const std::vector<double>& v) {
  bool z = true;
  for (double x : v) z = z && x == 0.0;
  return z;
}

}  // namespace

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const std::vector<double> rot = {0.1, -0.2, 0.15}, tran = {0.3, -0.1, 0.2}, rot0 = {1e-9, 0.0, -2e-9};
  const std::vector<double> X = {1.0, -2.0, 4.0}, S = {0.04, 0.09, 0.01, 0.005, -0.0025, 0.0075};
  for (int variant = 0; variant < 4; ++variant) {
    const std::vector<double>& w = (variant & 1) ? rot0 : rot;
    const double bs = (variant & 2) ? 1e-3 : 0.0;
    sba::LandmarkRegisterParams P;
    sba::landmark_register_fill(1, 1, w.data(), tran.data(), nullptr, bs, inf, &P);
    std::vector<double> y(3);
    for (int k = 0; k < 3; ++k) y[k] = -(P.Rn[3 * k] * X[0] + P.Rn[3 * k + 1] * X[1] + P.Rn[3 * k + 2] * X[2] + P.t[k]);
    y[0] += 0.02; y[1] -= 0.01;
    std::vector<double> nz(1, -7.0);
    expect(sba::landmark_register_noise(P, X.data(), S.data(), y.data(), nz.data()) == sba::LANDMARK_LIVE, "a plain observation takes part");
    // its chi2, from the non-robust sums
    std::vector<double> plain(SBA_RESECT_SIZE, 0.0);
    sba::landmark_register_accumulate(P, X.data(), S.data(), y.data(), nz[0], true, plain.data());
    const double s = 2.0 * plain[SBA_RESECT_COST];
    expect(s > 0.0 && std::isfinite(s), "its chi2 is positive");
    // an inlier: delta above sqrt(s) -> the non-robust sums to the bit
    sba::LandmarkRegisterRobust L;
    sba::landmark_register_robust_fill(2.0 * std::sqrt(s), &L);
    std::vector<double> in(SBA_RESECT_SIZE, 0.0);
    sba::landmark_register_accumulate_robust(P, L.delta, L.delta2, X.data(), S.data(), y.data(), nz[0], true, in.data());
    expect(in == plain, "an inlier adds the non-robust sums, bit for bit");
    expect(in[SBA_RESECT_NOUT] == 0.0 && in[SBA_RESECT_SW] == 1.0, "an inlier is used and no outlier");
    // an outlier: delta = sqrt(s) / 4 -> w = 1/4, rho = 2 delta sqrt(s) - delta^2 = 7/16 s
    sba::landmark_register_robust_fill(0.25 * std::sqrt(s), &L);
    std::vector<double> out(SBA_RESECT_SIZE, 0.0);
    sba::landmark_register_accumulate_robust(P, L.delta, L.delta2, X.data(), S.data(), y.data(), nz[0], true, out.data());
    expect(out[SBA_RESECT_NOUT] == 1.0 && out[SBA_RESECT_SW] == 1.0 && out[SBA_RESECT_NBEHIND] == 0.0, "an outlier is used and counted");
    bool scaled = true;
    for (int k = 0; k < SBA_RESECT_COST; ++k) scaled = scaled && std::fabs(out[k] - 0.25 * plain[k]) <= 1e-12 * std::fabs(plain[k]);
    expect(scaled, "an outlier's H and g carry w = delta / sqrt(s)");
    expect(std::fabs(out[SBA_RESECT_COST] - 0.5 * (7.0 / 16.0) * s) <= 1e-12 * s, "an outlier's cost is 1/2 rho(s)");
    // what takes no part adds exact zeros whatever it holds: NaN rows, and the padding observation's s = 0 under any delta
    for (double delta : {1e-300, 1.0, 1e300}) {
      sba::landmark_register_robust_fill(delta, &L);
      std::vector<double> acc(SBA_RESECT_SIZE, 0.0);
      sba::landmark_register_accumulate_robust(P, L.delta, L.delta2, std::vector<double>{nan, inf, 1.0}.data(), std::vector<double>(6, nan).data(),
                                               std::vector<double>(3, nan).data(), nan, false, acc.data());
      expect(all_zero(acc), "a NaN row that takes no part adds zeros");
      sba::landmark_register_accumulate_robust(P, L.delta, L.delta2, X.data(), S.data(), y.data(), nz[0], false, acc.data());
      expect(all_zero(acc), "a row out of range adds zeros");
      // a live observation whose factor fails at this pose: s = 0, not used
      sba::landmark_register_accumulate_robust(P, L.delta, L.delta2, X.data(), std::vector<double>{-0.04, -0.09, -0.01, 0, 0, 0}.data(), y.data(), 0.0,
                                               true, acc.data());
      expect(all_zero(acc), "a failed factor adds zeros");
    }
    // behind at this pose: used, counted behind
    const std::vector<double> yb = {-y[0], -y[1], -y[2]};
    sba::landmark_register_robust_fill(2.0, &L);
    std::vector<double> bh(SBA_RESECT_SIZE, 0.0);
    sba::landmark_register_accumulate_robust(P, L.delta, L.delta2, X.data(), S.data(), yb.data(), nz[0], true, bh.data());
    expect(bh[SBA_RESECT_SW] == 1.0 && bh[SBA_RESECT_NBEHIND] == 1.0 && sba::resect_row_finite(bh.data()), "a row behind is used and counted behind");
  }
  using sba::landmark_register_check_robust;
  expect(landmark_register_check_robust(2.0, 4.0) == nullptr && landmark_register_check_robust(2.0, 1.0) == nullptr, "a gate up to delta^2 is fine");
  expect(landmark_register_check_robust(2.0, 4.04) && landmark_register_check_robust(2.0, inf) && landmark_register_check_robust(2.0, nan),
         "a gate above delta^2 is refused");
  expect(landmark_register_check_robust(0.0, 1.0) && landmark_register_check_robust(-1.0, 1.0) && landmark_register_check_robust(inf, 1.0) &&
             landmark_register_check_robust(nan, 1.0), "huber_delta must be finite and > 0");
  if (failures) return 1;
  std::printf("robust landmark registration host checks passed\n");
  return 0;
}
