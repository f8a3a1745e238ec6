// TEST PROGRAM (tests/ only; built with g++ -fsanitize=address,undefined and run as a child process by
// tests/test_landmark_register_hampel_host_cpu.py): the host and device share of the Hampel joint registration
// (csrc/sba_landmarks_register_hampel.hpp) with exact-sized heap buffers over planted rows -- NaN rows, the padding observation
// with s = 0, one row behind, one observation in each of the loss's four rows, the Huber limit b = c = +inf -- and the option check.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../spherical_bundle_adjuster_amd/csrc/sba_landmarks_register_hampel.hpp"

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

bool all_finite(const std::vector<double>& v) {
  bool f = true;
  for (double x : v) f = f && std::isfinite(x);
  return f;
}

}  // namespace

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const int N = sba::SBA_HAMPEL_COUNT, NREJ = sba::SBA_HAMPEL_NREJ;
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
    std::vector<double> plain(N, 0.0);
    sba::landmark_register_accumulate(P, X.data(), S.data(), y.data(), nz[0], true, plain.data());
    const double s = 2.0 * plain[SBA_RESECT_COST], r = std::sqrt(s);
    expect(s > 0.0 && std::isfinite(s), "its chi2 is positive");
    sba::LandmarkRegisterHampel L;
    // row 1: sqrt(s) below a -> the non-robust sums to the bit
    sba::landmark_register_hampel_fill(2.0 * r, 4.0 * r, 8.0 * r, &L);
    std::vector<double> in(N, 0.0);
    sba::landmark_register_accumulate_hampel(P, L, X.data(), S.data(), y.data(), nz[0], true, in.data());
    expect(in == plain, "an inlier adds the non-robust sums, bit for bit");
    expect(in[SBA_RESECT_NOUT] == 0.0 && in[SBA_RESECT_SW] == 1.0 && in[NREJ] == 0.0, "an inlier is used, no outlier, not rejected");
    // rows 2, 3, 4: (a, b, c) in units of sqrt(s), and the weight and rho / s they give
    const double cases[3][5] = {{0.25, 2.0, 4.0, 0.25, 7.0 / 16.0}, {0.25, 0.5, 2.0, 1.0 / 6.0, 19.0 / 48.0}, {0.125, 0.25, 0.5, 0.0, 5.0 / 64.0}};
    for (int q = 0; q < 3; ++q) {
      sba::landmark_register_hampel_fill(cases[q][0] * r, cases[q][1] * r, cases[q][2] * r, &L);
      std::vector<double> out(N, 0.0);
      sba::landmark_register_accumulate_hampel(P, L, X.data(), S.data(), y.data(), nz[0], true, out.data());
      expect(out[SBA_RESECT_NOUT] == 1.0 && out[SBA_RESECT_SW] == 1.0 && out[SBA_RESECT_NBEHIND] == 0.0, "a downweighted observation is used and counted");
      expect(out[NREJ] == (q == 2 ? 1.0 : 0.0), "only an observation beyond c is rejected");
      bool scaled = true;
      for (int k = 0; k < SBA_RESECT_COST; ++k) scaled = scaled && std::fabs(out[k] - cases[q][3] * plain[k]) <= 1e-12 * std::fabs(plain[k]);
      expect(scaled, "H and g carry the row's weight");
      if (q == 2) {
        bool zero = true;
        for (int k = 0; k < SBA_RESECT_COST; ++k) zero = zero && out[k] == 0.0;
        expect(zero, "a rejected observation adds exact zeros to H and g");
      }
      expect(std::fabs(out[SBA_RESECT_COST] - 0.5 * cases[q][4] * s) <= 1e-12 * s, "the cost is 1/2 rho(s)");
    }
    // the Huber limit: b = c = +inf is the robust pass's arithmetic, and the unselected rows' inf - inf reaches no sum
    for (double a : {2.0 * r, 0.25 * r, 1e-3 * r}) {
      sba::landmark_register_hampel_fill(a, inf, inf, &L);
      sba::LandmarkRegisterRobust Hu;
      sba::landmark_register_robust_fill(a, &Hu);
      std::vector<double> hm(N, 0.0), hu(N, 0.0);
      sba::landmark_register_accumulate_hampel(P, L, X.data(), S.data(), y.data(), nz[0], true, hm.data());
      sba::landmark_register_accumulate_robust(P, Hu.delta, Hu.delta2, X.data(), S.data(), y.data(), nz[0], true, hu.data());
      expect(all_finite(hm) && hm[NREJ] == 0.0, "the Huber limit stays finite and rejects nothing");
      expect(hm == hu, "the Huber limit adds the robust sums, bit for bit");
    }
    // what takes no part adds exact zeros whatever it holds: NaN rows, and the padding observation's s = 0 under any thresholds
    for (double a : {1e-300, 1.0, 1e300}) {
      for (int limit = 0; limit < 2; ++limit) {
        sba::landmark_register_hampel_fill(a, limit ? inf : 2.0 * a, limit ? inf : 4.0 * a, &L);
        std::vector<double> acc(N, 0.0);
        sba::landmark_register_accumulate_hampel(P, L, std::vector<double>{nan, inf, 1.0}.data(), std::vector<double>(6, nan).data(),
                                                 std::vector<double>(3, nan).data(), nan, false, acc.data());
        expect(all_zero(acc), "a NaN row that takes no part adds zeros");
        sba::landmark_register_accumulate_hampel(P, L, X.data(), S.data(), y.data(), nz[0], false, acc.data());
        expect(all_zero(acc), "a row out of range adds zeros");
        // a live observation whose factor fails at this pose: s = 0, not used
        sba::landmark_register_accumulate_hampel(P, L, X.data(), std::vector<double>{-0.04, -0.09, -0.01, 0, 0, 0}.data(), y.data(), 0.0, true,
                                                 acc.data());
        expect(all_zero(acc), "a failed factor adds zeros");
      }
    }
    // behind at this pose: used, counted behind
    const std::vector<double> yb = {-y[0], -y[1], -y[2]};
    sba::landmark_register_hampel_fill(2.0, 4.0, 8.0, &L);
    std::vector<double> bh(N, 0.0);
    sba::landmark_register_accumulate_hampel(P, L, X.data(), S.data(), yb.data(), nz[0], true, bh.data());
    expect(bh[SBA_RESECT_SW] == 1.0 && bh[SBA_RESECT_NBEHIND] == 1.0 && all_finite(bh), "a row behind is used and counted behind");
  }
  using sba::landmark_register_check_hampel;
  expect(landmark_register_check_hampel(2.0, 4.0, 8.0, 4.0) == nullptr && landmark_register_check_hampel(2.0, inf, inf, 1.0) == nullptr,
         "finite a < b < c and the Huber limit are fine");
  expect(landmark_register_check_hampel(2.0, 4.0, 8.0, 4.04) && landmark_register_check_hampel(2.0, 4.0, 8.0, inf) &&
             landmark_register_check_hampel(2.0, 4.0, 8.0, nan), "a gate above a^2 is refused");
  expect(landmark_register_check_hampel(0.0, 4.0, 8.0, 1.0) && landmark_register_check_hampel(inf, inf, inf, 1.0) &&
             landmark_register_check_hampel(nan, 4.0, 8.0, 1.0), "a must be finite and > 0");
  expect(landmark_register_check_hampel(2.0, nan, 8.0, 1.0) && landmark_register_check_hampel(2.0, 4.0, nan, 1.0), "NaN thresholds are refused");
  expect(landmark_register_check_hampel(2.0, 2.0, 8.0, 1.0) && landmark_register_check_hampel(2.0, 1.0, 8.0, 1.0) &&
             landmark_register_check_hampel(2.0, 4.0, 4.0, 1.0) && landmark_register_check_hampel(2.0, 4.0, 3.0, 1.0), "a < b < c is demanded");
  expect(landmark_register_check_hampel(2.0, 4.0, inf, 1.0) && landmark_register_check_hampel(2.0, inf, 8.0, 1.0) &&
             landmark_register_check_hampel(2.0, -inf, -inf, 1.0), "exactly one infinite threshold, or -inf, is refused");
  if (failures) return 1;
  std::printf("Hampel landmark registration host checks passed\n");
  return 0;
}
