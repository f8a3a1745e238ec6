// TEST PROGRAM (tests/ only; built with g++ -fsanitize=address,undefined and run as a child process by
// tests/test_landmark_register_host_cpu.py): the host and device share of the joint registration
// (csrc/sba_landmarks_register.hpp) with exact-sized heap buffers -- the state of a pass in both frames, the freeze of every
// class and every skipped kind, the marker rules of the sums, the write-back's classes and the posterior's defining properties,
// and the option check.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../spherical_bundle_adjuster_amd/csrc/sba_landmarks_register.hpp"

namespace {

int failures = 0;
void expect(bool ok, const char* what) {
  if (!ok) { std::printf("FAILED: %s\n", what); ++failures; }
}

struct Out {
  std::vector<double> X = std::vector<double>(3, -7.0), S = std::vector<double>(6, -7.0), chi2 = std::vector<double>(1, -7.0);
  int cls = -1;
};

Out apply(const sba::LandmarkRegisterParams& P, const std::vector<double>& X, const std::vector<double>& S, const std::vector<double>& y, double noise) {
  Out o;
  o.cls = sba::landmark_register_one(P, X.data(), S.data(), y.data(), noise, o.X.data(), o.S.data(), o.chi2.data());
  return o;
}

int freeze(const sba::LandmarkRegisterParams& P, const std::vector<double>& X, const std::vector<double>& S, const std::vector<double>& y, double* noise) {
  std::vector<double> nz(1, -7.0);
  const int cls = sba::landmark_register_noise(P, X.data(), S.data(), y.data(), nz.data());
  *noise = nz[0];
  return cls;
}

}  // namespace

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const std::vector<double> rot = {0.1, -0.2, 0.15}, tran = {0.3, -0.1, 0.2}, rot0 = {1e-9, 0.0, -2e-9};
  std::vector<double> pc(36, 0.0);
  for (int a = 0; a < 6; ++a) pc[7 * a] = a < 3 ? 4e-8 : 1e-6;
  pc[1] = pc[6] = 1e-8; pc[3 * 6 + 1] = pc[6 + 3] = -2e-8;
  const std::vector<double> X = {1.0, -2.0, 4.0}, S = {0.04, 0.09, 0.01, 0.005, -0.0025, 0.0075};
  for (int variant = 0; variant < 4; ++variant) {
    const std::vector<double>& w = (variant & 1) ? rot0 : rot;
    const double bs = (variant & 2) ? 1e-3 : 0.0;
    sba::LandmarkRegisterParams P;
    sba::landmark_register_fill(1, 1, w.data(), tran.data(), pc.data(), bs, inf, &P);
    expect(P.small_angle == (variant & 1) && P.cov[0] == pc[0] && P.cov[6] == pc[7] && P.cov[20] == pc[35] && P.cov[1] == pc[1], "fill: frame and Sigma_c");
    // the bearing the landmark is seen along, a little off: c = Rn X + t, y = -c
    std::vector<double> y(3);
    for (int k = 0; k < 3; ++k) y[k] = -(P.Rn[3 * k] * X[0] + P.Rn[3 * k + 1] * X[1] + P.Rn[3 * k + 2] * X[2] + P.t[k]);
    y[0] += 0.02; y[1] -= 0.01;
    double nz = -7.0;
    expect(freeze(P, X, S, y, &nz) == sba::LANDMARK_LIVE && nz >= 0.0 && !std::signbit(nz) && (bs > 0.0) == (nz > 0.0), "a plain observation takes part");
    expect(sba::landmark_register_live(nz), "its noise says so");
    // behind at the freeze: the sign bit, also on a zero
    const std::vector<double> yb = {-y[0], -y[1], -y[2]};
    double nb = -7.0;
    expect(freeze(P, X, S, yb, &nb) == sba::LANDMARK_BEHIND && std::signbit(nb) && std::fabs(nb) == nz, "behind at the freeze: -s^2, the sign bit set");
    expect(!sba::landmark_register_live(nb), "behind at the freeze takes no part");
    // the skipped kinds
    double ns = -7.0;
    expect(freeze(P, X, {inf, inf, inf, 0, 0, 0}, y, &ns) == sba::LANDMARK_SKIPPED && std::isnan(ns), "the degenerate row of the structure is skipped");
    expect(freeze(P, {1.0, nan, 4.0}, S, y, &ns) == sba::LANDMARK_SKIPPED && std::isnan(ns), "NaN in X is skipped");
    expect(freeze(P, X, {0.04, 0.09, nan, 0.005, -0.0025, 0.0075}, y, &ns) == sba::LANDMARK_SKIPPED && std::isnan(ns), "NaN in Sigma is skipped");
    expect(freeze(P, X, S, {0.0, 0.0, 0.0}, &ns) == sba::LANDMARK_SKIPPED && std::isnan(ns), "a zero bearing is skipped");
    expect(freeze(P, X, S, {inf, 0.0, 0.0}, &ns) == sba::LANDMARK_SKIPPED && std::isnan(ns), "an infinite bearing is skipped");
    if (bs == 0.0) expect(freeze(P, X, {-0.04, -0.09, -0.01, 0, 0, 0}, y, &ns) == sba::LANDMARK_SKIPPED, "a negative variance without bearing noise is skipped");
    expect(!sba::landmark_register_live(ns), "skipped takes no part");
    // the sums: an observation that takes no part adds exact zeros whatever it holds; one that does adds a positive semi-definite block
    std::vector<double> acc(SBA_RESECT_SIZE, 0.0);
    sba::landmark_register_accumulate(P, std::vector<double>{nan, inf, 1.0}.data(), std::vector<double>(6, nan).data(), std::vector<double>(3, nan).data(), nan, false, acc.data());
    bool zeros = true;
    for (double v : acc) zeros = zeros && v == 0.0;
    expect(zeros, "an observation that takes no part adds zeros");
    sba::landmark_register_accumulate(P, X.data(), S.data(), y.data(), nz, true, acc.data());
    expect(acc[SBA_RESECT_SW] == 1.0 && acc[SBA_RESECT_NBEHIND] == 0.0 && acc[SBA_RESECT_NOUT] == 0.0 && acc[SBA_RESECT_COST] > 0.0, "one observation entered");
    expect(sba::resect_row_finite(acc.data()) && acc[SBA_RESECT_H] > 0.0 && acc[SBA_RESECT_H + 20] > 0.0, "its block has a positive diagonal");
    // a live observation whose factor fails at this pose adds zeros and is not counted
    std::vector<double> acc2(SBA_RESECT_SIZE, 0.0);
    sba::landmark_register_accumulate(P, X.data(), std::vector<double>{-0.04, -0.09, -0.01, 0, 0, 0}.data(), y.data(), 0.0, true, acc2.data());
    zeros = true;
    for (double v : acc2) zeros = zeros && v == 0.0;
    expect(zeros, "a failed factor adds zeros");
    // the write-back
    const Out f = apply(P, X, S, y, nz);
    expect(f.cls == sba::LANDMARK_FUSED && std::isfinite(f.chi2[0]) && f.chi2[0] >= 0.0, "a plain observation is fused");
    expect(std::fabs(f.chi2[0] - 2.0 * acc[SBA_RESECT_COST]) <= 1e-12 * f.chi2[0], "chi2 is twice its cost");
    const double m2 = f.S[0] * f.S[1] - f.S[3] * f.S[3];
    const double m3 = f.S[0] * (f.S[1] * f.S[2] - f.S[5] * f.S[5]) - f.S[3] * (f.S[3] * f.S[2] - f.S[5] * f.S[4]) + f.S[4] * (f.S[3] * f.S[5] - f.S[1] * f.S[4]);
    expect(f.S[0] > 0.0 && m2 > 0.0 && m3 > 0.0, "the posterior covariance is positive definite");
    // without a pose covariance the posterior is the conditional one: no variance above the prior's, none above the joint one's
    sba::LandmarkRegisterParams Pz = P;
    for (double& v : Pz.cov) v = 0.0;
    const Out c = apply(Pz, X, S, y, nz);
    expect(c.cls == sba::LANDMARK_FUSED && c.S[0] <= S[0] && c.S[1] <= S[1] && c.S[2] <= S[2], "conditional: no variance grows");
    expect(c.S[0] <= f.S[0] && c.S[1] <= f.S[1] && c.S[2] <= f.S[2] && c.X == f.X && c.chi2 == f.chi2, "the pose covariance only adds variance");
    sba::LandmarkRegisterParams Pg = P;
    Pg.chi2_gate = f.chi2[0] * 0.5;
    expect(apply(Pg, X, S, y, nz).cls == sba::LANDMARK_GATED && apply(Pg, X, S, y, nz).chi2[0] == f.chi2[0], "above the gate: gated, chi2 written");
    const Out b = apply(P, X, S, yb, nb);
    expect(b.cls == sba::LANDMARK_BEHIND && std::isfinite(b.chi2[0]), "marked behind: behind, chi2 written");
    expect(apply(P, X, S, yb, nz).cls == sba::LANDMARK_BEHIND, "behind at the solution only: behind");
    expect(apply(P, X, S, y, -nz).cls == sba::LANDMARK_BEHIND, "marked behind at the freeze, in front at the solution: behind");
    const Out sk = apply(P, {nan, 1.0, inf}, std::vector<double>(6, nan), {0.0, 0.0, 0.0}, nan);
    expect(sk.cls == sba::LANDMARK_SKIPPED && std::isnan(sk.chi2[0]), "marked skipped: skipped, chi2 NaN");
    const Out sf = apply(P, X, {-0.04, -0.09, -0.01, 0, 0, 0}, y, 0.0);
    expect(sf.cls == sba::LANDMARK_SKIPPED && std::isnan(sf.chi2[0]), "a factor that fails at the solution: skipped");
  }
  expect(sba::landmark_register_check_loss(0.0) == nullptr && sba::landmark_register_check_loss(-0.0) == nullptr &&
             sba::landmark_register_check_loss(1.0) && sba::landmark_register_check_loss(-1.0) && sba::landmark_register_check_loss(nan), "huber_delta");
  if (failures) return 1;
  std::printf("landmark registration host checks passed\n");
  return 0;
}
