// TEST PROGRAM (tests/ only; built with g++ -fsanitize=address,undefined and run as a child process by
// tests/test_landmark_fusion_host_cpu.py): the host and device share of the landmark map (csrc/sba_landmarks.hpp) with
// exact-sized heap buffers -- the state of a pass with and without a pose covariance and in the small-angle frame, one observation
// of every class and every skipped kind, the posterior's defining properties, and the option and index checks at their limits.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../spherical_bundle_adjuster_amd/csrc/sba_landmarks.hpp"

namespace {

int failures = 0;
void expect(bool ok, const char* what) {
  if (!ok) { std::printf("FAILED: %s\n", what); ++failures; }
}

struct Out {
  std::vector<double> X = std::vector<double>(3, -7.0), S = std::vector<double>(6, -7.0), chi2 = std::vector<double>(1, -7.0);
  int cls = -1;
};

Out run(const sba::LandmarkFuseParams& P, const std::vector<double>& X, const std::vector<double>& S, const std::vector<double>& y) {
  Out o;
  o.cls = sba::landmark_fuse_one(P, X.data(), S.data(), y.data(), o.X.data(), o.S.data(), o.chi2.data());
  return o;
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
    sba::LandmarkFuseParams P;
    sba::landmark_fuse_fill(1, 1, w.data(), tran.data(), (variant & 2) ? pc.data() : nullptr, 1e-3, inf, &P);
    expect(P.small_angle == (variant & 1) && P.have_pose_cov == ((variant & 2) ? 1 : 0), "fill: frame and pose covariance flags");
    // the bearing the landmark is seen along, a little off: c = Rn X + t, y = -c
    std::vector<double> y(3);
    for (int k = 0; k < 3; ++k) y[k] = -(P.Rn[3 * k] * X[0] + P.Rn[3 * k + 1] * X[1] + P.Rn[3 * k + 2] * X[2] + P.t[k]);
    y[0] += 0.02; y[1] -= 0.01;
    const Out f = run(P, X, S, y);
    expect(f.cls == sba::LANDMARK_FUSED && std::isfinite(f.chi2[0]) && f.chi2[0] >= 0.0, "a plain observation is fused");
    // the posterior: no variance grows, and the covariance stays positive definite (leading minors)
    expect(f.S[0] <= S[0] && f.S[1] <= S[1] && f.S[2] <= S[2] && f.S[0] > 0.0, "no variance grows");
    const double m2 = f.S[0] * f.S[1] - f.S[3] * f.S[3];
    const double m3 = f.S[0] * (f.S[1] * f.S[2] - f.S[5] * f.S[5]) - f.S[3] * (f.S[3] * f.S[2] - f.S[5] * f.S[4]) + f.S[4] * (f.S[3] * f.S[5] - f.S[1] * f.S[4]);
    expect(m2 > 0.0 && m3 > 0.0, "the posterior covariance is positive definite");
    // fusing the same bearing again moves the landmark less than the first time
    const Out g = run(P, f.X, f.S, y);
    double d1 = 0.0, d2 = 0.0;
    for (int k = 0; k < 3; ++k) { d1 += (f.X[k] - X[k]) * (f.X[k] - X[k]); d2 += (g.X[k] - f.X[k]) * (g.X[k] - f.X[k]); }
    expect(g.cls == sba::LANDMARK_FUSED && d2 < d1, "a second look moves the landmark less");
    // gated
    sba::LandmarkFuseParams Pg = P;
    Pg.chi2_gate = f.chi2[0] * 0.5;
    expect(run(Pg, X, S, y).cls == sba::LANDMARK_GATED && run(Pg, X, S, y).chi2[0] == f.chi2[0], "above the gate: gated, chi2 written");
    // behind
    const std::vector<double> yb = {-y[0], -y[1], -y[2]};
    const Out b = run(P, X, S, yb);
    expect(b.cls == sba::LANDMARK_BEHIND && std::isfinite(b.chi2[0]), "a landmark behind the bearing: behind, chi2 written");
    // the skipped kinds
    expect(run(P, X, {inf, inf, inf, 0, 0, 0}, y).cls == sba::LANDMARK_SKIPPED, "the degenerate row of the structure is skipped");
    expect(run(P, {1.0, nan, 4.0}, S, y).cls == sba::LANDMARK_SKIPPED, "NaN in X is skipped");
    expect(run(P, {inf, inf, inf}, {inf, inf, inf, 0, 0, 0}, y).cls == sba::LANDMARK_SKIPPED, "an infinite landmark is skipped");
    const Out sn = run(P, X, {0.04, 0.09, nan, 0.005, -0.0025, 0.0075}, y);
    expect(sn.cls == sba::LANDMARK_SKIPPED && std::isnan(sn.chi2[0]), "NaN in Sigma is skipped, chi2 is NaN");
    const Out z = run(P, X, S, {0.0, 0.0, 0.0});
    expect(z.cls == sba::LANDMARK_SKIPPED && std::isnan(z.chi2[0]), "a zero bearing is skipped");
    sba::LandmarkFuseParams P0 = P;
    P0.bearing_sigma2 = 0.0;
    if (!(variant & 2)) expect(run(P0, X, {-0.04, -0.09, -0.01, 0, 0, 0}, y).cls == sba::LANDMARK_SKIPPED, "a negative variance without bearing noise is skipped");
  }
  expect(sba::landmark_check_gate(9.21) == nullptr && sba::landmark_check_gate(inf) == nullptr && sba::landmark_check_gate(0.0) &&
             sba::landmark_check_gate(-1.0) && sba::landmark_check_gate(nan), "chi2_gate");
  {
    expect(sba::landmark_check_pose_cov(nullptr) == nullptr && sba::landmark_check_pose_cov(pc.data()) == nullptr, "pose_cov: absent or symmetric");
    std::vector<double> bad = pc;
    bad[1] = std::nextafter(bad[1], 1.0);
    expect(sba::landmark_check_pose_cov(bad.data()) != nullptr, "pose_cov: asymmetric in the last bit");
    bad = pc; bad[35] = nan;
    expect(sba::landmark_check_pose_cov(bad.data()) != nullptr, "pose_cov: NaN");
    bad = pc; bad[14] = -1e-9;
    expect(sba::landmark_check_pose_cov(bad.data()) != nullptr, "pose_cov: negative diagonal");
    bad = pc; bad[4] = bad[24] = inf;
    expect(sba::landmark_check_pose_cov(bad.data()) != nullptr, "pose_cov: infinite");
  }
  {
    const std::vector<int64_t> ok = {0, 2, 3, 9}, rep = {0, 2, 2, 9}, desc = {0, 3, 2, 9}, neg = {-1, 2, 3, 9}, top = {0, 2, 3, 10};
    expect(sba::landmark_check_index(ok.data(), ok.size(), 10) == nullptr, "idx: strictly increasing and in range");
    expect(sba::landmark_check_index(rep.data(), rep.size(), 10) != nullptr, "idx: a repeat");
    expect(sba::landmark_check_index(desc.data(), desc.size(), 10) != nullptr, "idx: descending");
    expect(sba::landmark_check_index(neg.data(), neg.size(), 10) != nullptr, "idx: negative");
    expect(sba::landmark_check_index(top.data(), top.size(), 10) != nullptr, "idx: == n");
    expect(sba::landmark_check_index(ok.data(), ok.size(), 3) != nullptr, "idx: m > n");
    expect(sba::landmark_check_index(nullptr, 10, 10) == nullptr && sba::landmark_check_index(nullptr, 9, 10) != nullptr &&
               sba::landmark_check_index(nullptr, 11, 10) != nullptr, "dense: m must equal n");
    expect(sba::landmark_check_index(nullptr, 0, 0) == nullptr && sba::landmark_check_index(ok.data(), 0, 10) == nullptr, "empty");
  }
  if (failures) return 1;
  std::printf("landmark fusion host checks passed\n");
  return 0;
}
