// TEST HARNESS (tests/ only): the host and device share of the landmark map (csrc/sba_landmarks.hpp, header-only, no HIP)
// compiled for the CPU: the state of a fusion pass, the per-observation update the kernels call, and the option and index checks
// of sba_landmarks_fuse.
#include "../../spherical_bundle_adjuster_amd/csrc/sba_landmarks.hpp"

// One bearing per landmark.  Xo, So: the posterior where the class is LANDMARK_FUSED, the prior elsewhere (what the kernels leave
// in the planes); chi2 and cls per observation.  pose_cov: 36 doubles or null.
extern "C" void landmark_fusion_harness_fuse(long long n, const double* X, const double* cov, const double* y, const double* rot,
                                             const double* tran, const double* pose_cov, double bearing_sigma, double gate, double* Xo,
                                             double* So, double* chi2, int* cls) {
  sba::LandmarkFuseParams P;
  sba::landmark_fuse_fill(static_cast<unsigned long long>(n), static_cast<unsigned long long>(n), rot, tran, pose_cov, bearing_sigma, gate, &P);
  for (long long i = 0; i < n; ++i) {
    double xo[3], so[6];
    cls[i] = sba::landmark_fuse_one(P, X + 3 * i, cov + 6 * i, y + 3 * i, xo, so, chi2 + i);
    const bool fused = cls[i] == sba::LANDMARK_FUSED;
    for (int k = 0; k < 3; ++k) Xo[3 * i + k] = fused ? xo[k] : X[3 * i + k];
    for (int k = 0; k < 6; ++k) So[6 * i + k] = fused ? so[k] : cov[6 * i + k];
  }
}

// which: 0 cov_scale, 1 bearing_sigma, 2 chi2_gate; returns 1 when accepted
extern "C" int landmark_fusion_harness_check(int which, double value) {
  const char* why = which == 0 ? sba::resect_weight_check_scale(value)
                               : (which == 1 ? sba::resect_weight_check_sigma(value) : sba::landmark_check_gate(value));
  return why == nullptr ? 1 : 0;
}

extern "C" int landmark_fusion_harness_check_pose_cov(const double* c36) { return sba::landmark_check_pose_cov(c36) == nullptr ? 1 : 0; }

extern "C" int landmark_fusion_harness_check_index(const int64_t* idx, size_t m, size_t n) {
  return sba::landmark_check_index(idx, m, n) == nullptr ? 1 : 0;
}
