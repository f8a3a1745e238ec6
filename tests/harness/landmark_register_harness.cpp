// TEST HARNESS (tests/ only): the host and device share of the joint registration (csrc/sba_landmarks_register.hpp,
// header-only, no HIP) compiled for the CPU: the freeze of one observation, one observation into the sums of the reduce pass,
// the write-back of one observation, and the option check of the entry points.
#include "../../spherical_bundle_adjuster_amd/csrc/sba_landmarks_register.hpp"

// noise, cls per observation at the freeze pose.
extern "C" void landmark_register_harness_freeze(long long n, const double* X, const double* cov, const double* y, const double* rot_ref,
                                                 const double* tran_ref, double bearing_sigma, double* noise, int* cls) {
  sba::LandmarkRegisterParams P;
  sba::landmark_register_fill(static_cast<unsigned long long>(n), static_cast<unsigned long long>(n), rot_ref, tran_ref, nullptr, bearing_sigma,
                              INFINITY, &P);
  for (long long i = 0; i < n; ++i) cls[i] = sba::landmark_register_noise(P, X + 3 * i, cov + 6 * i, y + 3 * i, noise + i);
}

// out: H row-major (36), g (6), cost, n_used, n_behind -- one set of lane sums over all rows, expanded by resect_expand_row.
extern "C" void landmark_register_harness_eval(long long n, const double* X, const double* cov, const double* y, const double* noise,
                                               const double* rot, const double* tran, double* out) {
  sba::LandmarkRegisterParams P;
  sba::landmark_register_fill(static_cast<unsigned long long>(n), static_cast<unsigned long long>(n), rot, tran, nullptr, 0.0, INFINITY, &P);
  double acc[SBA_RESECT_SIZE] = {0};
  for (long long i = 0; i < n; ++i)
    sba::landmark_register_accumulate(P, X + 3 * i, cov + 6 * i, y + 3 * i, noise[i], sba::landmark_register_live(noise[i]), acc);
  sba_normal_eq ne;
  double n_behind = 0.0;
  sba::resect_expand_row(acc, &ne, &n_behind);
  for (int k = 0; k < 36; ++k) out[k] = ne.H[k];
  for (int k = 0; k < 6; ++k) out[36 + k] = ne.g[k];
  out[42] = ne.cost; out[43] = ne.sum_w; out[44] = n_behind;
}

// Xo, So: the posterior where the class is LANDMARK_FUSED, the prior elsewhere (what the kernels leave in the planes).
extern "C" void landmark_register_harness_apply(long long n, const double* X, const double* cov, const double* y, const double* noise,
                                                const double* rot, const double* tran, const double* pose_cov, double gate, double* Xo,
                                                double* So, double* chi2, int* cls) {
  sba::LandmarkRegisterParams P;
  sba::landmark_register_fill(static_cast<unsigned long long>(n), static_cast<unsigned long long>(n), rot, tran, pose_cov, 0.0, gate, &P);
  for (long long i = 0; i < n; ++i) {
    double xo[3], so[6];
    cls[i] = sba::landmark_register_one(P, X + 3 * i, cov + 6 * i, y + 3 * i, noise[i], xo, so, chi2 + i);
    const bool fused = cls[i] == sba::LANDMARK_FUSED;
    for (int k = 0; k < 3; ++k) Xo[3 * i + k] = fused ? xo[k] : X[3 * i + k];
    for (int k = 0; k < 6; ++k) So[6 * i + k] = fused ? so[k] : cov[6 * i + k];
  }
}

// returns 1 when accepted
extern "C" int landmark_register_harness_check_loss(double huber_delta) { return sba::landmark_register_check_loss(huber_delta) == nullptr ? 1 : 0; }
