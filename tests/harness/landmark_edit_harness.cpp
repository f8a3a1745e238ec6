// TEST HARNESS (tests/ only): the host and device share of the landmark map's edits (csrc/sba_landmarks_edit.hpp, header-only, no
// HIP) compiled for the CPU: the score and the class of a prune per landmark, the very functions the kernels call, and the option,
// index and size checks of the entry points.
#include "../../spherical_bundle_adjuster_amd/csrc/sba_landmarks_edit.hpp"

extern "C" void landmark_edit_harness_scores(long long n, const double* X, const double* cov, double* out) {
  for (long long i = 0; i < n; ++i) out[i] = sba::landmark_score(X + 3 * i, cov + 6 * i);
}

// mask: n bytes or null (none)
extern "C" void landmark_edit_harness_classes(long long n, const double* X, const double* cov, const uint32_t* counts, const uint8_t* mask,
                                              double max_score, uint32_t min_count, int* cls) {
  for (long long i = 0; i < n; ++i)
    cls[i] = sba::landmark_prune_class(X + 3 * i, cov + 6 * i, counts[i], mask ? mask[i] : static_cast<unsigned char>(1), max_score, min_count);
}

// return 1 when accepted
extern "C" int landmark_edit_harness_check_max_score(double v) { return sba::landmark_check_max_score(v) == nullptr ? 1 : 0; }

extern "C" int landmark_edit_harness_check_gather_index(const int64_t* idx, size_t m, size_t n) {
  return sba::landmark_check_gather_index(idx, m, n) == nullptr ? 1 : 0;
}

extern "C" int landmark_edit_harness_check_sizes(size_t n, size_t n_add) { return sba::landmark_check_sizes(n, n_add) == nullptr ? 1 : 0; }
