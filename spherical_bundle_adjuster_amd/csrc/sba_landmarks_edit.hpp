// Host and device share of the landmark map's edits (include/sba_hip.h: sba_landmarks_scores / _prune / _append / _gather):
// the score of one landmark, the class a prune puts it in, and the option, index and size checks of the entry points.
// HIP-free; the kernels are in sba_landmarks_edit.hip, the entry points in sba_landmarks.cpp.  Per landmark X with covariance
// Sigma (rows xx, yy, zz, xy, xz, yz) and `count` accepted observations:
//
//   score = ((Sigma_xx + Sigma_yy) + Sigma_zz) / ((X.x X.x + X.y X.y) + X.z X.z)        trace Sigma / X . X of sba_structure.hpp
//
// in exactly this order, in f64, without contraction: the division is correctly rounded on both sides, so float64 arithmetic in
// the same order reproduces the score to the bit.  Nothing is special-cased: a non-finite input gives a non-finite score, X = 0
// gives +inf or NaN.  The classes of a prune, tested in this order: INVALID (a non-finite entry of X or Sigma, a negative
// variance), UNCERTAIN (!(score <= max_score)), UNOBSERVED (count < min_count), MASKED (the caller's mask byte is 0), KEPT.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "sba_rotation.hpp"

#if defined(__clang__)
#pragma STDC FP_CONTRACT OFF
#endif

namespace sba {

// The class of a landmark in a prune, tested in this order.
enum {
  LANDMARK_INVALID = 0,
  LANDMARK_UNCERTAIN = 1,
  LANDMARK_UNOBSERVED = 2,
  LANDMARK_MASKED = 3,
  LANDMARK_KEPT = 4,
  LANDMARK_PRUNE_CLASSES = 5
};

SBA_HD inline double landmark_score(const double X[3], const double Sg[6]) {
  const double tr = (Sg[0] + Sg[1]) + Sg[2];
  const double xx = (X[0] * X[0] + X[1] * X[1]) + X[2] * X[2];
  return tr / xx;
}

// mask_byte: the caller's mask entry, non-zero when there is no mask.
SBA_HD inline int landmark_prune_class(const double X[3], const double Sg[6], unsigned int count, unsigned char mask_byte, double max_score,
                                       unsigned int min_count) {
  bool ok = std::isfinite(X[0]) && std::isfinite(X[1]) && std::isfinite(X[2]);
  for (int k = 0; k < 6; ++k) ok = ok && std::isfinite(Sg[k]);
  ok = ok && !(Sg[0] < 0.0) && !(Sg[1] < 0.0) && !(Sg[2] < 0.0);
  if (!ok) return LANDMARK_INVALID;
  if (!(landmark_score(X, Sg) <= max_score)) return LANDMARK_UNCERTAIN;
  if (count < min_count) return LANDMARK_UNOBSERVED;
  if (mask_byte == 0) return LANDMARK_MASKED;
  return LANDMARK_KEPT;
}

// Option, index and size checks of the entry points: nullptr = fine, otherwise what is wrong (SBA_ERR_INVALID_ARG).
inline const char* landmark_check_max_score(double max_score) {
  return max_score >= 0.0 ? nullptr : "max_score must be >= 0 (+inf: no cut)";
}
// Rows of a gather: any order, repeats allowed, every one of them on the map.
inline const char* landmark_check_gather_index(const int64_t* idx, size_t m, size_t n) {
  if (m > 0 && !idx) return "null index array";
  for (size_t j = 0; j < m; ++j)
    if (idx[j] < 0 || static_cast<uint64_t>(idx[j]) >= n) return "idx out of range";
  return nullptr;
}
// A map of n + n_add landmarks, or m gathered rows: every byte count of the ten planes, the rows and the scratch fits a size_t.
inline const char* landmark_check_sizes(size_t n, size_t n_add) {
  const size_t limit = static_cast<size_t>(-1) / 256;
  return n <= limit && n_add <= limit - n ? nullptr : "too many landmarks: the byte counts overflow";
}

}  // namespace sba

#if defined(__clang__)
#pragma STDC FP_CONTRACT DEFAULT
#endif
