// TEST PROGRAM (tests/ only; built with g++ -fsanitize=address,undefined and run as a child process by
// tests/test_landmark_edit_host_cpu.py): the host and device share of the landmark map's edits (csrc/sba_landmarks_edit.hpp) with
// exact-sized heap buffers -- the score in its stated order, one landmark of every class and the order the classes are tested in,
// and the option, index and size checks at their limits.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../spherical_bundle_adjuster_amd/csrc/sba_landmarks_edit.hpp"

namespace {

int failures = 0;
void expect(bool ok, const char* what) {
  if (!ok) { std::printf("FAILED: %s\n", what); ++failures; }
}

int cls(const std::vector<double>& X, const std::vector<double>& S, unsigned count, unsigned char mask, double max_score, unsigned min_count) {
  return sba::landmark_prune_class(X.data(), S.data(), count, mask, max_score, min_count);
}

}  // namespace

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const std::vector<double> X = {1.0, -2.0, 4.0}, S = {0.04, 0.09, 0.01, 0.005, -0.0025, 0.0075};
  const double score = sba::landmark_score(X.data(), S.data());
  expect(score == ((0.04 + 0.09) + 0.01) / ((1.0 * 1.0 + -2.0 * -2.0) + 4.0 * 4.0), "the score in its stated order");
  const std::vector<double> zero = {0.0, 0.0, 0.0}, none = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  expect(sba::landmark_score(zero.data(), S.data()) == inf, "X = 0: +inf");
  expect(std::isnan(sba::landmark_score(zero.data(), none.data())), "X = 0 without a covariance: NaN");
  expect(std::isnan(sba::landmark_score(std::vector<double>{1.0, nan, 0.0}.data(), S.data())), "a NaN goes through");
  // one landmark of every class, and the order
  expect(cls(X, S, 0, 1, inf, 0) == sba::LANDMARK_KEPT, "no cut: kept");
  expect(cls(X, S, 0, 1, score, 0) == sba::LANDMARK_KEPT, "a score equal to the cut is kept");
  expect(cls(X, S, 0, 1, std::nextafter(score, 0.0), 0) == sba::LANDMARK_UNCERTAIN, "a score above the cut");
  expect(cls(X, S, 1, 1, inf, 2) == sba::LANDMARK_UNOBSERVED && cls(X, S, 2, 1, inf, 2) == sba::LANDMARK_KEPT, "count against min_count");
  expect(cls(X, S, 5, 0, inf, 0) == sba::LANDMARK_MASKED && cls(X, S, 5, 255, inf, 0) == sba::LANDMARK_KEPT, "the mask byte");
  expect(cls({1.0, nan, 4.0}, S, 0, 0, 0.0, 9) == sba::LANDMARK_INVALID, "NaN in X comes first");
  expect(cls({inf, 0.0, 0.0}, S, 5, 1, inf, 0) == sba::LANDMARK_INVALID, "an infinite coordinate");
  expect(cls(X, {0.04, 0.09, 0.01, 0.005, inf, 0.0075}, 5, 1, inf, 0) == sba::LANDMARK_INVALID, "inf in Sigma");
  expect(cls(X, {0.04, -0.09, 0.01, 0.0, 0.0, 0.0}, 5, 1, inf, 0) == sba::LANDMARK_INVALID, "a negative variance");
  expect(cls(X, {0.04, 0.09, 0.01, -0.005, -0.0025, -0.0075}, 5, 1, inf, 0) == sba::LANDMARK_KEPT, "negative covariances are fine");
  expect(cls(X, S, 0, 0, std::nextafter(score, 0.0), 9) == sba::LANDMARK_UNCERTAIN, "uncertain before unobserved and masked");
  expect(cls(X, S, 0, 0, inf, 9) == sba::LANDMARK_UNOBSERVED, "unobserved before masked");
  expect(cls(zero, S, 5, 1, inf, 0) == sba::LANDMARK_KEPT && cls(zero, S, 5, 1, 1e300, 0) == sba::LANDMARK_UNCERTAIN, "X = 0: +inf <= +inf only");
  expect(cls(zero, none, 5, 1, inf, 0) == sba::LANDMARK_UNCERTAIN, "a NaN score is uncertain at every cut");
  // the checks
  expect(sba::landmark_check_max_score(0.0) == nullptr && sba::landmark_check_max_score(1e-3) == nullptr &&
             sba::landmark_check_max_score(inf) == nullptr && sba::landmark_check_max_score(-1e-300) && sba::landmark_check_max_score(-inf) &&
             sba::landmark_check_max_score(nan), "max_score");
  {
    const std::vector<int64_t> ok = {9, 0, 3, 3, 2}, neg = {0, -1, 3}, top = {0, 10, 3}, big = {0, std::numeric_limits<int64_t>::max()},
                               low = {std::numeric_limits<int64_t>::min()};
    expect(sba::landmark_check_gather_index(ok.data(), ok.size(), 10) == nullptr, "idx: any order, repeats");
    expect(sba::landmark_check_gather_index(neg.data(), neg.size(), 10) != nullptr, "idx: negative");
    expect(sba::landmark_check_gather_index(top.data(), top.size(), 10) != nullptr, "idx: == n");
    expect(sba::landmark_check_gather_index(big.data(), big.size(), 10) != nullptr && sba::landmark_check_gather_index(low.data(), low.size(), 10) != nullptr,
           "idx: the limits of int64");
    expect(sba::landmark_check_gather_index(ok.data(), ok.size(), 0) != nullptr, "idx: an empty map has no rows");
    expect(sba::landmark_check_gather_index(nullptr, 0, 10) == nullptr && sba::landmark_check_gather_index(ok.data(), 0, 0) == nullptr, "idx: empty");
    expect(sba::landmark_check_gather_index(nullptr, 3, 10) != nullptr, "idx: null with m > 0");
  }
  {
    const size_t top = static_cast<size_t>(-1);
    expect(sba::landmark_check_sizes(0, 0) == nullptr && sba::landmark_check_sizes(10000000, 10000000) == nullptr, "sizes: plain");
    expect(sba::landmark_check_sizes(top, 1) != nullptr && sba::landmark_check_sizes(1, top) != nullptr && sba::landmark_check_sizes(top, top) != nullptr &&
               sba::landmark_check_sizes(top / 2, top / 2 + 2) != nullptr && sba::landmark_check_sizes(0, top / 64) != nullptr, "sizes: overflow");
    expect(sba::landmark_check_sizes(top / 256, 0) == nullptr && sba::landmark_check_sizes(top / 256, 1) != nullptr, "sizes: the limit");
  }
  if (failures) return 1;
  std::printf("landmark edit host checks passed\n");
  return 0;
}
