// TEST HARNESS (tests/ only; built with g++ by tests/test_landmark_associate_cpu.py): the host and device share of the landmark
// map's association (csrc/sba_landmarks_associate.hpp) behind a C interface -- the claim key with its halves and its order, the
// claim of a list of accepted rows in the order given (the minimum of integers: any order gives the same slots), and the option,
// row and size checks.
#include <cstddef>
#include <cstdint>

#include "../../spherical_bundle_adjuster_amd/csrc/sba_landmarks_associate.hpp"

extern "C" {

unsigned long long landmark_associate_harness_key(float d0, unsigned int row) { return sba::associate_key(d0, row); }
unsigned int landmark_associate_harness_key_row(unsigned long long key) { return sba::associate_key_row(key); }
float landmark_associate_harness_key_distance(unsigned long long key) { return sba::associate_key_distance(key); }
int landmark_associate_harness_key_before(unsigned long long a, unsigned long long b) { return sba::associate_key_before(a, b) ? 1 : 0; }
unsigned long long landmark_associate_harness_unclaimed() { return sba::kAssociateUnclaimed; }

// slots [n], preset here; rows / landmarks / dist [count]: matcher-accepted rows in any order.  Returns the rows within the cut.
long long landmark_associate_harness_claim(size_t n, size_t count, const int* rows, const int* landmarks, const float* dist, float max_distance,
                                           unsigned long long* slots) {
  for (size_t i = 0; i < n; ++i) slots[i] = sba::kAssociateUnclaimed;
  long long accepted = 0;
  for (size_t k = 0; k < count; ++k) {
    if (!sba::associate_within(dist[k], max_distance)) continue;
    ++accepted;
    const unsigned long long key = sba::associate_key(dist[k], static_cast<unsigned int>(rows[k]));
    unsigned long long& slot = slots[static_cast<size_t>(landmarks[k])];
    if (sba::associate_key_before(key, slot)) slot = key;
  }
  return accepted;
}

int landmark_associate_harness_check_options(float ratio, float max_distance) { return sba::associate_check_options(ratio, max_distance) == nullptr ? 1 : 0; }
int landmark_associate_harness_check_rows(int dim, size_t stride) { return sba::descriptor_check_rows(dim, stride) == nullptr ? 1 : 0; }
int landmark_associate_harness_check_sizes(size_t n, size_t m) { return sba::associate_check_sizes(n, m) == nullptr ? 1 : 0; }

}  // extern "C"
