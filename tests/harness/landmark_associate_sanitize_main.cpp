// TEST PROGRAM (tests/ only; built with g++ -fsanitize=address,undefined and run as a child process by
// tests/test_landmark_associate_cpu.py): the host and device share of the landmark map's association
// (csrc/sba_landmarks_associate.hpp) with exact-sized heap buffers -- the key's halves and its order at the ends of the float
// range, a claim whose winner does not depend on the order of arrival, the inclusive distance cut, and the checks at their limits.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../spherical_bundle_adjuster_amd/csrc/sba_landmarks_associate.hpp"

namespace {

int failures = 0;
void expect(bool ok, const char* what) {
  if (!ok) { std::printf("FAILED: %s\n", what); ++failures; }
}

struct Row { int row, landmark; float dist; };

std::vector<unsigned long long> claim(size_t n, const std::vector<Row>& rows, float max_distance, long long* accepted) {
  std::vector<unsigned long long> slots(n, sba::kAssociateUnclaimed);
  *accepted = 0;
  for (const Row& r : rows) {
    if (!sba::associate_within(r.dist, max_distance)) continue;
    ++*accepted;
    const unsigned long long key = sba::associate_key(r.dist, static_cast<unsigned int>(r.row));
    if (sba::associate_key_before(key, slots[static_cast<size_t>(r.landmark)])) slots[static_cast<size_t>(r.landmark)] = key;
  }
  return slots;
}

}  // namespace

int main() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const float fmax = std::numeric_limits<float>::max(), tiny = std::numeric_limits<float>::denorm_min();
  // the halves come back, and the bit order is the value order for d0 >= 0
  const std::vector<float> ds = {0.0f, tiny, 1.0f, std::nextafter(1.0f, 2.0f), std::sqrt(2.0f), 1000.0f, fmax, inf};
  const unsigned int top_row = (1u << 31) - 1u;
  for (size_t a = 0; a < ds.size(); ++a) {
    const unsigned long long k0 = sba::associate_key(ds[a], 0u), k1 = sba::associate_key(ds[a], top_row);
    expect(sba::associate_key_row(k0) == 0u && sba::associate_key_row(k1) == top_row, "the row half");
    expect(sba::associate_key_distance(k0) == ds[a] && sba::associate_key_distance(k1) == ds[a], "the distance half");
    expect(sba::associate_key_before(k0, k1) && !sba::associate_key_before(k1, k0) && !sba::associate_key_before(k0, k0), "equal distances: the lower row");
    expect(k1 != sba::kAssociateUnclaimed && sba::associate_key_before(k1, sba::kAssociateUnclaimed), "every key beats an unclaimed slot");
    for (size_t b = a + 1; b < ds.size(); ++b)
      expect(sba::associate_key_before(k1, sba::associate_key(ds[b], 0u)), "a smaller distance wins whatever the rows");
  }
  // the cut is inclusive; a NaN distance is never within it
  expect(sba::associate_within(1.0f, 1.0f) && !sba::associate_within(std::nextafter(1.0f, 2.0f), 1.0f) && sba::associate_within(fmax, inf) &&
             sba::associate_within(inf, inf) && !sba::associate_within(nan, inf) && !sba::associate_within(1.0f, nan), "the distance cut");
  // a claim: the same slots in every order of arrival
  {
    std::vector<Row> rows = {{7, 2, 1.0f}, {3, 2, 1.0f}, {9, 2, std::sqrt(2.0f)}, {1, 0, std::sqrt(2.0f)}, {4, 3, 1.0f}, {5, 3, 0.0f}, {6, 1, 3.0f}};
    long long acc = 0;
    const std::vector<unsigned long long> want = claim(5, rows, inf, &acc);
    expect(acc == 7 && sba::associate_key_row(want[2]) == 3u && sba::associate_key_distance(want[2]) == 1.0f, "equal distances: row 3 before row 7");
    expect(sba::associate_key_row(want[3]) == 5u && sba::associate_key_row(want[0]) == 1u && sba::associate_key_row(want[1]) == 6u, "the other winners");
    expect(want[4] == sba::kAssociateUnclaimed, "nobody claims landmark 4");
    std::sort(rows.begin(), rows.end(), [](const Row& a, const Row& b) { return a.row > b.row; });
    do {
      expect(claim(5, rows, inf, &acc) == want, "the order of arrival does not matter");
    } while (std::next_permutation(rows.begin(), rows.end(), [](const Row& a, const Row& b) { return a.row > b.row; }));
    const std::vector<unsigned long long> cut = claim(5, rows, 1.0f, &acc);
    expect(acc == 4 && cut[0] == sba::kAssociateUnclaimed && cut[1] == sba::kAssociateUnclaimed && cut[2] == want[2] && cut[3] == want[3], "max_distance = 1");
  }
  // the checks
  expect(sba::associate_check_options(0.3f, inf) == nullptr && sba::associate_check_options(tiny, tiny) == nullptr &&
             sba::associate_check_options(1.5f, 1.0f) == nullptr, "options: fine");
  expect(sba::associate_check_options(0.0f, inf) && sba::associate_check_options(-0.3f, inf) && sba::associate_check_options(inf, inf) &&
             sba::associate_check_options(nan, inf), "options: ratio");
  expect(sba::associate_check_options(0.3f, 0.0f) && sba::associate_check_options(0.3f, -1.0f) && sba::associate_check_options(0.3f, -inf) &&
             sba::associate_check_options(0.3f, nan), "options: max_distance");
  expect(sba::descriptor_check_rows(1, 4) == nullptr && sba::descriptor_check_rows(256, 1024) == nullptr && sba::descriptor_check_rows(36, 148) == nullptr,
         "rows: fine");
  expect(sba::descriptor_check_rows(0, 4) && sba::descriptor_check_rows(-1, 4) && sba::descriptor_check_rows(257, 2048) && sba::descriptor_check_rows(36, 140) &&
             sba::descriptor_check_rows(36, 146) && sba::descriptor_check_rows(1, 0), "rows: refused");
  {
    const size_t lim = static_cast<size_t>(1) << 31, top = static_cast<size_t>(-1);
    expect(sba::associate_check_sizes(0, 0) == nullptr && sba::associate_check_sizes(lim - 1, lim - 1) == nullptr, "sizes: fine");
    expect(sba::associate_check_sizes(lim, 1) && sba::associate_check_sizes(1, lim) && sba::associate_check_sizes(top, top), "sizes: refused");
  }
  if (failures) return 1;
  std::printf("landmark associate host checks passed\n");
  return 0;
}
