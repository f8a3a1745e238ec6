// TEST PROGRAM (tests/ only; built with g++ -fsanitize=address,undefined and run as a child process by
// tests/test_resection_consensus_host_cpu.py): the host side of the robust resection guess at its edge sizes -- the sampler
// when a trial must draw every match (n = 6 with 6, n = 64 with 64) and from a large handle, the row moments, the DLT finish
// on general and on planar rows, and the pick -- with exact-sized heap buffers, so an index one past an end is caught.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../spherical_bundle_adjuster_amd/csrc/sba_resection_consensus.hpp"

namespace {

int failures = 0;
void expect(bool ok, const char* what) {
  if (!ok) { std::printf("FAILED: %s\n", what); ++failures; }
}

// a seeded scene: landmarks at distance 2 .. 10, exact bearings of the pose (rot about z by 0.3, tran (0.1, -0.2, 0.4))
void make_rows(int m, bool planar, std::vector<double>* rows) {
  uint64_t s = 12345;
  rows->assign(static_cast<size_t>(m) * SBA_RESECT_ROW, 0.0);
  const double c = std::cos(0.3), sn = std::sin(0.3), t[3] = {0.1, -0.2, 0.4};
  for (int i = 0; i < m; ++i) {
    double X[3];
    for (int k = 0; k < 3; ++k) X[k] = -6.0 + 12.0 * static_cast<double>(sba::epi::splitmix64(s) >> 11) / 9007199254740992.0;
    if (planar) X[2] = 3.0;
    const double Y[3] = {c * X[0] - sn * X[1] - t[0], sn * X[0] + c * X[1] - t[1], X[2] - t[2]};
    const double len = std::sqrt(Y[0] * Y[0] + Y[1] * Y[1] + Y[2] * Y[2]);
    for (int k = 0; k < 3; ++k) { (*rows)[SBA_RESECT_ROW * i + k] = X[k]; (*rows)[SBA_RESECT_ROW * i + 3 + k] = Y[k] / len; }
  }
}

void check_sample(uint64_t seed, uint64_t n, int m, int trials) {
  for (int t = 0; t < trials; ++t) {
    std::vector<long long> idx(m, -1);
    sba::resect_sample_trial(seed, t, n, m, idx.data());
    for (int i = 0; i < m; ++i) {
      expect(idx[i] >= 0 && static_cast<uint64_t>(idx[i]) < n, "sampled index in range");
      for (int j = 0; j < i; ++j) expect(idx[i] != idx[j], "sampled indices distinct");
    }
  }
}

}  // namespace

int main() {
  check_sample(7, 6, 6, 128);
  check_sample(7, 64, 64, 128);
  check_sample(0, 7, 6, 128);
  check_sample(~0ull, 10000000ull, 64, 1024);

  for (int m : {6, 7, 64}) {
    std::vector<double> rows;
    make_rows(m, false, &rows);
    std::vector<double> mom(SBA_RESECT_MOM_COUNT, -1.0);
    sba::resect_row_moments(rows.data(), m, mom.data());
    expect(mom[SBA_RESECT_MOM_N] == m, "row count");
    double rot[3], tran[3];
    sba_resection_guess_info info;
    const int rc = sba::resect_trial_pose(rows.data(), m, rot, tran, &info);
    expect(rc == SBA_OK, "a general sample finishes");
    expect(std::fabs(rot[2] - 0.3) < 1e-9 && std::fabs(rot[0]) < 1e-9 && std::fabs(tran[2] - 0.4) < 1e-9, "exact rows give the pose");
    make_rows(m, true, &rows);
    expect(sba::resect_trial_pose(rows.data(), m, rot, tran, &info) == SBA_ERR_NUMERIC, "a planar sample is refused");
  }
  {
    std::vector<double> rows;
    make_rows(5, false, &rows);
    double rot[3], tran[3];
    sba_resection_guess_info info;
    expect(sba::resect_trial_pose(rows.data(), 5, rot, tran, &info) == SBA_ERR_NUMERIC, "five rows are refused");
    expect(sba::resect_trial_pose(rows.data(), 0, rot, tran, &info) == SBA_ERR_NUMERIC, "no rows are refused");
  }
  {
    std::vector<long long> c = {3, 9, -1, 9, 2};
    expect(sba::resect_pick(c.data(), 5) == 1, "first maximum");
    std::vector<long long> none(1024, -1);
    expect(sba::resect_pick(none.data(), 1024) == -1, "no count");
    none[1023] = 0;
    expect(sba::resect_pick(none.data(), 1024) == 1023, "a zero count beats a refusal");
    expect(sba::resect_pick(none.data(), 0) == -1, "no trials");
  }
  if (failures) return 1;
  std::printf("resection consensus host checks passed\n");
  return 0;
}
