// TEST HARNESS (tests/ only): exposes the HIP-free per-match arithmetic of the triangulated structure
// (csrc/sba_structure.hpp: structure_block, on top of cov_block of csrc/sba_covariance.hpp) so that it can be driven on the CPU
// with blocks from the dense restatement.
#include "../../spherical_bundle_adjuster_amd/csrc/sba_structure.hpp"

extern "C" {
// Per match i: U[3 i] = (U11, U12, U22) and W[12 i] the scaled block and coupling, s[2 i] the depth scaling (as
// cov_harness_blocks takes them), nu[3 i] = -R x1, A[9 i] = d e / d rot (row-major 3 x 3), x2[3 i], d[2 i]; cov36: Sigma_c.
// xyz[3 i], cov[6 i], score[i] out.  Returns the number of degenerate matches.
long long structure_harness_blocks(long long n, const double* U, const double* W, const double* s, const double* nu, const double* A,
                                   const double* x2, const double* d, const double* t, double min_sin2, const double* cov36,
                                   double* xyz, double* cov, double* score) {
  long long ndeg = 0;
  for (long long i = 0; i < n; ++i) {
    const double U11 = U[3 * i], U12 = U[3 * i + 1], U22 = U[3 * i + 2];
    const double inv_det = 1.0 / (U11 * U22 - U12 * U12);
    const double *w1 = W + 12 * i, *w2 = w1 + 6;
    double z1[6], z2[6], Ui[3], Am[3][3];
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) Am[r][c] = A[9 * i + 3 * r + c];
    const bool ok = sba::cov_block(U11, U12, U22, inv_det, w1, w2, min_sin2, z1, z2, Ui);
    if (!ok) ++ndeg;
    sba::structure_block(ok, true, nu + 3 * i, Am, s[2 * i], s[2 * i + 1], z1, z2, Ui, cov36, x2[3 * i], x2[3 * i + 1], x2[3 * i + 2],
                         d[2 * i], d[2 * i + 1], t, xyz + 3 * i, cov + 6 * i, score + i);
  }
  return ndeg;
}
// want_cov = false: X alone, nothing else is written.
void structure_harness_xyz(long long n, const double* nu, const double* x2, const double* d, const double* t, double* xyz) {
  const double A[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
  for (long long i = 0; i < n; ++i)
    sba::structure_block(false, false, nu + 3 * i, A, 1.0, 1.0, nullptr, nullptr, nullptr, nullptr, x2[3 * i], x2[3 * i + 1],
                         x2[3 * i + 2], d[2 * i], d[2 * i + 1], t, xyz + 3 * i, nullptr, nullptr);
}
}
