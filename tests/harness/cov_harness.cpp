// TEST HARNESS (tests/ only): exposes the HIP-free part of the joint covariance (csrc/sba_covariance.hpp) -- the host finish
// between the two device passes and the per-match 2x2 block arithmetic the kernels run -- so that it can be driven on the
// CPU with blocks from the dense restatement.
#include "../../spherical_bundle_adjuster_amd/csrc/sba_covariance.hpp"

extern "C" {
// S21: upper triangle of S row by row.  Returns SBA_OK or SBA_ERR_NUMERIC (cov and dim untouched).
int cov_harness_finish(const double* S21, int tran_param, const double* tran, long long n_used, double* cov36, int* dim) {
  return sba::cov_finish(S21, tran_param, tran, n_used, cov36, dim) ? SBA_OK : SBA_ERR_NUMERIC;
}
// Per match i: U[3 i] = (U11, U12, U22), W[12 i] = the two rows of W, s[2 i] the depth scaling; 1 / det formed as
// joint_block() forms it.  out[3 i] = (var d1, var d2, cov) or (inf, inf, 0); S21 (may be null) receives
// -sum W^T U^-1 W over the used matches (upper triangle).  Returns the number of degenerate matches.
long long cov_harness_blocks(long long n, const double* U, const double* W, const double* s, double min_sin2, const double* cov36,
                             double* out, double* S21) {
  long long ndeg = 0;
  if (S21) for (int k = 0; k < 21; ++k) S21[k] = 0.0;
  for (long long i = 0; i < n; ++i) {
    const double U11 = U[3 * i], U12 = U[3 * i + 1], U22 = U[3 * i + 2];
    const double inv_det = 1.0 / (U11 * U22 - U12 * U12);
    const double *w1 = W + 12 * i, *w2 = w1 + 6;
    double z1[6], z2[6], Ui[3];
    if (!sba::cov_block(U11, U12, U22, inv_det, w1, w2, min_sin2, z1, z2, Ui)) {
      ++ndeg;
      if (out) { out[3 * i] = HUGE_VAL; out[3 * i + 1] = HUGE_VAL; out[3 * i + 2] = 0.0; }
      continue;
    }
    if (out) sba::cov_depth_block(s[2 * i], s[2 * i + 1], Ui, z1, z2, cov36, out + 3 * i);
    if (S21) {
      int k = 0;
      for (int a = 0; a < 6; ++a)
        for (int c = a; c < 6; ++c) S21[k++] -= w1[a] * z1[c] + w2[a] * z2[c];
    }
  }
  return ndeg;
}
int cov_harness_layout(int* out7) {
  out7[0] = sba::COV_OUT_S; out7[1] = sba::COV_OUT_COST; out7[2] = sba::COV_OUT_SW; out7[3] = sba::COV_OUT_NUSED;
  out7[4] = sba::COV_OUT_NDEG; out7[5] = sba::COV_OUT_COUNT; out7[6] = sba::COV_ROW;
  return 0;
}
}
