// Entry points of the batched triangulated structure (include/sba_hip.h): for every pair of a batch one 3-D point per match with
// its 3 x 3 covariance and the score trace / X.X at (rot[g], tran[g]) and the batch's resident depths, and the cut driven by
// that score -- what sba_structure.cpp does for one problem.  Every call makes two launches on the batch's stream with no host
// wait between them: the batched covariance's reduce + finish (sba_batch_covariance.cpp: cov_enqueue; batch_cov_kernel,
// unchanged), then batch_structure_kernel (sba_batch_structure.hip), which reads every pair's Sigma_c from the pair's record.
// The cut hands the score plane to the batch's selection and compaction (sba_quantile.cpp), unchanged.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <limits>
#include <vector>

#include "sba_batch.hpp"

namespace {

using sba::batch::CovPass;

size_t up256(size_t v) { return (v + 255) & ~size_t(255); }
bool aligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15u) == 0; }

// The whole-call refusals every entry point here shares: those of sba_batch_covariance_joint but the NULL out.
int check_call(sba_batch* b, const double* rot, const double* tran, double min_sin2_parallax) {
  if (!b) return sba::set_error(SBA_ERR_INVALID_ARG, "null batch handle");
  if (!(min_sin2_parallax >= 0.0)) return sba::set_error(SBA_ERR_INVALID_ARG, "min_sin2_parallax must be >= 0");
  return sba::batch::joint_check(b, rot, tran);            // the refusals of sba_batch_solve_joint
}

int check_ranks(const sba_batch* b, const size_t* ranks, int num_ranks) {
  for (int g = 0; g < b->num_pairs; ++g)
    for (int j = 0; j < num_ranks && b->n[g] > 0; ++j)     // an empty pair takes no part: its ranks are not looked at
      if (ranks[static_cast<size_t>(g) * num_ranks + j] >= b->n[g])
        return sba::set_error(SBA_ERR_INVALID_ARG, "pair %d: rank %zu is not below its %zu matches", g,
                              ranks[static_cast<size_t>(g) * num_ranks + j], b->n[g]);
  return SBA_OK;
}

// Blocks per pair of the structure pass.  There is no reduction, so a pair's rows may be split over several blocks without
// changing a bit: as many as the CUs allow per pair, never more than the largest pair has 256-vector tiles.
// SBA_BATCH_STRUCTURE_BPP (tests) overrides it.
int blocks_per_pair(const sba_batch* b) {
  size_t max_vecs = 0;
  for (size_t m : b->n) max_vecs = std::max(max_vecs, (m + 1) / 2);
  const long long tiles = static_cast<long long>(std::max<size_t>(1, (max_vecs + 255) / 256));
  long long bpp = std::min<long long>(std::max<long long>(b->num_cus / std::max(1, b->num_pairs), 1), tiles);
  if (const char* env = std::getenv("SBA_BATCH_STRUCTURE_BPP")) { const long long v = std::atoll(env); if (v >= 1) bpp = v; }
  return static_cast<int>(std::min<long long>(bpp, 65535));
}

// The two launches: reduce + finish, then the structure pass into the device destinations (caller row order, any of them null).
// fill: what a pair without a covariance gets in every row.  *cp: what cov_wait still has to wait for.
int enqueue_pass(sba_batch* b, const double* rot, const double* tran, const sba_lm_options* opt, double min_sin2_parallax,
                 double fill, double* xyz, double* cov, double* score, CovPass* cp) {
  const int rc = sba::batch::cov_enqueue(b, rot, tran, opt, min_sin2_parallax, nullptr, cp);
  if (rc) return rc;
  if (sba::batch::batch_rows(b) == 0) return SBA_OK;
  SBA_TRY_HIP(sba::launch_batch_structure(b->store, cp->pl, b->desc_dev, b->num_pairs, blocks_per_pair(b), cp->o, min_sin2_parallax,
                                          fill, b->offsets_dev, b->cov_rec_host_dev, xyz, cov, score, b->stream));
  return SBA_OK;
}

// The records and the stream, then out / status; *failures: pairs without a covariance.
int finish_pass(sba_batch* b, CovPass* cp, sba_joint_cov* out, int* status, int* failures) {
  int rc = sba::batch::cov_wait(b, cp, "batched structure: reduce pass and finish");
  if (rc) return rc;
  rc = sba::stream_wait(b->stream, "batched structure pass", &b->poisoned);
  if (rc) return rc;
  *failures = sba::batch::cov_read(b, out, status);
  return SBA_OK;
}

}  // namespace

extern "C" {

int sba_batch_structure_joint(sba_batch* b, const double* rot, const double* tran, const sba_lm_options* opt,
                              double min_sin2_parallax, sba_joint_cov* out, double* xyz, double* xyz_cov, double* score,
                              int* status) {
  int rc = check_call(b, rot, tran, min_sin2_parallax);
  if (rc) return rc;
  const int B = b->num_pairs;
  if (B == 0) return SBA_OK;
  if (!out) return sba::set_error(SBA_ERR_INVALID_ARG, "out is null");

  SBA_TRY_HIP(hipSetDevice(b->device));
  const size_t base = b->offsets.front(), total = b->offsets.back() - base;
  // The outputs asked for pass through a scratch of their own (xyz | cov | score, 3 + 6 + 1 doubles per row at the most):
  // nothing of the batch's work planes is borrowed, so nothing needs re-zeroing.
  const size_t off_cov = xyz ? up256(3 * total * sizeof(double)) : 0;
  const size_t off_score = off_cov + (xyz_cov ? up256(6 * total * sizeof(double)) : 0);
  const size_t need = off_score + (score ? up256(total * sizeof(double)) : 0);
  double *xyz_dev = nullptr, *cov_dev = nullptr, *score_dev = nullptr;
  if (total > 0 && need > 0) {
    rc = sba::batch::grow_scratch(&b->structure_scratch, &b->structure_scratch_bytes, need, b->stream, &b->poisoned);
    if (rc) return rc;
    char* s = static_cast<char*>(b->structure_scratch);
    if (xyz) xyz_dev = reinterpret_cast<double*>(s);
    if (xyz_cov) cov_dev = reinterpret_cast<double*>(s + off_cov);
    if (score) score_dev = reinterpret_cast<double*>(s + off_score);
  }
  CovPass cp;
  rc = enqueue_pass(b, rot, tran, opt, min_sin2_parallax, std::numeric_limits<double>::quiet_NaN(), xyz_dev, cov_dev, score_dev, &cp);
  if (rc) return rc;
  if (xyz_dev) SBA_TRY_HIP(hipMemcpyAsync(xyz + 3 * base, xyz_dev, 3 * total * sizeof(double), hipMemcpyDeviceToHost, b->stream));
  if (cov_dev) SBA_TRY_HIP(hipMemcpyAsync(xyz_cov + 6 * base, cov_dev, 6 * total * sizeof(double), hipMemcpyDeviceToHost, b->stream));
  if (score_dev) SBA_TRY_HIP(hipMemcpyAsync(score + base, score_dev, total * sizeof(double), hipMemcpyDeviceToHost, b->stream));
  int failures = 0;
  rc = finish_pass(b, &cp, out, status, &failures);
  if (rc) return rc;
  return sba::batch::cov_failed(failures, B);
}

int sba_batch_structure_joint_device(sba_batch* b, const double* rot, const double* tran, const sba_lm_options* opt,
                                     double min_sin2_parallax, sba_joint_cov* out, double* xyz, double* xyz_cov, double* score,
                                     int* status) {
  int rc = check_call(b, rot, tran, min_sin2_parallax);
  if (rc) return rc;
  if (!aligned16(xyz) || !aligned16(xyz_cov) || !aligned16(score))
    return sba::set_error(SBA_ERR_INVALID_ARG, "the device destinations must be 16-byte aligned");
  const int B = b->num_pairs;
  if (B == 0) return SBA_OK;
  if (!out) return sba::set_error(SBA_ERR_INVALID_ARG, "out is null");

  SBA_TRY_HIP(hipSetDevice(b->device));
  CovPass cp;
  rc = enqueue_pass(b, rot, tran, opt, min_sin2_parallax, std::numeric_limits<double>::quiet_NaN(), xyz, xyz_cov, score, &cp);
  if (rc) return rc;
  int failures = 0;
  rc = finish_pass(b, &cp, out, status, &failures);
  if (rc) return rc;
  return sba::batch::cov_failed(failures, B);
}

int sba_batch_structure_order_stats(sba_batch* b, const double* rot, const double* tran, const sba_lm_options* opt,
                                    double min_sin2_parallax, const size_t* ranks, int num_ranks, double* values, int* status) {
  if (!ranks || !values) return sba::set_error(SBA_ERR_INVALID_ARG, "ranks/values must not be null");
  if (num_ranks < 1 || num_ranks > sba::kSelectMaxRanks)
    return sba::set_error(SBA_ERR_INVALID_ARG, "num_ranks %d outside 1...%d", num_ranks, sba::kSelectMaxRanks);
  int rc = check_call(b, rot, tran, min_sin2_parallax);
  if (rc) return rc;
  rc = check_ranks(b, ranks, num_ranks);
  if (rc) return rc;
  const int B = b->num_pairs;
  if (B == 0) return SBA_OK;

  SBA_TRY_HIP(hipSetDevice(b->device));
  const size_t rows = sba::batch::batch_rows(b), nvals = static_cast<size_t>(B) * num_ranks;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  CovPass cp;
  if (rows == 0) {
    std::fill(values, values + nvals, nan);
    rc = enqueue_pass(b, rot, tran, opt, min_sin2_parallax, 0.0, nullptr, nullptr, nullptr, &cp);
    if (rc) return rc;
  } else {
    // In the scratch plane a pair without a covariance has +0.0 in every row: the selection runs on it like on any pair, and
    // its values are replaced below.
    sba::SelectScratch s;
    double* plane = nullptr;
    rc = sba::batch::select_plane(b, num_ranks, &s, &plane);
    if (rc) return rc;
    rc = enqueue_pass(b, rot, tran, opt, min_sin2_parallax, 0.0, nullptr, nullptr, plane, &cp);
    if (rc) return rc;
    rc = sba::batch::select_enqueue(b, s, ranks, num_ranks, nullptr);
    if (rc) return rc;
    SBA_TRY_HIP(hipMemcpyAsync(values, s.values, nvals * sizeof(double), hipMemcpyDeviceToHost, b->stream));
  }
  std::vector<int> st(B);
  int failures = 0;
  rc = finish_pass(b, &cp, nullptr, st.data(), &failures);
  if (rc) return rc;
  for (int g = 0; g < B; ++g) {
    if (status) status[g] = st[g];
    if (st[g] != SBA_OK) std::fill(values + static_cast<size_t>(g) * num_ranks, values + static_cast<size_t>(g + 1) * num_ranks, nan);
  }
  return sba::batch::cov_failed(failures, B);
}

int sba_batch_structure_keep_below(sba_batch* b, const double* rot, const double* tran, const sba_lm_options* opt,
                                   double min_sin2_parallax, const size_t* rank, const double* scale, double* threshold,
                                   size_t* n_kept, long long* kept_index, int* status) {
  if (!rank || !scale || !threshold || !n_kept)
    return sba::set_error(SBA_ERR_INVALID_ARG, "rank/scale/threshold/n_kept must not be null");
  int rc = check_call(b, rot, tran, min_sin2_parallax);
  if (rc) return rc;
  rc = check_ranks(b, rank, 1);
  if (rc) return rc;
  const int B = b->num_pairs;
  for (int g = 0; g < B; ++g)
    if (!std::isfinite(scale[g]) || scale[g] < 0.0) return sba::set_error(SBA_ERR_INVALID_ARG, "scale must be finite and >= 0");
  if (B == 0) return SBA_OK;

  SBA_TRY_HIP(hipSetDevice(b->device));
  const size_t rows = sba::batch::batch_rows(b);
  const double nan = std::numeric_limits<double>::quiet_NaN();
  CovPass cp;
  std::vector<int> st(B);
  int failures = 0;
  if (rows == 0) {
    rc = enqueue_pass(b, rot, tran, opt, min_sin2_parallax, 0.0, nullptr, nullptr, nullptr, &cp);
    if (rc) return rc;
    rc = finish_pass(b, &cp, nullptr, st.data(), &failures);
    if (rc) return rc;
    sba::batch::compact_nothing(b, n_kept);
  } else {
    // A pair without a covariance is not cut: its rows of the scratch plane are +0.0, so the selection picks 0, the threshold
    // is scale * 0 = 0 and the keep-rule 0 <= 0 keeps every row; the threshold it reports is replaced below.
    sba::SelectScratch s;
    double* plane = nullptr;
    rc = sba::batch::select_plane(b, 1, &s, &plane);
    if (rc) return rc;
    rc = enqueue_pass(b, rot, tran, opt, min_sin2_parallax, 0.0, nullptr, nullptr, plane, &cp);
    if (rc) return rc;
    rc = sba::batch::select_enqueue(b, s, rank, 1, scale);
    if (rc) return rc;
    // the records leave the handle with the old layout: read them before the compaction
    rc = sba::batch::cov_wait(b, &cp, "batched structure: reduce pass and finish");
    if (rc) return rc;
    failures = sba::batch::cov_read(b, nullptr, st.data());
    rc = sba::batch::select_keep(b, s, threshold, n_kept, kept_index);
    if (rc) return rc;
  }
  for (int g = 0; g < B; ++g) {
    if (status) status[g] = st[g];
    if (st[g] != SBA_OK || rows == 0) threshold[g] = nan;
  }
  return sba::batch::cov_failed(failures, B);
}

}  // extern "C"
