// Entry point of the batched joint covariance (include/sba_hip.h): every pair's 6 x 6 pose block and per-match depth blocks at
// (rot[g], tran[g]) and the batch's resident depths -- what sba_problem_covariance_joint does for one problem, per pair of a
// batch.  Kernel: sba_batch_covariance.hip; algebra and finish: sba_covariance.hpp.  The record setup, the launches and the
// read-out are written once (sba::batch::cov_enqueue / cov_wait / cov_read): the batched structure (sba_batch_structure.cpp)
// runs its reduce pass and finish through them.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "sba_batch.hpp"
#include "sba_covariance.hpp"
#include "sba_lm.hpp"

namespace sba {
namespace batch {

int cov_enqueue(sba_batch* b, const double* rot, const double* tran, const sba_lm_options* opt, double min_sin2_parallax,
                double* depth_dev, CovPass* cp) {
  const int B = b->num_pairs;
  joint_options(opt, &cp->o);
  const sba_lm_options& o = cp->o;
  cp->seq = 0;
  if (!b->cov_rec_host) {
    const size_t bytes = sizeof(sba::BatchCovRec) * static_cast<size_t>(B) + 64;
    SBA_TRY_HIP(hipHostMalloc(reinterpret_cast<void**>(&b->cov_rec_host), bytes, hipHostMallocMapped | hipHostMallocCoherent));
    std::memset(b->cov_rec_host, 0, bytes);
    SBA_TRY_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&b->cov_rec_host_dev), b->cov_rec_host, 0));
    b->cov_seq = 0;
  }
  sba::BatchCovRec* rec = b->cov_rec_host;
  volatile unsigned long long* flag = reinterpret_cast<volatile unsigned long long*>(rec + B);
  unsigned long long* flag_dev = reinterpret_cast<unsigned long long*>(b->cov_rec_host_dev + B);
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (int g = 0; g < B; ++g) {
    sba::BatchCovRec& r = rec[g];
    bool finite = true;
    for (int a = 0; a < 3; ++a) {
      r.rot[a] = rot[3 * g + a]; r.tran[a] = tran[3 * g + a];
      finite = finite && std::isfinite(r.rot[a]) && std::isfinite(r.tran[a]);
    }
    r.refused = finite ? 0 : 1;
    r.dim_status = 0;
  }
  sba::Planes& pl = cp->pl;
  for (int k = 0; k < 3; ++k) { pl.x1[k] = b->coord[k]; pl.x2[k] = b->coord[3 + k]; }
  pl.d1 = b->dplane[0]; pl.d2 = b->dplane[1];

  bool device_finish = true;     // SBA_BATCH_DEVICE_COV=0: reduce launch, the host's cov_finish per pair, depth launch (the second oracle)
  if (const char* env = std::getenv("SBA_BATCH_DEVICE_COV")) device_finish = std::strcmp(env, "0") != 0;
  const int gauge_dim = o.tran_param == SBA_TRAN_SPHERE ? 5 : 6;
  if (device_finish) {
    const unsigned long long seq = ++b->cov_seq;
    SBA_TRY_HIP(sba::launch_batch_cov(b->store, pl, b->desc_dev, B, o, min_sin2_parallax,
                                      sba::kCovReduce | sba::kCovFinish | (depth_dev ? sba::kCovDepth : 0), b->offsets_dev, depth_dev,
                                      b->cov_rec_host_dev, b->lm_ticket, flag_dev, seq, b->stream));
    cp->seq = seq;
  } else {
    unsigned long long seq = ++b->cov_seq;
    SBA_TRY_HIP(sba::launch_batch_cov(b->store, pl, b->desc_dev, B, o, min_sin2_parallax, sba::kCovReduce, b->offsets_dev, nullptr,
                                      b->cov_rec_host_dev, b->lm_ticket, flag_dev, seq, b->stream));
    const int rc = sba::wait_for_sequence(flag, seq, b->stream, "batched joint covariance reduce pass", &b->poisoned);
    if (rc) return rc;
    for (int g = 0; g < B; ++g) {
      sba::BatchCovRec& r = rec[g];
      int dim = gauge_dim;
      const bool ok = !r.refused && sba::cov_finish(r.row + sba::COV_OUT_S, o.tran_param, r.tran,
                                                    static_cast<long long>(r.row[sba::COV_OUT_NUSED]), r.sigma, &dim);
      if (!ok) for (int k = 0; k < 36; ++k) r.sigma[k] = nan;
      r.dim_status = static_cast<unsigned long long>(static_cast<unsigned>(ok ? dim : gauge_dim)) | (ok ? 0ull : 1ull << 32);
    }
    if (depth_dev) {
      seq = ++b->cov_seq;
      SBA_TRY_HIP(sba::launch_batch_cov(b->store, pl, b->desc_dev, B, o, min_sin2_parallax, sba::kCovDepth, b->offsets_dev, depth_dev,
                                        b->cov_rec_host_dev, b->lm_ticket, flag_dev, seq, b->stream));
    }
  }
  return SBA_OK;
}

int cov_wait(sba_batch* b, CovPass* cp, const char* what) {
  if (cp->seq == 0) return SBA_OK;
  const volatile unsigned long long* flag = reinterpret_cast<const volatile unsigned long long*>(b->cov_rec_host + b->num_pairs);
  const unsigned long long seq = cp->seq;
  cp->seq = 0;
  return sba::wait_for_sequence(flag, seq, b->stream, what, &b->poisoned);
}

int cov_read(const sba_batch* b, sba_joint_cov* out, int* status) {
  int failures = 0;
  for (int g = 0; g < b->num_pairs; ++g) {
    const sba::BatchCovRec& r = b->cov_rec_host[g];
    const bool failed = (r.dim_status >> 32) != 0;
    if (out) {
      sba_joint_cov& e = out[g];
      std::memcpy(e.cov, r.sigma, sizeof(e.cov));
      e.cost = r.row[sba::COV_OUT_COST]; e.sum_w = r.row[sba::COV_OUT_SW];
      e.n_used = static_cast<long long>(r.row[sba::COV_OUT_NUSED]);
      e.n_degenerate = static_cast<long long>(r.row[sba::COV_OUT_NDEG]);
      e.dim = static_cast<int>(r.dim_status & 0xffffffffull);
      e.dof = static_cast<int>(e.n_used - e.dim);
    }
    if (status) status[g] = failed ? SBA_ERR_NUMERIC : SBA_OK;
    if (failed) ++failures;
  }
  return failures;
}

int cov_failed(int failures, int num_pairs) {
  if (failures)
    return sba::set_error(SBA_ERR_NUMERIC, "%d of %d pairs have no joint covariance: a non-finite point, fewer used matches than the "
                                           "gauge's dimension, or a reduced camera system that is not finite or rank-deficient (see "
                                           "per-pair status)", failures, num_pairs);
  return SBA_OK;
}

}  // namespace batch
}  // namespace sba

extern "C" {

int sba_batch_covariance_joint(sba_batch* b, const double* rot, const double* tran, const sba_lm_options* opt,
                               double min_sin2_parallax, sba_joint_cov* out, double* depth_cov, int* status) {
  if (!b) return sba::set_error(SBA_ERR_INVALID_ARG, "null batch handle");
  if (!(min_sin2_parallax >= 0.0)) return sba::set_error(SBA_ERR_INVALID_ARG, "min_sin2_parallax must be >= 0");
  int rc = sba::batch::joint_check(b, rot, tran);          // the refusals of sba_batch_solve_joint
  if (rc) return rc;
  const int B = b->num_pairs;
  if (B == 0) return SBA_OK;
  if (!out) return sba::set_error(SBA_ERR_INVALID_ARG, "out is null");

  SBA_TRY_HIP(hipSetDevice(b->device));
  const size_t base = b->offsets.front(), total = b->offsets.back() - base;
  const bool want_depths = depth_cov && total > 0;
  // The per-match output passes through the d-only stage's work planes (4 planes >= 3 * total doubles; no stage overlaps
  // another) and they are handed back zeroed, the state ensure_depth_work leaves them in.
  double* dd_dev = nullptr;
  if (want_depths) {
    rc = sba::batch::ensure_depth_work(b);
    if (rc) return rc;
    dd_dev = b->depth_work;
  }
  sba::batch::CovPass cp;
  rc = sba::batch::cov_enqueue(b, rot, tran, opt, min_sin2_parallax, dd_dev, &cp);
  if (rc) return rc;
  rc = sba::batch::cov_wait(b, &cp, "batched joint covariance");
  if (rc) return rc;
  if (want_depths) {
    SBA_TRY_HIP(hipMemcpyAsync(depth_cov + 3 * base, dd_dev, 3 * total * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    SBA_TRY_HIP(hipMemsetAsync(dd_dev, 0, 3 * total * sizeof(double), b->stream));
    rc = sba::stream_wait(b->stream, "batched joint covariance depth rows", &b->poisoned);
    if (rc) return rc;
  }
  return sba::batch::cov_failed(sba::batch::cov_read(b, out, status), B);
}

}  // extern "C"
