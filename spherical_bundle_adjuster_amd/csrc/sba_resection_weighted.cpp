// Entry points of the covariance-weighted resection (include/sba_hip.h): the handle's copy of the landmark covariances, the
// freeze of the factored weights at a reference pose, the weighted evaluation and solve, and the covariance of the resected
// pose.  Kernels: sba_resection_weighted.hip; algebra, option checks and the host finish: sba_resection_weighted.hpp; handle
// refusals, work memory, the published row: sba_resection_entry.hpp; the LM schedule is sba_lm.hpp's.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sba_lm.hpp"
#include "sba_problem.hpp"
#include "sba_resection_entry.hpp"
#include "sba_resection_weighted.hpp"

namespace {

// sba_resection_entry.hpp's unweighted pass is not called from this file.
[[maybe_unused]] const auto unweighted_pass_unused = &resect_reduce_pass;

bool finite3(const double* a, const double* b) {
  for (int i = 0; i < 3; ++i)
    if (!std::isfinite(a[i]) || !std::isfinite(b[i])) return false;
  return true;
}

// The refusals that need no device: the handle's, then the state of the weighted resection.
int wres_check(sba_problem* p, bool need_frozen) {
  const int rc = resect_check_handle(p);
  if (rc) return rc;
  if (!p->wres_have_cov)
    return sba::set_error(SBA_ERR_UNSUPPORTED, "no landmark covariances on the handle (every upload and compaction drops them): call "
                                               "sba_problem_resection_set_landmark_cov");
  if (need_frozen && !p->wres_frozen)
    return sba::set_error(SBA_ERR_UNSUPPORTED, "the resection weights are not frozen: call sba_problem_resection_freeze_weights");
  return SBA_OK;
}

sba::ResectWeightPlanes wres_planes(const sba_problem* p) {
  sba::ResectWeightPlanes wp;
  for (int k = 0; k < 3; ++k) wp.q[k] = p->wres_planes + static_cast<size_t>(k) * p->wres_plane_elems;
  return wp;
}

// resect_prepare, with the grid of the weighted reduce pass (its own occupancy, the same caps).
int wres_prepare(sba_problem* p, bool loss, ResectWork* w) {
  const int rc = resect_prepare(p, loss, w);
  if (rc) return rc;
  int& occ = p->wres_occ[p->store][loss ? 1 : 0];
  if (occ == 0) {
    SBA_TRY_HIP(sba::resect_wreduce_blocks_per_cu(p->store, loss, &occ));
    occ = std::max(1, occ);
  }
  const size_t ppt = static_cast<size_t>(sba::points_per_lane(p->store));
  const size_t blocks = ((p->n + ppt - 1) / ppt + 255) / 256;
  int cap = 1 << 30;
  if (const char* env = std::getenv("SBA_RESECT_GRID")) { const int v = std::atoi(env); if (v >= 1) cap = v; }
  w->grid = static_cast<int>(std::min<size_t>({blocks, static_cast<size_t>(p->num_cus) * std::min(occ, 2), static_cast<size_t>(cap)}));
  return SBA_OK;
}

int wres_reduce_pass(sba_problem* p, const ResectWork& w, const double rot[3], const double tran[3], double huber_delta, double* row) {
  sba::ResectParams prm;
  sba::fill_resect_params(p->n, rot, tran, huber_delta, &prm);
  const unsigned long long seq = ++p->joint_seq;
  SBA_TRY_HIP(sba::launch_resect_wreduce(p->store, w.pl, wres_planes(p), prm, w.partials, w.grid, w.out_dev,
                                         p->publish ? p->joint_host_dev : nullptr, seq, p->stream));
  return resect_fetch(p, w, seq, SBA_RESECT_COUNT, "weighted resection reduce pass", row);
}

// The freeze: the planes allocated (and zeroed) when the handle's plane size changed, one pass, the count fetched.
int wres_freeze(sba_problem* p, const ResectWork& w, const double rot[3], const double tran[3], double bearing_sigma) {
  if (!p->wres_planes || p->wres_plane_elems != p->plane_elems) {
    if (p->wres_planes) SBA_TRY_HIP(hipFree(p->wres_planes));
    p->wres_planes = nullptr; p->wres_plane_elems = 0;
    const size_t bytes = (3 * p->plane_elems + 2) * sizeof(double);
    SBA_TRY_HIP(hipMalloc(reinterpret_cast<void**>(&p->wres_planes), bytes));
    p->wres_plane_elems = p->plane_elems;
    SBA_TRY_HIP(hipMemsetAsync(p->wres_planes, 0, bytes, p->stream));
  }
  p->wres_frozen = false;
  sba::ResectWeightParams prm;
  sba::fill_resect_params(p->n, rot, tran, 0.0, &prm.P);
  prm.cov_scale = p->wres_cov_scale;
  prm.bearing_sigma2 = bearing_sigma * bearing_sigma;
  double* q[3];
  for (int k = 0; k < 3; ++k) q[k] = p->wres_planes + static_cast<size_t>(k) * p->wres_plane_elems;
  unsigned long long* counter = reinterpret_cast<unsigned long long*>(p->wres_planes + 3 * p->wres_plane_elems);
  SBA_TRY_HIP(sba::launch_resect_weights(p->store, w.pl, prm, p->wres_cov, q, counter, w.depths_grid, p->stream));
  unsigned long long zeros = 0;
  SBA_TRY_HIP(hipMemcpyAsync(&zeros, counter, sizeof(zeros), hipMemcpyDeviceToHost, p->stream));
  const int rc = sba::stream_wait(p->stream, "resection weight pass", &p->poisoned);
  if (rc) return rc;
  p->wres_n_zero = static_cast<long long>(zeros);
  p->wres_frozen = true;
  return SBA_OK;
}

int wres_set_cov(sba_problem* p, const void* cov, double cov_scale, bool from_device) {
  if (!p) return sba::set_error(SBA_ERR_INVALID_ARG, "null problem handle");
  int rc = resect_check_handle(p);
  if (rc) return rc;
  if (!cov && p->n > 0) return sba::set_error(SBA_ERR_INVALID_ARG, "null covariance array");
  if (from_device && (reinterpret_cast<uintptr_t>(cov) & 15u)) return sba::set_error(SBA_ERR_INVALID_ARG, "the covariance rows must be 16-byte aligned");
  if (const char* why = sba::resect_weight_check_scale(cov_scale)) return sba::set_error(SBA_ERR_INVALID_ARG, "%s", why);
  SBA_TRY_HIP(hipSetDevice(p->device));
  const size_t elems = 6 * p->plane_elems;       // whole vectors of matches: the freeze loads the padding too
  if (!p->wres_cov || p->wres_cov_elems != elems) {
    if (p->wres_cov) SBA_TRY_HIP(hipFree(p->wres_cov));
    p->wres_cov = nullptr; p->wres_cov_elems = 0;
    SBA_TRY_HIP(hipMalloc(reinterpret_cast<void**>(&p->wres_cov), elems * sizeof(double)));
    p->wres_cov_elems = elems;
  }
  p->wres_have_cov = false;
  p->wres_frozen = false;
  SBA_TRY_HIP(hipMemsetAsync(p->wres_cov, 0, elems * sizeof(double), p->stream));
  if (p->n > 0)
    SBA_TRY_HIP(hipMemcpyAsync(p->wres_cov, cov, 6 * p->n * sizeof(double), from_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                               p->stream));
  rc = sba::stream_wait(p->stream, "landmark covariance copy", &p->poisoned);
  if (rc) return rc;
  p->wres_cov_scale = cov_scale;
  p->wres_have_cov = true;
  return SBA_OK;
}

}  // namespace

extern "C" {

int sba_problem_resection_set_landmark_cov(sba_problem* p, const double* cov, double cov_scale) {
  return wres_set_cov(p, cov, cov_scale, false);
}

int sba_problem_resection_set_landmark_cov_device(sba_problem* p, const void* cov_dev, double cov_scale) {
  return wres_set_cov(p, cov_dev, cov_scale, true);
}

int sba_problem_resection_freeze_weights(sba_problem* p, const double rot_w[3], const double tran_w[3], double bearing_sigma,
                                         long long* n_zero_weight) {
  if (!p || !rot_w || !tran_w) return sba::set_error(SBA_ERR_INVALID_ARG, "null argument");
  int rc = wres_check(p, false);
  if (rc) return rc;
  if (const char* why = sba::resect_weight_check_sigma(bearing_sigma)) return sba::set_error(SBA_ERR_INVALID_ARG, "%s", why);
  if (!finite3(rot_w, tran_w)) return sba::set_error(SBA_ERR_NUMERIC, "non-finite rot/tran");
  ResectWork w;
  rc = wres_prepare(p, false, &w);
  if (rc) return rc;
  rc = wres_freeze(p, w, rot_w, tran_w, bearing_sigma);
  if (rc) return rc;
  if (n_zero_weight) *n_zero_weight = p->wres_n_zero;
  return SBA_OK;
}

int sba_problem_resection_weights(sba_problem* p, double* info) {
  if (!p) return sba::set_error(SBA_ERR_INVALID_ARG, "null problem handle");
  int rc = wres_check(p, true);
  if (rc) return rc;
  if (!info && p->n > 0) return sba::set_error(SBA_ERR_INVALID_ARG, "null output array");
  if (p->n == 0) return SBA_OK;
  ResectWork w;
  rc = wres_prepare(p, false, &w);
  if (rc) return rc;
  const size_t ppt = static_cast<size_t>(sba::points_per_lane(p->store));
  const size_t rows = (p->n + ppt - 1) / ppt * ppt;
  sba::DeviceBuffer buf(&p->poisoned);
  SBA_TRY_HIP(buf.alloc(rows * 6 * sizeof(double)));
  SBA_TRY_HIP(sba::launch_resect_weight_rows(p->store, w.pl, wres_planes(p), p->n, buf.as<double>(), w.depths_grid, p->stream));
  SBA_TRY_HIP(hipMemcpyAsync(info, buf.ptr, p->n * 6 * sizeof(double), hipMemcpyDeviceToHost, p->stream));
  return sba::stream_wait(p->stream, "resection weight rows", &p->poisoned);
}

int sba_problem_eval_resection_weighted(sba_problem* p, const double rot[3], const double tran[3], const sba_lm_options* opt,
                                        sba_resection_eq* out) {
  if (!p || !rot || !tran || !out) return sba::set_error(SBA_ERR_INVALID_ARG, "null argument");
  int rc = wres_check(p, true);
  if (rc) return rc;
  if (!finite3(rot, tran)) return sba::set_error(SBA_ERR_NUMERIC, "non-finite rot/tran");
  sba_lm_options o;
  if (opt) o = *opt; else sba::lm_default_options(&o);
  ResectWork w;
  rc = wres_prepare(p, o.huber_delta > 0.0, &w);
  if (rc) return rc;
  double row[sba::JOINT_ROW] = {0};
  rc = wres_reduce_pass(p, w, rot, tran, o.huber_delta, row);
  if (rc) return rc;
  rc = sba::stream_wait(p->stream, "stream synchronisation", &p->poisoned);
  if (rc) return rc;
  if (!sba::resect_row_finite(row)) return sba::set_error(SBA_ERR_NUMERIC, "non-finite weighted resection sums (non-finite data in a match with weight?)");
  sba::resect_expand_row(row, &out->eq, &out->n_behind);
  return SBA_OK;
}

int sba_problem_solve_resection_weighted(sba_problem* p, double rot[3], double tran[3], const sba_lm_options* opt, double bearing_sigma,
                                         int reweight_rounds, sba_lm_summary* summary, double* n_behind, int store_depths) {
  if (!p || !rot || !tran) return sba::set_error(SBA_ERR_INVALID_ARG, "null argument");
  int rc = wres_check(p, false);
  if (rc) return rc;
  if (const char* why = sba::resect_weight_check_sigma(bearing_sigma)) return sba::set_error(SBA_ERR_INVALID_ARG, "%s", why);
  if (const char* why = sba::resect_weight_check_rounds(reweight_rounds)) return sba::set_error(SBA_ERR_INVALID_ARG, "%s", why);
  if (!finite3(rot, tran)) return sba::set_error(SBA_ERR_NUMERIC, "non-finite rot/tran");
  sba_lm_options o;
  if (opt) o = *opt; else sba::lm_default_options(&o);
  sba_lm_summary local;
  sba_lm_summary* sum = summary ? summary : &local;
  std::memset(sum, 0, sizeof(*sum));
  const auto t_start = std::chrono::steady_clock::now();
  ResectWork w;
  rc = wres_prepare(p, o.huber_delta > 0.0, &w);
  if (rc) return rc;
  struct Visit { double rot[3], tran[3], n_behind; };
  std::vector<Visit> visits;
  double seconds_eval = 0.0;
  int eval_rc = SBA_OK;
  auto evaluate = [&](const double r[3], const double t[3], sba_normal_eq* ne) -> bool {
    const auto t0 = std::chrono::steady_clock::now();
    double row[sba::JOINT_ROW] = {0};
    eval_rc = wres_reduce_pass(p, w, r, t, o.huber_delta, row);
    seconds_eval += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (eval_rc) return false;
    if (!sba::resect_row_finite(row)) return false;
    Visit v;
    for (int a = 0; a < 3; ++a) { v.rot[a] = r[a]; v.tran[a] = t[a]; }
    sba::resect_expand_row(row, ne, &v.n_behind);
    visits.push_back(v);
    return true;
  };
  double r[3] = {rot[0], rot[1], rot[2]}, t[3] = {tran[0], tran[1], tran[2]};
  for (int round = 0; round < reweight_rounds; ++round) {
    rc = wres_freeze(p, w, r, t, bearing_sigma);
    if (rc) return rc;
    visits.clear();
    seconds_eval = 0.0;
    const int status = sba::lm_solve(SBA_MODE_RT, r, t, o, evaluate, sum);
    if (eval_rc) return eval_rc;
    rc = sba::stream_wait(p->stream, "stream synchronisation", &p->poisoned);
    if (rc) return rc;
    sum->seconds_eval = seconds_eval;
    if (status != SBA_OK) {
      sum->seconds_total = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
      return sba::set_error(status, "weighted resection solve failed in round %d: non-finite sums or 5 consecutive invalid steps", round + 1);
    }
  }
  if (store_depths) {
    sba::ResectParams prm;
    sba::fill_resect_params(p->n, r, t, 0.0, &prm);
    p->folded_valid = false;     // the d2 plane is rewritten: the next per-match sweep refolds
    SBA_TRY_HIP(sba::launch_resect_depths(p->store, w.pl, prm, p->dplane[1], w.depths_grid, p->stream));
    rc = sba::stream_wait(p->stream, "resection depth pass", &p->poisoned);
    if (rc) return rc;
  }
  if (n_behind) {
    *n_behind = 0.0;
    for (size_t k = visits.size(); k-- > 0;)
      if (std::memcmp(visits[k].rot, r, sizeof(r)) == 0 && std::memcmp(visits[k].tran, t, sizeof(t)) == 0) { *n_behind = visits[k].n_behind; break; }
  }
  for (int a = 0; a < 3; ++a) { rot[a] = r[a]; tran[a] = t[a]; }
  sum->seconds_total = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
  return SBA_OK;
}

int sba_problem_resection_covariance(sba_problem* p, const double rot[3], const double tran[3], const sba_lm_options* opt,
                                     sba_resection_cov* out) {
  if (!p || !rot || !tran || !out) return sba::set_error(SBA_ERR_INVALID_ARG, "null argument");
  int rc = wres_check(p, true);
  if (rc) return rc;
  if (!finite3(rot, tran)) return sba::set_error(SBA_ERR_NUMERIC, "non-finite rot/tran");
  sba_lm_options o;
  if (opt) o = *opt; else sba::lm_default_options(&o);
  ResectWork w;
  rc = wres_prepare(p, o.huber_delta > 0.0, &w);
  if (rc) return rc;
  double row[sba::JOINT_ROW] = {0};
  rc = wres_reduce_pass(p, w, rot, tran, o.huber_delta, row);
  if (rc) return rc;
  rc = sba::stream_wait(p->stream, "stream synchronisation", &p->poisoned);
  if (rc) return rc;
  const char* why = "";
  if (sba::resect_cov_finish(row, static_cast<long long>(p->n), p->wres_n_zero, out, &why) != SBA_OK)
    return sba::set_error(SBA_ERR_NUMERIC, "%s", why);
  return SBA_OK;
}

}  // extern "C"
