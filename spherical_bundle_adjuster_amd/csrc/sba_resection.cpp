// Entry points of the spherical resection (include/sba_hip.h): a new frame's pose from the handle's landmarks X_i = d1_i x1_i
// and bearings y_i = x2_i, the bearing's depth eliminated in closed form.  Kernels: sba_resection.hip; row layouts, the DLT
// finish and the log map: sba_resection.hpp; the LM schedule is sba_lm.hpp's, driven through its evaluator callback.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sba_lm.hpp"
#include "sba_problem.hpp"
#include "sba_resection.hpp"
#include "sba_resection_entry.hpp"

namespace {

int resect_check(sba_problem* p, const double* rot, const double* tran) {
  if (!p || !rot || !tran) return sba::set_error(SBA_ERR_INVALID_ARG, "null argument");
  const int rc = resect_check_handle(p);
  if (rc) return rc;
  for (int i = 0; i < 3; ++i)
    if (!std::isfinite(rot[i]) || !std::isfinite(tran[i])) return sba::set_error(SBA_ERR_NUMERIC, "non-finite rot/tran");
  return SBA_OK;
}

int resect_store_depths(sba_problem* p, const ResectWork& w, const double rot[3], const double tran[3], double* d2_out) {
  sba::ResectParams prm;
  sba::fill_resect_params(p->n, rot, tran, 0.0, &prm);
  p->folded_valid = false;     // the d2 plane is rewritten: the next per-match sweep refolds
  SBA_TRY_HIP(sba::launch_resect_depths(p->store, w.pl, prm, p->dplane[1], w.depths_grid, p->stream));
  if (d2_out && p->n > 0)
    SBA_TRY_HIP(hipMemcpyAsync(d2_out, p->dplane[1], p->n * sizeof(double), hipMemcpyDeviceToHost, p->stream));
  return sba::stream_wait(p->stream, "resection depth pass", &p->poisoned);
}

}  // namespace

extern "C" {

int sba_problem_eval_resection(sba_problem* p, const double rot[3], const double tran[3], const sba_lm_options* opt,
                               sba_resection_eq* out) {
  if (!out) return sba::set_error(SBA_ERR_INVALID_ARG, "null argument");
  int rc = resect_check(p, rot, tran);
  if (rc) return rc;
  sba_lm_options o;
  if (opt) o = *opt; else sba::lm_default_options(&o);
  ResectWork w;
  rc = resect_prepare(p, o.huber_delta > 0.0, &w);
  if (rc) return rc;
  double row[sba::JOINT_ROW] = {0};
  rc = resect_reduce_pass(p, w, rot, tran, o.huber_delta, row);
  if (rc) return rc;
  rc = sba::stream_wait(p->stream, "stream synchronisation", &p->poisoned);
  if (rc) return rc;
  if (!sba::resect_row_finite(row)) return sba::set_error(SBA_ERR_NUMERIC, "non-finite resection sums (a zero bearing, non-finite data?)");
  sba::resect_expand_row(row, &out->eq, &out->n_behind);
  return SBA_OK;
}

int sba_problem_solve_resection(sba_problem* p, double rot[3], double tran[3], const sba_lm_options* opt, sba_lm_summary* summary,
                                double* n_behind, int store_depths) {
  int rc = resect_check(p, rot, tran);
  if (rc) return rc;
  sba_lm_options o;
  if (opt) o = *opt; else sba::lm_default_options(&o);     // the defaults carry SBA_TRAN_FREE: the landmarks fix the scale
  sba_lm_summary local;
  sba_lm_summary* sum = summary ? summary : &local;
  std::memset(sum, 0, sizeof(*sum));
  const auto t_start = std::chrono::steady_clock::now();
  ResectWork w;
  rc = resect_prepare(p, o.huber_delta > 0.0, &w);
  if (rc) return rc;
  struct Visit { double rot[3], tran[3], n_behind; };
  std::vector<Visit> visits;          // every evaluated point: the result is one of them
  double seconds_eval = 0.0;
  int eval_rc = SBA_OK;
  auto evaluate = [&](const double r[3], const double t[3], sba_normal_eq* ne) -> bool {
    const auto t0 = std::chrono::steady_clock::now();
    double row[sba::JOINT_ROW] = {0};
    eval_rc = resect_reduce_pass(p, w, r, t, o.huber_delta, row);
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
  const int status = sba::lm_solve(SBA_MODE_RT, r, t, o, evaluate, sum);
  if (eval_rc) return eval_rc;       // a bounded wait or a HIP call failed: the message is set, the wait has poisoned the handle
  rc = sba::stream_wait(p->stream, "stream synchronisation", &p->poisoned);
  if (rc) return rc;
  sum->seconds_eval = seconds_eval;
  if (status != SBA_OK) {
    sum->seconds_total = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
    return sba::set_error(status, "resection solve failed: non-finite sums or 5 consecutive invalid steps");
  }
  if (store_depths) {
    rc = resect_store_depths(p, w, r, t, nullptr);
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

int sba_problem_resection_depths(sba_problem* p, const double rot[3], const double tran[3], double* d2_out) {
  int rc = resect_check(p, rot, tran);
  if (rc) return rc;
  ResectWork w;
  rc = resect_prepare(p, false, &w);
  if (rc) return rc;
  return resect_store_depths(p, w, rot, tran, d2_out);
}

int sba_problem_resection_guess(sba_problem* p, double rot[3], double tran[3], sba_resection_guess_info* info, double* moments) {
  if (!p || !rot || !tran || !info) return sba::set_error(SBA_ERR_INVALID_ARG, "null argument");
  int rc = resect_check_handle(p);
  if (rc) return rc;
  if (p->n < 6) return sba::set_error(SBA_ERR_NUMERIC, "the linear resection needs at least 6 matches (the handle holds %zu)", p->n);
  ResectWork w;
  rc = resect_prepare(p, false, &w);
  if (rc) return rc;
  double row[sba::JOINT_ROW] = {0};
  const unsigned long long seq = ++p->joint_seq;
  SBA_TRY_HIP(sba::launch_resect_moments(p->store, w.pl, p->n, w.partials, w.moments_grid, w.out_dev,
                                         p->publish ? p->joint_host_dev : nullptr, seq, p->stream));
  rc = resect_fetch(p, w, seq, SBA_RESECT_MOM_COUNT, "resection moments pass", row);
  if (rc) return rc;
  double r[3], t[3];
  sba_resection_guess_info res;
  const char* why = "";
  if (sba::resect_dlt_finish(row, row[SBA_RESECT_MOM_N], r, t, &res, &why) != SBA_OK) {
    rc = sba::stream_wait(p->stream, "stream synchronisation", &p->poisoned);
    if (rc) return rc;
    return sba::set_error(SBA_ERR_NUMERIC, "%s", why);
  }
  double eq_row[sba::JOINT_ROW] = {0};
  rc = resect_reduce_pass(p, w, r, t, 0.0, eq_row);       // n_behind at the result
  if (rc) return rc;
  rc = sba::stream_wait(p->stream, "stream synchronisation", &p->poisoned);
  if (rc) return rc;
  if (!sba::resect_row_finite(eq_row)) return sba::set_error(SBA_ERR_NUMERIC, "non-finite resection sums at the linear result");
  res.n_behind = eq_row[SBA_RESECT_NBEHIND];
  *info = res;
  if (moments) std::memcpy(moments, row, SBA_RESECT_MOMENTS * sizeof(double));
  for (int a = 0; a < 3; ++a) { rot[a] = r[a]; tran[a] = t[a]; }
  return SBA_OK;
}

}  // extern "C"
