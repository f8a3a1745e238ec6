// Entry points of the robust resection guess (include/sba_hip.h): candidate poses scored against every match in one
// streaming pass, and the guess built on it -- sampled minimal DLT trials on the host, their consensus by inlier count on
// the device, a linear refit over the winner's inliers.  Kernels: sba_resection_consensus.hip; sampler, trial moments and
// pick: sba_resection_consensus.hpp; what it shares with the other resection entry points: sba_resection_entry.hpp.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <thread>
#include <vector>

#include "sba_problem.hpp"
#include "sba_resection.hpp"
#include "sba_resection_consensus.hpp"
#include "sba_resection_entry.hpp"

namespace {

// The handle's work memory of this family: [1024][12] candidate table, [1024] counts, [rows] sampled indices, [rows][6] rows.
struct ConsensusWork {
  double* table = nullptr;
  unsigned long long* counts = nullptr;
  long long* index = nullptr;
  double* rows = nullptr;
  int score_grid = 0;
};

int consensus_prepare(sba_problem* p, size_t sampled_rows, ConsensusWork* c) {
  const size_t table_bytes = size_t(SBA_RESECT_MAX_TRIALS) * SBA_RESECT_CANDIDATE * sizeof(double);
  const size_t counts_bytes = size_t(SBA_RESECT_MAX_TRIALS) * sizeof(unsigned long long);
  const size_t need = table_bytes + counts_bytes + sampled_rows * (sizeof(long long) + SBA_RESECT_ROW * sizeof(double));
  if (p->consensus_scratch_bytes < need) {
    if (p->consensus_scratch) SBA_TRY_HIP(hipFree(p->consensus_scratch));
    p->consensus_scratch = nullptr; p->consensus_scratch_bytes = 0;
    SBA_TRY_HIP(hipMalloc(&p->consensus_scratch, need));
    p->consensus_scratch_bytes = need;
  }
  char* base = static_cast<char*>(p->consensus_scratch);
  c->table = reinterpret_cast<double*>(base);
  c->counts = reinterpret_cast<unsigned long long*>(base + table_bytes);
  c->index = reinterpret_cast<long long*>(base + table_bytes + counts_bytes);
  c->rows = reinterpret_cast<double*>(base + table_bytes + counts_bytes + sampled_rows * sizeof(long long));
  // the score pass: every resident block per CU (4 with f64 planes, 3 with f32: 10.6 ms against 12.2 ms at two for 10^7 matches
  // x 1024 candidates -- more waves per SIMD cover the dependent f64 chains), capped like the other passes by SBA_RESECT_GRID
  int& occ = p->score_occ[p->store];
  if (occ == 0) {
    SBA_TRY_HIP(sba::resect_score_blocks_per_cu(p->store, &occ));
    occ = std::max(1, occ);
  }
  const size_t ppt = static_cast<size_t>(sba::points_per_lane(p->store));
  const size_t blocks = ((p->n + ppt - 1) / ppt + 255) / 256;
  int cap = 1 << 30;
  if (const char* env = std::getenv("SBA_RESECT_GRID")) { const int v = std::atoi(env); if (v >= 1) cap = v; }
  c->score_grid = static_cast<int>(std::min<size_t>({blocks, static_cast<size_t>(p->num_cus) * occ, static_cast<size_t>(cap)}));
  return SBA_OK;
}

// counts[k] of the `count` poses (rot | tran)[k]; waits for the result.
int score_poses(sba_problem* p, const ResectWork& w, const ConsensusWork& c, const double* rot, const double* tran, int count,
                double tau2, long long* n_inlier) {
  std::vector<double> table(static_cast<size_t>(count) * SBA_RESECT_CANDIDATE);
  for (int k = 0; k < count; ++k) {
    sba::ResectParams prm;
    sba::fill_resect_params(p->n, rot + 3 * k, tran + 3 * k, 0.0, &prm);
    for (int i = 0; i < 9; ++i) table[size_t(SBA_RESECT_CANDIDATE) * k + i] = prm.Rn[i];
    for (int i = 0; i < 3; ++i) table[size_t(SBA_RESECT_CANDIDATE) * k + 9 + i] = prm.t[i];
  }
  SBA_TRY_HIP(hipMemcpyAsync(c.table, table.data(), table.size() * sizeof(double), hipMemcpyHostToDevice, p->stream));
  SBA_TRY_HIP(sba::launch_resect_score(p->store, w.pl, p->n, c.table, count, tau2, c.counts, c.score_grid, p->stream));
  static_assert(sizeof(long long) == sizeof(unsigned long long), "the counts are copied out as they stand");
  SBA_TRY_HIP(hipMemcpyAsync(n_inlier, c.counts, static_cast<size_t>(count) * sizeof(long long), hipMemcpyDeviceToHost, p->stream));
  return sba::stream_wait(p->stream, "resection score pass", &p->poisoned);      // `table` lives until here
}

bool threshold_ok(double t) { return std::isfinite(t) && t > 0.0; }

}  // namespace

extern "C" {

int sba_problem_score_resection(sba_problem* p, const double* rot, const double* tran, int count, double threshold,
                                long long* n_inlier) {
  if (!p || !rot || !tran || !n_inlier) return sba::set_error(SBA_ERR_INVALID_ARG, "null argument");
  int rc = resect_check_handle(p);
  if (rc) return rc;
  if (!threshold_ok(threshold)) return sba::set_error(SBA_ERR_INVALID_ARG, "threshold must be finite and > 0");
  if (count < 1 || count > SBA_RESECT_MAX_TRIALS)
    return sba::set_error(SBA_ERR_INVALID_ARG, "count must be 1 .. %d (got %d)", int(SBA_RESECT_MAX_TRIALS), count);
  for (int i = 0; i < 3 * count; ++i)
    if (!std::isfinite(rot[i]) || !std::isfinite(tran[i])) return sba::set_error(SBA_ERR_NUMERIC, "non-finite rot/tran (candidate %d)", i / 3);
  if (p->n == 0) {
    for (int k = 0; k < count; ++k) n_inlier[k] = 0;
    return SBA_OK;
  }
  ResectWork w;
  rc = resect_prepare(p, false, &w);
  if (rc) return rc;
  ConsensusWork c;
  rc = consensus_prepare(p, 0, &c);
  if (rc) return rc;
  std::vector<long long> counts(count);
  rc = score_poses(p, w, c, rot, tran, count, threshold * threshold, counts.data());
  if (rc) return rc;
  std::memcpy(n_inlier, counts.data(), counts.size() * sizeof(long long));
  return SBA_OK;
}

int sba_problem_resection_guess_consensus(sba_problem* p, const sba_resection_consensus_options* opt, double rot[3], double tran[3],
                                          sba_resection_consensus_info* info, long long* trial_inliers, double* trial_rot,
                                          double* trial_tran) {
  if (!p || !opt || !rot || !tran || !info) return sba::set_error(SBA_ERR_INVALID_ARG, "null argument");
  int rc = resect_check_handle(p);
  if (rc) return rc;
  if (!threshold_ok(opt->threshold)) return sba::set_error(SBA_ERR_INVALID_ARG, "threshold must be finite and > 0");
  if (opt->trials < 0 || opt->trials > SBA_RESECT_MAX_TRIALS)
    return sba::set_error(SBA_ERR_INVALID_ARG, "trials must be 1 .. %d, or 0 for %d (got %d)", int(SBA_RESECT_MAX_TRIALS),
                          int(SBA_RESECT_DEFAULT_TRIALS), opt->trials);
  if (opt->sample_size != 0 && (opt->sample_size < SBA_RESECT_MIN_SAMPLE || opt->sample_size > SBA_RESECT_MAX_SAMPLE))
    return sba::set_error(SBA_ERR_INVALID_ARG, "sample_size must be %d .. %d, or 0 for %d (got %d)", int(SBA_RESECT_MIN_SAMPLE),
                          int(SBA_RESECT_MAX_SAMPLE), int(SBA_RESECT_MIN_SAMPLE), opt->sample_size);
  const int trials = opt->trials ? opt->trials : SBA_RESECT_DEFAULT_TRIALS;
  const int m = opt->sample_size ? opt->sample_size : SBA_RESECT_MIN_SAMPLE;
  if (p->n < static_cast<size_t>(m))
    return sba::set_error(SBA_ERR_NUMERIC, "a trial draws %d distinct matches (the handle holds %zu)", m, p->n);
  const double tau2 = opt->threshold * opt->threshold;
  ResectWork w;
  rc = resect_prepare(p, false, &w);
  if (rc) return rc;
  ConsensusWork c;
  const size_t nrows = static_cast<size_t>(trials) * m;
  rc = consensus_prepare(p, nrows, &c);
  if (rc) return rc;

  // sample on the host, gather on the device (the handle's data may never have been on the host), rows back in one copy
  std::vector<long long> index(nrows);
  for (int t = 0; t < trials; ++t) sba::resect_sample_trial(opt->seed, t, p->n, m, index.data() + static_cast<size_t>(t) * m);
  std::vector<double> rows(nrows * SBA_RESECT_ROW);
  SBA_TRY_HIP(hipMemcpyAsync(c.index, index.data(), nrows * sizeof(long long), hipMemcpyHostToDevice, p->stream));
  SBA_TRY_HIP(sba::launch_resect_gather(p->store, w.pl, c.index, static_cast<int>(nrows), c.rows, p->stream));
  SBA_TRY_HIP(hipMemcpyAsync(rows.data(), c.rows, rows.size() * sizeof(double), hipMemcpyDeviceToHost, p->stream));
  rc = sba::stream_wait(p->stream, "resection gather", &p->poisoned);
  if (rc) return rc;

  // the trials: each on its own rows, spread over the host threads in contiguous ranges -- no trial reads another's result
  std::vector<double> t_rot(3 * static_cast<size_t>(trials), 0.0), t_tran(3 * static_cast<size_t>(trials), 0.0);
  std::vector<char> t_ok(trials, 0);
  auto run = [&](int first, int last) {
    for (int t = first; t < last; ++t) {
      sba_resection_guess_info gi;
      t_ok[t] = sba::resect_trial_pose(rows.data() + static_cast<size_t>(t) * m * SBA_RESECT_ROW, m, &t_rot[3 * t], &t_tran[3 * t], &gi) == SBA_OK;
      if (!t_ok[t]) for (int a = 0; a < 3; ++a) t_rot[3 * t + a] = t_tran[3 * t + a] = 0.0;
    }
  };
  const int nt = std::max(1, std::min(sba::host_threads(), trials));
  if (nt == 1) {
    run(0, trials);
  } else {
    std::vector<std::thread> pool;
    for (int t = 1; t < nt; ++t)
      pool.emplace_back(run, static_cast<int>(static_cast<long long>(trials) * t / nt), static_cast<int>(static_cast<long long>(trials) * (t + 1) / nt));
    run(0, static_cast<int>(static_cast<long long>(trials) / nt));
    for (auto& th : pool) th.join();
  }

  // score the trials that finished, packed; a refused trial keeps the count -1
  std::vector<int> slot;
  std::vector<double> c_rot, c_tran;
  for (int t = 0; t < trials; ++t)
    if (t_ok[t]) {
      slot.push_back(t);
      c_rot.insert(c_rot.end(), &t_rot[3 * t], &t_rot[3 * t] + 3);
      c_tran.insert(c_tran.end(), &t_tran[3 * t], &t_tran[3 * t] + 3);
    }
  if (slot.empty())
    return sba::set_error(SBA_ERR_NUMERIC, "none of the %d trials finished: every sample of %d matches is degenerate (a planar set?)", trials, m);
  std::vector<long long> packed(slot.size()), counts(trials, -1);
  rc = score_poses(p, w, c, c_rot.data(), c_tran.data(), static_cast<int>(slot.size()), tau2, packed.data());
  if (rc) return rc;
  for (size_t k = 0; k < slot.size(); ++k) counts[slot[k]] = packed[k];
  const int best = sba::resect_pick(counts.data(), trials);

  sba_resection_consensus_info res;
  std::memset(&res, 0, sizeof(res));
  res.n = static_cast<long long>(p->n);
  res.best_trial = best;
  res.best_trial_inliers = counts[best];
  res.n_valid_trials = static_cast<long long>(slot.size());
  res.n_inlier = counts[best];
  double r[3] = {t_rot[3 * best], t_rot[3 * best + 1], t_rot[3 * best + 2]};
  double t[3] = {t_tran[3 * best], t_tran[3 * best + 1], t_tran[3 * best + 2]};

  if (opt->refit) {
    // the DLT moments over the pick's inliers only, the finish, and the refit's own score: kept if it is no worse
    sba::ResectParams prm;
    sba::fill_resect_params(p->n, r, t, opt->threshold, &prm);      // delta2 = threshold * threshold = tau2
    double row[sba::JOINT_ROW] = {0};
    const unsigned long long seq = ++p->joint_seq;
    SBA_TRY_HIP(sba::launch_resect_inlier_moments(p->store, w.pl, prm, w.partials, w.moments_grid, w.out_dev,
                                                  p->publish ? p->joint_host_dev : nullptr, seq, p->stream));
    rc = resect_fetch(p, w, seq, SBA_RESECT_MOM_COUNT, "resection inlier moments pass", row);
    if (rc) return rc;
    double rr[3], rt[3];
    const char* why = "";
    if (sba::resect_dlt_finish(row, row[SBA_RESECT_MOM_N], rr, rt, &res.refit, &why) == SBA_OK) {
      long long refit_count = 0;
      rc = score_poses(p, w, c, rr, rt, 1, tau2, &refit_count);
      if (rc) return rc;
      if (refit_count >= res.n_inlier) {
        res.refit_used = 1;
        res.n_inlier = refit_count;
        for (int a = 0; a < 3; ++a) { r[a] = rr[a]; t[a] = rt[a]; }
      }
    }
  }

  double eq_row[sba::JOINT_ROW] = {0};
  rc = resect_reduce_pass(p, w, r, t, 0.0, eq_row);       // n_behind at the returned pose
  if (rc) return rc;
  rc = sba::stream_wait(p->stream, "stream synchronisation", &p->poisoned);
  if (rc) return rc;
  if (!sba::resect_row_finite(eq_row)) return sba::set_error(SBA_ERR_NUMERIC, "non-finite resection sums at the consensus result");
  res.n_behind = eq_row[SBA_RESECT_NBEHIND];
  *info = res;
  if (trial_inliers) std::memcpy(trial_inliers, counts.data(), static_cast<size_t>(trials) * sizeof(long long));
  if (trial_rot) std::memcpy(trial_rot, t_rot.data(), t_rot.size() * sizeof(double));
  if (trial_tran) std::memcpy(trial_tran, t_tran.data(), t_tran.size() * sizeof(double));
  for (int a = 0; a < 3; ++a) { rot[a] = r[a]; tran[a] = t[a]; }
  return SBA_OK;
}

}  // extern "C"
