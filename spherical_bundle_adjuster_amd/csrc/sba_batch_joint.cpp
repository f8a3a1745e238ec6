// Entry points of the batched joint solve (include/sba_hip.h): every pair's depths, rotation and translation free together --
// what sba_problem_eval_joint / sba_problem_solve_joint do for one problem, per pair of a batch, on the batch's resident planes.
// Kernels: sba_batch_joint.hip; step logic: sba_joint_solver.hpp (one JointSolver per pair, on the device or -- lock-step -- here).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sba_batch.hpp"
#include "sba_joint_solver.hpp"
#include "sba_lm.hpp"

namespace {

struct BatchJointWork {
  sba::Planes pl;
  double *c1 = nullptr, *c2 = nullptr, *sc1 = nullptr, *sc2 = nullptr;
  volatile unsigned long long* flag = nullptr;      // the sequence word behind the rows, host / device address
  unsigned long long* flag_dev = nullptr;
};

int batch_joint_check(sba_batch* b, const double* rot, const double* tran) {
  if (!b) return sba::set_error(SBA_ERR_INVALID_ARG, "null batch handle");
  SBA_REFUSE_POISONED(b);
  if (!b->uploaded) return sba::set_error(SBA_ERR_NOT_UPLOADED, "no pairs uploaded");
  if (b->num_pairs > 0 && (!rot || !tran)) return sba::set_error(SBA_ERR_INVALID_ARG, "rot/tran must not be null");
  if (!b->has_d12)
    return sba::set_error(SBA_ERR_UNSUPPORTED, "the joint solve needs per-match depths (upload d12)");
  if (!b->publish && b->num_pairs > 0)
    return sba::set_error(SBA_ERR_UNSUPPORTED, "the batched joint solve needs host-mapped publication (SBA_PUBLISH=0 is set)");
  return SBA_OK;
}

void batch_joint_options(const sba_lm_options* opt, sba_lm_options* o) {
  if (opt) { *o = *opt; return; }
  sba::lm_default_options(o);
  o->tran_param = SBA_TRAN_SPHERE;     // the gauge: with a free translation (d, t) -> 0 minimises the cost
}

// Work planes (the d-only stage's: the two stages never overlap) and the mapped buffers, allocated on first use.
int batch_joint_prepare(sba_batch* b, BatchJointWork* w, bool zero_candidates) {
  SBA_TRY_HIP(hipSetDevice(b->device));
  const size_t B = static_cast<size_t>(b->num_pairs), elems = b->plane_elems;
  { const int rc = sba::batch::ensure_depth_work(b); if (rc) return rc; }
  if (!b->joint_out_host) {
    SBA_TRY_HIP(hipHostMalloc(reinterpret_cast<void**>(&b->joint_pass_host), sizeof(sba::BatchJointPass) * B,
                              hipHostMallocMapped | hipHostMallocCoherent));
    std::memset(b->joint_pass_host, 0, sizeof(sba::BatchJointPass) * B);
    SBA_TRY_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&b->joint_pass_host_dev), b->joint_pass_host, 0));
    SBA_TRY_HIP(hipHostMalloc(reinterpret_cast<void**>(&b->joint_out_host), sizeof(double) * (B * sba::JOINT_ROW + 8),
                              hipHostMallocMapped | hipHostMallocCoherent));
    std::memset(b->joint_out_host, 0, sizeof(double) * (B * sba::JOINT_ROW + 8));
    SBA_TRY_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&b->joint_out_host_dev), b->joint_out_host, 0));
    b->joint_seq = 0;
  }
  double* work = b->depth_work;
  w->c1 = work; w->c2 = work + elems; w->sc1 = work + 2 * elems; w->sc2 = work + 3 * elems;
  // zeroed on entry: an accepted candidate plane becomes a depth plane, whose padding must be zeros like an uploaded plane's
  if (zero_candidates) SBA_TRY_HIP(hipMemsetAsync(work, 0, 2 * elems * sizeof(double), b->stream));
  for (int k = 0; k < 3; ++k) { w->pl.x1[k] = b->coord[k]; w->pl.x2[k] = b->coord[3 + k]; }
  w->pl.d1 = b->dplane[0]; w->pl.d2 = b->dplane[1];
  w->flag = reinterpret_cast<volatile unsigned long long*>(b->joint_out_host + B * sba::JOINT_ROW);
  w->flag_dev = reinterpret_cast<unsigned long long*>(b->joint_out_host_dev + B * sba::JOINT_ROW);
  return SBA_OK;
}

// One launch of batch_joint_pass_kernel over the records in b->joint_pass_host; the rows are in b->joint_out_host afterwards.
int batch_joint_pass(sba_batch* b, const BatchJointWork& w, const sba_lm_options& o, const char* what) {
  const unsigned long long seq = ++b->joint_seq;
  SBA_TRY_HIP(sba::launch_batch_joint_pass(b->store, w.pl, b->desc_dev, b->joint_pass_host_dev, b->num_pairs, o, b->dplane[0], b->dplane[1],
                                           w.c1, w.c2, w.sc1, w.sc2, b->joint_out_host_dev, b->lm_ticket, seq, b->stream));
  return sba::wait_for_sequence(w.flag, seq, b->stream, what, &b->poisoned);
}

bool finite3(const double* v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }

}  // namespace

namespace sba {
namespace batch {

int joint_check(sba_batch* b, const double* rot, const double* tran) { return batch_joint_check(b, rot, tran); }
void joint_options(const sba_lm_options* opt, sba_lm_options* o) { batch_joint_options(opt, o); }

}  // namespace batch
}  // namespace sba

extern "C" {

int sba_batch_eval_joint(sba_batch* b, const double* rot, const double* tran, double radius, const sba_lm_options* opt,
                         sba_joint_eq* out) {
  int rc = batch_joint_check(b, rot, tran);
  if (rc) return rc;
  if (!(radius > 0.0)) return sba::set_error(SBA_ERR_INVALID_ARG, "radius must be positive (+inf: no depth damping)");
  const int B = b->num_pairs;
  if (B == 0) return SBA_OK;
  if (!out) return sba::set_error(SBA_ERR_INVALID_ARG, "out is null");
  for (int g = 0; g < B; ++g)
    if (!finite3(rot + 3 * g) || !finite3(tran + 3 * g)) return sba::set_error(SBA_ERR_NUMERIC, "non-finite rot/tran of pair %d", g);
  sba_lm_options o;
  batch_joint_options(opt, &o);
  BatchJointWork w;
  rc = batch_joint_prepare(b, &w, false);
  if (rc) return rc;
  for (int g = 0; g < B; ++g) {
    sba::BatchJointPass& ps = b->joint_pass_host[g];
    ps = sba::BatchJointPass{};
    for (int a = 0; a < 3; ++a) { ps.rot[a] = rot[3 * g + a]; ps.tran[a] = tran[3 * g + a]; }
    ps.radius = radius; ps.n = b->n[g]; ps.kind = sba::kJointReduce; ps.flags = 1u;     // as a solve's first pass: the scaling is computed here
  }
  rc = batch_joint_pass(b, w, o, "batched joint reduce pass");
  if (rc) return rc;
  for (int g = 0; g < B; ++g) {
    const double* row = b->joint_out_host + static_cast<size_t>(g) * sba::JOINT_ROW;
    sba_normal_eq full, red;
    sba::expand_pack(SBA_MODE_RT, row + sba::JOINT_OUT_PACK, &full);
    sba::joint_expand_reduced(row, &red);
    sba_joint_eq& e = out[g];
    std::memcpy(e.S, red.H, sizeof(e.S)); std::memcpy(e.gs, red.g, sizeof(e.gs));
    std::memcpy(e.V, full.H, sizeof(e.V)); std::memcpy(e.gc, full.g, sizeof(e.gc));
    e.cost = full.cost; e.sum_w = full.sum_w; e.n_outlier = full.n_outlier;
    e.gd_max = row[sba::JOINT_OUT_GDMAX];
  }
  return SBA_OK;
}

int sba_batch_solve_joint(sba_batch* b, double* rot, double* tran, const sba_lm_options* opt, sba_lm_summary* summaries, int* status,
                          double* d12_out) {
  int rc = batch_joint_check(b, rot, tran);
  if (rc) return rc;
  const int B = b->num_pairs;
  if (B == 0) return SBA_OK;
  sba_lm_options o;
  batch_joint_options(opt, &o);
  const auto t_start = std::chrono::steady_clock::now();
  BatchJointWork w;
  rc = batch_joint_prepare(b, &w, true);
  if (rc) return rc;
  const size_t base = b->offsets.front(), total = b->offsets.back() - base;
  const bool want_out = d12_out && total > 0;
  sba::DeviceBuffer out_dev(&b->poisoned), flip_dev(&b->poisoned);
  if (want_out) SBA_TRY_HIP(out_dev.alloc(2 * total * sizeof(double)));
  std::vector<unsigned char> refused(B, 0);      // a non-finite start: SBA_ERR_NUMERIC for that pair, its depths unchanged
  for (int g = 0; g < B; ++g) refused[g] = finite3(rot + 3 * g) && finite3(tran + 3 * g) ? 0 : 1;

  bool device_solve = true;      // SBA_BATCH_DEVICE_JOINT=0: host solvers in lock-step, one launch per pass (the second oracle)
  if (const char* env = std::getenv("SBA_BATCH_DEVICE_JOINT")) device_solve = std::strcmp(env, "0") != 0;
  std::vector<sba_lm_summary> sum_local(B);
  std::vector<int> st_local(B, SBA_OK);
  if (device_solve) {
    sba::BatchLmIo* io = b->lm_io_host;
    for (int g = 0; g < B; ++g) {
      io[g] = sba::BatchLmIo{};
      for (int a = 0; a < 3; ++a) { io[g].rot[a] = rot[3 * g + a]; io[g].tran[a] = tran[3 * g + a]; }
      io[g].status = refused[g] ? SBA_ERR_NUMERIC : SBA_OK;
    }
    const unsigned long long seq = ++b->joint_seq;
    SBA_TRY_HIP(sba::launch_batch_joint_solve(b->store, w.pl, b->desc_dev, B, o, b->dplane[0], b->dplane[1], w.c1, w.c2, w.sc1, w.sc2,
                                              b->offsets_dev, want_out ? out_dev.as<double>() : nullptr, b->lm_io_host_dev, b->lm_ticket,
                                              w.flag_dev, seq, b->stream));
    rc = sba::wait_for_sequence(w.flag, seq, b->stream, "batched joint solve", &b->poisoned);
    if (rc) return rc;
    for (int g = 0; g < B; ++g) {
      sum_local[g] = io[g].summary; st_local[g] = io[g].status;
      if (!refused[g]) for (int a = 0; a < 3; ++a) { rot[3 * g + a] = io[g].rot[a]; tran[3 * g + a] = io[g].tran[a]; }
    }
  } else {
    std::vector<sba::JointSolver> solver(B);
    std::vector<unsigned char> flip(B, 0), active(B, 1);
    int remaining = 0;
    for (int g = 0; g < B; ++g) {
      solver[g].start(rot + 3 * g, tran + 3 * g, o);
      if (refused[g]) active[g] = 0; else ++remaining;
    }
    const int max_passes = sba::batch_joint_pass_bound(o);
    for (int pass = 0; remaining > 0 && pass < max_passes; ++pass) {
      for (int g = 0; g < B; ++g) {
        sba::BatchJointPass& ps = b->joint_pass_host[g];
        ps = sba::BatchJointPass{};
        ps.radius = 1.0;
        if (!active[g]) continue;                         // n = 0: the pair is finished
        const sba::JointPassRequest& rq = solver[g].request();
        for (int a = 0; a < 3; ++a) { ps.rot[a] = rq.rot[a]; ps.tran[a] = rq.tran[a]; ps.rot_cand[a] = rq.rot_cand[a]; ps.tran_cand[a] = rq.tran_cand[a]; }
        for (int k = 0; k < 6; ++k) ps.delta_c[k] = rq.delta_c[k];
        ps.radius = rq.radius; ps.n = b->n[g]; ps.kind = static_cast<unsigned>(rq.kind);
        ps.flags = (rq.first ? 1u : 0u) | (flip[g] ? 8u : 0u);
      }
      rc = batch_joint_pass(b, w, o, "batched joint pass");
      if (rc) return rc;
      for (int g = 0; g < B; ++g) {
        if (!active[g]) continue;
        solver[g].feed(b->joint_out_host + static_cast<size_t>(g) * sba::JOINT_ROW);
        if (solver[g].take_candidate()) flip[g] ^= 1;
        if (solver[g].done()) { active[g] = 0; --remaining; }
      }
    }
    // results back into the batch's own depth planes (pairs that ended on an odd number of accepted steps), and out to the host
    for (unsigned char& f : flip) f = static_cast<unsigned char>((f & 1) | 2);      // bit 0: copy back; bit 1: write `out`
    SBA_TRY_HIP(flip_dev.alloc(static_cast<size_t>(B)));
    SBA_TRY_HIP(hipMemcpyAsync(flip_dev.ptr, flip.data(), static_cast<size_t>(B), hipMemcpyHostToDevice, b->stream));
    SBA_TRY_HIP(sba::launch_batch_depth_finish(b->store, b->desc_dev, flip_dev.as<unsigned char>(), B, b->dplane[0], b->dplane[1], w.c1, w.c2,
                                               b->offsets_dev, want_out ? out_dev.as<double>() : nullptr, b->stream));
    for (int g = 0; g < B; ++g) {
      sum_local[g] = solver[g].summary();
      // a pair the pass bound ran out on: never silent
      st_local[g] = refused[g] ? SBA_ERR_NUMERIC : (solver[g].done() ? solver[g].status() : SBA_ERR_NUMERIC);
      if (!refused[g]) for (int a = 0; a < 3; ++a) { rot[3 * g + a] = solver[g].rot()[a]; tran[3 * g + a] = solver[g].tran()[a]; }
    }
  }
  if (want_out)
    SBA_TRY_HIP(hipMemcpyAsync(d12_out + 2 * base, out_dev.ptr, 2 * total * sizeof(double), hipMemcpyDeviceToHost, b->stream));
  rc = sba::stream_wait(b->stream, "batched joint solve", &b->poisoned);
  if (rc) return rc;
  const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
  int failures = 0;
  for (int g = 0; g < B; ++g) {
    if (summaries) { summaries[g] = sum_local[g]; summaries[g].seconds_total = seconds; }   // wall clock of the whole batch
    if (status) status[g] = st_local[g];
    if (st_local[g] != SBA_OK) ++failures;
  }
  if (failures) return sba::set_error(SBA_ERR_NUMERIC, "%d of %d pairs failed in the joint solve (see per-pair status)", failures, B);
  return SBA_OK;
}

}  // extern "C"
