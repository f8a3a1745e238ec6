// Entry points of the joint solve (include/sba_hip.h): depths, rotation and translation free together -- the reference's
// ba_spherical_costfunctor (spherical_bundle_adjuster.cpp:843-889).  Kernels: sba_joint.hip; step logic: sba_joint_solver.hpp.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "sba_joint_solver.hpp"
#include "sba_lm.hpp"
#include "sba_problem.hpp"
#include "sba_rotation.hpp"

namespace {

// What a joint call needs from the handle, set up once per call: the work planes (candidate depths, depth scaling), the
// block rows and the mapped host row the finalize kernel publishes to.
struct JointWork {
  sba::Planes pl;
  double *c1 = nullptr, *c2 = nullptr, *sc1 = nullptr, *sc2 = nullptr, *out_dev = nullptr, *partials = nullptr;
  size_t elems = 0;
  int grid = 0;
};

int joint_check(sba_problem* p, const double* rot, const double* tran) {
  if (!p || !rot || !tran) return sba::set_error(SBA_ERR_INVALID_ARG, "null argument");
  SBA_REFUSE_POISONED(p);
  if (!p->uploaded) return sba::set_error(SBA_ERR_NOT_UPLOADED, "no correspondences uploaded");
  if (sba::shim::is_collective(p) || p->shard_count != 1)
    return sba::set_error(SBA_ERR_UNSUPPORTED, "the joint solve runs on one unsharded problem: its reduction row (%d doubles) is wider "
                                               "than the %d-double exchange of the transports", int(sba::JOINT_OUT_COUNT), int(SBA_PACK_SIZE));
  if (!p->has_d12 && p->n > 0)
    return sba::set_error(SBA_ERR_UNSUPPORTED, "the joint solve needs per-match depths (upload d12 or call sba_problem_set_depths)");
  for (int i = 0; i < 3; ++i)
    if (!std::isfinite(rot[i]) || !std::isfinite(tran[i])) return sba::set_error(SBA_ERR_NUMERIC, "non-finite rot/tran");
  return SBA_OK;
}

int joint_prepare(sba_problem* p, JointWork* w) {
  SBA_TRY_HIP(hipSetDevice(p->device));
  if (!p->joint_host) {
    SBA_TRY_HIP(hipHostMalloc(reinterpret_cast<void**>(&p->joint_host), (sba::JOINT_ROW + 8) * sizeof(double),
                              hipHostMallocMapped | hipHostMallocCoherent));
    std::memset(p->joint_host, 0, (sba::JOINT_ROW + 8) * sizeof(double));
    SBA_TRY_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&p->joint_host_dev), p->joint_host, 0));
  }
  const size_t n = p->n, elems = std::max<size_t>(p->plane_elems, 2);
  // Work planes and rows live in the handle's d-only scratch (the two stages never overlap; the d-only stage re-zeroes
  // its planes on entry and keeps a block that is large enough).
  const size_t max_grid_rows = static_cast<size_t>(p->num_cus) * 16 + 1;
  const size_t need = (4 * elems + (max_grid_rows + 1) * sba::JOINT_ROW) * sizeof(double);
  if (p->depth_scratch_bytes < need) {
    if (p->depth_scratch) SBA_TRY_HIP(hipFree(p->depth_scratch));
    p->depth_scratch = nullptr; p->depth_scratch_bytes = 0;
    SBA_TRY_HIP(hipMalloc(&p->depth_scratch, need));
    p->depth_scratch_bytes = need;
  }
  double* work = static_cast<double*>(p->depth_scratch);
  // zeroed: an accepted candidate plane becomes a depth plane, whose padding must be zeros like an uploaded plane's
  SBA_TRY_HIP(hipMemsetAsync(work, 0, 4 * elems * sizeof(double), p->stream));
  w->elems = elems;
  w->c1 = work; w->c2 = work + elems; w->sc1 = work + 2 * elems; w->sc2 = work + 3 * elems;
  w->out_dev = work + 4 * elems; w->partials = w->out_dev + sba::JOINT_ROW;
  int& occ = p->joint_occ[p->store];
  if (occ == 0) {
    SBA_TRY_HIP(sba::joint_blocks_per_cu(p->store, &occ));
    occ = std::max(1, occ);
  }
  w->grid = sba::joint_grid((n + 1) / 2, p->num_cus, occ);
  for (int k = 0; k < 3; ++k) { w->pl.x1[k] = p->coord[k]; w->pl.x2[k] = p->coord[3 + k]; }
  w->pl.d1 = p->dplane[0]; w->pl.d2 = p->dplane[1];
  return SBA_OK;
}

void joint_camera(size_t n, const double rot[3], const double tran[3], double huber_delta, sba::SweepParams* prm) {
  sba::fill_sweep_params(n, SBA_DEPTH_PER_MATCH, rot, tran, 1.0, 1.0, huber_delta, prm, false);
}

// Wait for the row of the pass enqueued last and copy `count` results out.
int joint_fetch(sba_problem* p, const JointWork& w, unsigned long long seq, int count, const char* what, double* row) {
  if (p->publish) {
    const int rc = sba::wait_for_sequence(reinterpret_cast<volatile unsigned long long*>(p->joint_host + sba::JOINT_ROW), seq, p->stream,
                                          what, &p->poisoned);
    if (rc) return rc;
  } else {
    SBA_TRY_HIP(hipMemcpyAsync(p->joint_host, w.out_dev, count * sizeof(double), hipMemcpyDeviceToHost, p->stream));
    const int rc = sba::stream_wait(p->stream, what, &p->poisoned);
    if (rc) return rc;
  }
  std::memcpy(row, p->joint_host, count * sizeof(double));
  return SBA_OK;
}

int joint_reduce_pass(sba_problem* p, const JointWork& w, const double* d1, const double* d2, const double rot[3], const double tran[3],
                      double radius, bool first, const sba_lm_options& o, double* row) {
  sba::JointParams prm{};
  joint_camera(p->n, rot, tran, o.huber_delta, &prm.cur);
  prm.cand = prm.cur;
  double B[9];
  sba::factored_frame(rot, B, prm.J);
  prm.small_angle = !(rot[0] * rot[0] + rot[1] * rot[1] + rot[2] * rot[2] > DBL_EPSILON) ? 1 : 0;
  prm.inv_radius = 1.0 / radius;
  prm.min_diagonal = o.min_lm_diagonal; prm.max_diagonal = o.max_lm_diagonal;
  prm.first = first ? 1 : 0; prm.jacobi_scaling = o.jacobi_scaling ? 1 : 0;
  const unsigned long long seq = ++p->joint_seq;
  SBA_TRY_HIP(sba::launch_joint_reduce(p->store, w.pl, d1, d2, w.sc1, w.sc2, prm, w.partials, w.grid, w.out_dev,
                                       p->publish ? p->joint_host_dev : nullptr, seq, p->stream));
  return joint_fetch(p, w, seq, sba::JOINT_OUT_COUNT, "joint reduce pass", row);
}

int joint_step_pass(sba_problem* p, const JointWork& w, const double* d1, const double* d2, double* c1, double* c2,
                    const sba::JointPassRequest& rq, const sba_lm_options& o, double* row) {
  sba::JointParams prm{};
  joint_camera(p->n, rq.rot, rq.tran, o.huber_delta, &prm.cur);
  joint_camera(p->n, rq.rot_cand, rq.tran_cand, o.huber_delta, &prm.cand);
  double B[9];
  sba::factored_frame(rq.rot, B, prm.J);
  prm.small_angle = !(rq.rot[0] * rq.rot[0] + rq.rot[1] * rq.rot[1] + rq.rot[2] * rq.rot[2] > DBL_EPSILON) ? 1 : 0;
  for (int k = 0; k < 6; ++k) prm.delta_c[k] = rq.delta_c[k];
  prm.inv_radius = 1.0 / rq.radius;
  prm.min_diagonal = o.min_lm_diagonal; prm.max_diagonal = o.max_lm_diagonal;
  prm.first = 0; prm.jacobi_scaling = o.jacobi_scaling ? 1 : 0;
  const unsigned long long seq = ++p->joint_seq;
  SBA_TRY_HIP(sba::launch_joint_step(p->store, w.pl, d1, d2, c1, c2, w.sc1, w.sc2, prm, w.partials, w.grid, w.out_dev,
                                     p->publish ? p->joint_host_dev : nullptr, seq, p->stream));
  return joint_fetch(p, w, seq, sba::JOINT_STEP_COUNT, "joint step pass", row);
}

void joint_options(const sba_lm_options* opt, sba_lm_options* o) {
  if (opt) { *o = *opt; return; }
  sba::lm_default_options(o);
  o->tran_param = SBA_TRAN_SPHERE;     // the gauge: with a free translation (d, t) -> 0 minimises the cost
}

}  // namespace

extern "C" {

int sba_problem_eval_joint(sba_problem* p, const double rot[3], const double tran[3], double radius, const sba_lm_options* opt,
                           sba_joint_eq* out) {
  if (!out) return sba::set_error(SBA_ERR_INVALID_ARG, "null argument");
  int rc = joint_check(p, rot, tran);
  if (rc) return rc;
  if (!(radius > 0.0)) return sba::set_error(SBA_ERR_INVALID_ARG, "radius must be positive (+inf: no depth damping)");
  sba_lm_options o;
  joint_options(opt, &o);
  JointWork w;
  rc = joint_prepare(p, &w);
  if (rc) return rc;
  double row[sba::JOINT_ROW] = {0};
  rc = joint_reduce_pass(p, w, p->dplane[0], p->dplane[1], rot, tran, radius, true, o, row);
  if (rc) return rc;
  { const int _rc = sba::stream_wait(p->stream, "stream synchronisation", &p->poisoned); if (_rc) return _rc; }
  sba_normal_eq full, red;
  sba::expand_pack(SBA_MODE_RT, row + sba::JOINT_OUT_PACK, &full);
  sba::joint_expand_reduced(row, &red);
  std::memcpy(out->S, red.H, sizeof(out->S)); std::memcpy(out->gs, red.g, sizeof(out->gs));
  std::memcpy(out->V, full.H, sizeof(out->V)); std::memcpy(out->gc, full.g, sizeof(out->gc));
  out->cost = full.cost; out->sum_w = full.sum_w; out->n_outlier = full.n_outlier;
  out->gd_max = row[sba::JOINT_OUT_GDMAX];
  return SBA_OK;
}

int sba_problem_solve_joint(sba_problem* p, double rot[3], double tran[3], const sba_lm_options* opt, sba_lm_summary* summary,
                            double* d12_out) {
  int rc = joint_check(p, rot, tran);
  if (rc) return rc;
  sba_lm_options o;
  joint_options(opt, &o);
  sba_lm_summary local;
  sba_lm_summary* sum = summary ? summary : &local;
  std::memset(sum, 0, sizeof(*sum));
  const auto t_start = std::chrono::steady_clock::now();
  JointWork w;
  rc = joint_prepare(p, &w);
  if (rc) return rc;
  p->folded_valid = false;     // the depth planes are rewritten: the next per-match sweep refolds
  const size_t n = p->n;
  double *cur1 = p->dplane[0], *cur2 = p->dplane[1], *c1 = w.c1, *c2 = w.c2;
  double row[sba::JOINT_ROW] = {0};
  double seconds_eval = 0.0;
  sba::JointSolver solver;
  solver.start(rot, tran, o);
  while (!solver.done()) {
    const sba::JointPassRequest& rq = solver.request();
    const auto t0 = std::chrono::steady_clock::now();
    rc = rq.kind == sba::kJointReduce ? joint_reduce_pass(p, w, cur1, cur2, rq.rot, rq.tran, rq.radius, rq.first, o, row)
                                      : joint_step_pass(p, w, cur1, cur2, c1, c2, rq, o, row);
    // A pass that fails here failed in a bounded wait or a HIP call: the wait has poisoned the handle (every later entry point
    // refuses it), so leaving without draining the stream mirrors the d-only stage.  If a step was accepted before, the
    // handle's planes may hold a candidate: "depths unchanged" is promised for a non-finite START only (include/sba_hip.h).
    if (rc) return rc;
    seconds_eval += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    solver.feed(row);
    if (solver.take_candidate()) { std::swap(cur1, c1); std::swap(cur2, c2); }
  }
  // the problem's depth planes must end up holding the result
  if (cur1 != p->dplane[0]) {
    SBA_TRY_HIP(hipMemcpyAsync(p->dplane[0], cur1, w.elems * sizeof(double), hipMemcpyDeviceToDevice, p->stream));
    SBA_TRY_HIP(hipMemcpyAsync(p->dplane[1], cur2, w.elems * sizeof(double), hipMemcpyDeviceToDevice, p->stream));
  }
  if (d12_out && n > 0) {
    sba::DeviceBuffer aos(&p->poisoned);
    SBA_TRY_HIP(aos.alloc(2 * n * sizeof(double)));
    SBA_TRY_HIP(sba::launch_planes_to_d12(p->dplane[0], p->dplane[1], n, aos.as<double>(), p->stream));
    SBA_TRY_HIP(hipMemcpyAsync(d12_out, aos.ptr, 2 * n * sizeof(double), hipMemcpyDeviceToHost, p->stream));
    { const int _rc = sba::stream_wait(p->stream, "stream synchronisation", &p->poisoned); if (_rc) return _rc; }
  }
  { const int _rc = sba::stream_wait(p->stream, "stream synchronisation", &p->poisoned); if (_rc) return _rc; }
  *sum = solver.summary();
  sum->seconds_eval = seconds_eval;
  sum->seconds_total = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
  for (int a = 0; a < 3; ++a) { rot[a] = solver.rot()[a]; tran[a] = solver.tran()[a]; }
  if (solver.status() != SBA_OK)
    return sba::set_error(solver.status(), "joint solve failed: non-finite cost or 5 consecutive invalid steps");
  return SBA_OK;
}

}  // extern "C"
