// Host step logic of the JOINT solve -- depths, rotation and translation free together (the reference's
// ba_spherical_costfunctor, spherical_bundle_adjuster.cpp:843-889) -- as a resumable state machine.  No HIP in here: the
// same source drives the device passes in sba_joint.cpp and is exercised on the CPU by tests/test_joint_solver_cpu.py
// with numpy-emulated passes.
//
// Parameter vector [d | camera]: the 2n per-match depths and the camera (rot, tran) through detail::Param (6 local
// parameters with SBA_TRAN_FREE, 5 with SBA_TRAN_SPHERE).  The depth blocks are private to a match, so one LM iteration
// is two streaming passes with the <= 6-dim reduced camera system (the Schur complement) solved in between:
//
//   request().kind == kJointReduce : joint_reduce_kernel at (rot, tran, d) with the depth damping of `radius`
//        -> feed(row): reduced system S, gs; unreduced camera block (SBA_PACK_* layout), cost, max |g_d|
//      host: Param projection, Jacobi scaling and damping of the camera columns, Cholesky -> camera step
//   request().kind == kJointStep   : joint_step_kernel given the ambient camera step delta_c and the candidate camera
//        -> feed(row): candidate cost, model cost change, |delta d|^2, |d|^2
//      host: parameter / function tolerance, step quality, accept (take_candidate() -> the caller's candidate planes
//      become its depths) or reject
//
// The schedule is the one of sba_lm.hpp / sba_depth_solver.hpp (Ceres' TrustRegionMinimizer + LevenbergMarquardtStrategy
// defaults): Jacobi scaling fixed at the first evaluation, D^2 = clamp(diag(H_s), min, max) / radius kept across rejected
// steps, the same order of the termination checks.  No line search: the joint problem has no bounds.
// summary().num_evaluations counts device passes of either kind.
#pragma once
#include <algorithm>
#include <cmath>

#include "../../include/sba_hip.h"
#include "sba_lm.hpp"

#if defined(__clang__)
#pragma STDC FP_CONTRACT OFF
#endif

// On the device the solver lives in LDS and is fed from inside a kernel (sba_batch_joint.hip): feed() is inlined into every
// kernel that calls it, a call would put a stack frame into scratch memory.  The host build is not affected.
#if defined(__HIP_DEVICE_COMPILE__)
#define SBA_JOINT_FEED_INLINE __attribute__((always_inline))
#else
#define SBA_JOINT_FEED_INLINE
#endif

namespace sba {

// Row of a reduce pass: [0..23] the unreduced camera block in SBA_PACK_* layout (sum w F^T F, sum w F^T e, cost, outliers),
// [24..44] the upper triangle of S = sum (w F^T F - W^T U^-1 W) over [rot | tran], row by row, [45..50] the reduced
// gradient sum (w F^T e - W^T U^-1 g_d), [51] max |g_d| (unscaled depth gradient, a maximum).
// Row of a step pass: four sums.
enum {
  JOINT_OUT_PACK = 0,
  JOINT_OUT_S = 24,
  JOINT_OUT_GS = 45,
  JOINT_OUT_GDMAX = 51,
  JOINT_OUT_COUNT = 52,
  JOINT_STEP_CAND_COST = 0,
  JOINT_STEP_MODEL = 1,     // -sum w (J delta)^T (e + J delta / 2) over the full step
  JOINT_STEP_DSTEP2 = 2,    // |delta d|^2
  JOINT_STEP_D2 = 3,        // |d|^2
  JOINT_STEP_COUNT = 4,
  JOINT_ROW = 64            // doubles per block-partial row (512 B: whole 128-byte lines)
};
enum { kJointReduce = 0, kJointStep = 1 };

struct JointPassRequest {
  int kind = kJointReduce;
  bool first = true;          // first reduce pass of the solve: compute and store the depth Jacobi scaling
  double radius = 0.0;
  double rot[3] = {0, 0, 0}, tran[3] = {0, 0, 0};            // the current point (both kinds)
  double delta_c[6] = {0, 0, 0, 0, 0, 0};                    // kJointStep: ambient camera step [rot | tran]
  double rot_cand[3] = {0, 0, 0}, tran_cand[3] = {0, 0, 0};  // kJointStep: Plus(camera, step)
};

// Upper triangle (row by row) + gradient of a reduce row -> sba_normal_eq over [rot | tran].
SBA_HD inline void joint_expand_reduced(const double* row, sba_normal_eq* ne) {
  *ne = sba_normal_eq{};
  int k = JOINT_OUT_S;
  for (int a = 0; a < 6; ++a)
    for (int b = a; b < 6; ++b) {
      ne->H[6 * a + b] = row[k];
      ne->H[6 * b + a] = row[k];
      ++k;
    }
  for (int a = 0; a < 6; ++a) ne->g[a] = row[JOINT_OUT_GS + a];
  ne->cost = row[SBA_PACK_COST];
  ne->sum_w = row[SBA_PACK_SW];
  ne->n_outlier = row[SBA_PACK_NOUT];
}

class JointSolver {
 public:
  SBA_HD void start(const double rot0[3], const double tran0[3], const sba_lm_options& o) {
    o_ = o;
    for (int a = 0; a < 3; ++a) { rot_[a] = rot0[a]; tran_[a] = tran0[a]; }
    sum_ = sba_lm_summary{};
    sum_.termination = SBA_TERM_FAILURE;
    radius_ = o.initial_trust_region_radius;
    nu_ = 2.0;
    reuse_ = false;
    first_ = true;
    invalid_ = 0;
    it_ = 0;
    done_ = false;
    swap_ = false;
    rc_ = SBA_OK;
    cost_ = gmax_ = 0.0;
    request_reduce();
  }
  SBA_HD bool done() const { return done_; }
  SBA_HD int status() const { return rc_; }                       // SBA_OK or SBA_ERR_NUMERIC
  SBA_HD const JointPassRequest& request() const { return rq_; }
  SBA_HD const sba_lm_summary& summary() const { return sum_; }
  SBA_HD const double* rot() const { return rot_; }               // current accepted camera (the result once done)
  SBA_HD const double* tran() const { return tran_; }
  SBA_HD bool take_candidate() { const bool s = swap_; swap_ = false; return s; }

  // `row`: the reductions of the requested pass (JOINT_OUT_* / JOINT_STEP_* slots).
  SBA_HD SBA_JOINT_FEED_INLINE void feed(const double* row) {
    if (done_) return;
    sum_.num_evaluations++;
    if (rq_.kind == kJointReduce) feed_reduce(row); else feed_step(row);
  }

 private:
  SBA_HD void request_reduce() {
    rq_.kind = kJointReduce;
    rq_.first = first_;
    rq_.radius = radius_;
    for (int a = 0; a < 3; ++a) { rq_.rot[a] = rot_[a]; rq_.tran[a] = tran_[a]; }
  }
  SBA_HD void finish(int term, int rc = SBA_OK) {
    sum_.termination = term;
    sum_.final_cost = cost_;
    sum_.final_gradient_max_norm = gmax_;
    sum_.final_radius = radius_;
    rc_ = rc;
    done_ = true;
  }
  SBA_HD void invalid_step() {
    if (++invalid_ >= 5) { finish(SBA_TERM_FAILURE, SBA_ERR_NUMERIC); return; }
    radius_ /= nu_; nu_ *= 2.0; reuse_ = true;
    request_reduce();
  }

  SBA_HD void feed_reduce(const double* row) {
    using namespace detail;
    const bool first = first_;
    first_ = false;
    cost_ = row[SBA_PACK_COST];
    if (first) {
      sum_.initial_cost = cost_;
      if (!std::isfinite(cost_)) { finish(SBA_TERM_FAILURE, SBA_ERR_NUMERIC); return; }
    }
    // unreduced camera block: Jacobi scaling, LM diagonal and the gradient norm are those of the FULL Jacobian's columns
    sba_normal_eq full, red;
    expand_pack(SBA_MODE_RT, row + JOINT_OUT_PACK, &full);
    joint_expand_reduced(row, &red);
    par_.build(SBA_MODE_RT, o_.tran_param, tran_);
    const int m = par_.m;
    double Vf[kDim * kDim], gcf[kDim], Sf[kDim * kDim], gsf[kDim];
    par_.project(full, Vf, gcf);
    par_.project(red, Sf, gsf);
    if (first) {
      SBA_UNROLL
      for (int i = 0; i < kDim; ++i)
        if (i < m) scale_[i] = o_.jacobi_scaling ? 1.0 / (1.0 + std::sqrt(std::max(Vf[i * kDim + i], 0.0))) : 1.0;
    }
    gmax_ = row[JOINT_OUT_GDMAX];
    SBA_UNROLL
    for (int i = 0; i < kDim; ++i)
      if (i < m) gmax_ = std::max(gmax_, std::fabs(gcf[i]));
    // Ceres' end-of-iteration checks, in its order
    if (it_ >= o_.max_num_iterations) { finish(SBA_TERM_NO_CONVERGENCE); return; }
    if (gmax_ <= o_.gradient_tolerance) { finish(SBA_TERM_CONVERGENCE_GRADIENT); return; }
    if (radius_ < o_.min_trust_region_radius) { finish(SBA_TERM_MIN_RADIUS); return; }
    sum_.num_iterations = ++it_;
    if (!reuse_) {
      SBA_UNROLL
      for (int i = 0; i < kDim; ++i)
        if (i < m) diag_[i] = std::min(std::max(scale_[i] * Vf[i * kDim + i] * scale_[i], o_.min_lm_diagonal), o_.max_lm_diagonal);
    }
    double A[kDim * kDim], rhs[kDim], y[kDim];
    SBA_UNROLL
    for (int i = 0; i < kDim; ++i) {
      SBA_UNROLL
      for (int j = 0; j < kDim; ++j)
        if (i < m && j < m) A[i * kDim + j] = scale_[i] * Sf[i * kDim + j] * scale_[j];
    }
    SBA_UNROLL
    for (int i = 0; i < kDim; ++i)
      if (i < m) { A[i * kDim + i] += diag_[i] / radius_; rhs[i] = -(scale_[i] * gsf[i]); }
    if (!cholesky_solve(m, A, rhs, y)) { invalid_step(); return; }
    double delta[kDim];
    SBA_UNROLL
    for (int i = 0; i < kDim; ++i) delta[i] = i < m ? scale_[i] * y[i] : 0.0;
    // ambient camera step P delta (what the depth back-substitution and the model use) and the candidate Plus(camera, delta)
    SBA_UNROLL
    for (int i = 0; i < kDim; ++i) {
      double s = 0;
      SBA_UNROLL
      for (int j = 0; j < kDim; ++j)
        if (j < m) s += par_.P[i * kDim + j] * delta[j];
      rq_.delta_c[i] = s;
    }
    par_.plus(rot_, tran_, delta, rq_.rot_cand, rq_.tran_cand);
    rq_.kind = kJointStep;
    rq_.first = false;
    rq_.radius = radius_;
    for (int a = 0; a < 3; ++a) { rq_.rot[a] = rot_[a]; rq_.tran[a] = tran_[a]; }
  }

  SBA_HD void feed_step(const double* row) {
    const double model = row[JOINT_STEP_MODEL], cand_cost = row[JOINT_STEP_CAND_COST];
    if (!(model > 0.0)) { invalid_step(); return; }
    invalid_ = 0;
    double step2 = row[JOINT_STEP_DSTEP2], x2 = row[JOINT_STEP_D2];
    for (int a = 0; a < 3; ++a) {
      step2 += (rq_.rot_cand[a] - rot_[a]) * (rq_.rot_cand[a] - rot_[a]) + (rq_.tran_cand[a] - tran_[a]) * (rq_.tran_cand[a] - tran_[a]);
      x2 += rot_[a] * rot_[a] + tran_[a] * tran_[a];
    }
    if (std::sqrt(step2) <= o_.parameter_tolerance * (std::sqrt(x2) + o_.parameter_tolerance)) {
      finish(SBA_TERM_CONVERGENCE_PARAMETER);
      return;
    }
    const double change = cost_ - cand_cost;
    if (std::isfinite(cand_cost) && std::fabs(change) <= o_.function_tolerance * cost_) { finish(SBA_TERM_CONVERGENCE_FUNCTION); return; }
    const double quality = std::isfinite(cand_cost) ? change / model : -1.0;
    if (quality > o_.min_relative_decrease) {
      swap_ = true;                              // the candidate planes become the current depths
      for (int a = 0; a < 3; ++a) { rot_[a] = rq_.rot_cand[a]; tran_[a] = rq_.tran_cand[a]; }
      sum_.num_successful_steps++;
      const double q = 2.0 * quality - 1.0;
      radius_ = std::min(o_.max_trust_region_radius, radius_ / std::max(1.0 / 3.0, 1.0 - q * q * q));
      nu_ = 2.0; reuse_ = false;
    } else {
      radius_ /= nu_; nu_ *= 2.0; reuse_ = true;
    }
    request_reduce();
  }

  sba_lm_options o_{};
  sba_lm_summary sum_{};
  JointPassRequest rq_;
  detail::Param par_;
  double rot_[3] = {0, 0, 0}, tran_[3] = {0, 0, 0};
  double scale_[6] = {0}, diag_[6] = {0};
  double radius_ = 0, nu_ = 2, cost_ = 0, gmax_ = 0;
  bool reuse_ = false, first_ = true, done_ = false, swap_ = false;
  int invalid_ = 0, it_ = 0, rc_ = SBA_OK;
};

}  // namespace sba

#if defined(__clang__)
#pragma STDC FP_CONTRACT DEFAULT
#endif
