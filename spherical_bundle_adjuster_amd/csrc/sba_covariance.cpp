// Entry point of the joint solve's covariance (include/sba_hip.h): the pose's 6 x 6 block and every match's 2 x 2 depth
// block at a point (rot, tran, the handle's depths).  Kernels: sba_covariance.hip; algebra and host finish: sba_covariance.hpp.
// cov_first_pass -- checks, reduce pass, host finish -- also opens the entry points of sba_structure.cpp.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "sba_covariance.hpp"
#include "sba_lm.hpp"
#include "sba_problem.hpp"
#include "sba_rotation.hpp"

namespace sba {
namespace shim {

int cov_first_pass(sba_problem* p, const double rot[3], const double tran[3], const sba_lm_options* opt, double min_sin2_parallax,
                   size_t front_elems, CovPass* cp) {
  if (!p || !rot || !tran || !cp) return sba::set_error(SBA_ERR_INVALID_ARG, "null argument");
  if (!(min_sin2_parallax >= 0.0)) return sba::set_error(SBA_ERR_INVALID_ARG, "min_sin2_parallax must be >= 0");
  // the refusals of sba_problem_solve_joint
  SBA_REFUSE_POISONED(p);
  if (!p->uploaded) return sba::set_error(SBA_ERR_NOT_UPLOADED, "no correspondences uploaded");
  if (sba::shim::is_collective(p) || p->shard_count != 1)
    return sba::set_error(SBA_ERR_UNSUPPORTED, "the joint covariance runs on one unsharded problem, as the joint solve does");
  if (!p->has_d12 && p->n > 0)
    return sba::set_error(SBA_ERR_UNSUPPORTED, "the joint covariance needs per-match depths (upload d12 or call sba_problem_set_depths)");
  for (int i = 0; i < 3; ++i)
    if (!std::isfinite(rot[i]) || !std::isfinite(tran[i])) return sba::set_error(SBA_ERR_NUMERIC, "non-finite rot/tran");
  sba_lm_options o;
  if (opt) {
    o = *opt;
  } else {
    sba::lm_default_options(&o);
    o.tran_param = SBA_TRAN_SPHERE;     // the gauge of the joint solve's defaults
  }

  SBA_TRY_HIP(hipSetDevice(p->device));
  const size_t n = p->n, npairs = (n + 1) / 2;
  // Rows, results and the per-match pass's own front live in the handle's d-only scratch (no stage overlaps another, and the
  // d-only stage and the joint solve re-zero their planes on entry): [front_elems] front, [COV_ROW] results, [grid][COV_ROW] rows.
  const size_t out_elems = (front_elems + 15) / 16 * 16;
  const size_t max_grid_rows = static_cast<size_t>(p->num_cus) * 16 + 1;
  const size_t need = (out_elems + (max_grid_rows + 1) * sba::COV_ROW) * sizeof(double);
  if (p->depth_scratch_bytes < need) {
    if (p->depth_scratch) SBA_TRY_HIP(hipFree(p->depth_scratch));
    p->depth_scratch = nullptr; p->depth_scratch_bytes = 0;
    SBA_TRY_HIP(hipMalloc(&p->depth_scratch, need));
    p->depth_scratch_bytes = need;
  }
  double* dd_dev = static_cast<double*>(p->depth_scratch);
  double *out_dev = dd_dev + out_elems, *partials = out_dev + sba::COV_ROW;
  int& occ = p->cov_occ[p->store];
  if (occ == 0) {
    SBA_TRY_HIP(sba::cov_blocks_per_cu(p->store, &occ));
    occ = std::max(1, occ);
  }
  const int grid = sba::joint_grid(npairs, p->num_cus, occ);

  sba::Planes& pl = cp->pl;
  for (int k = 0; k < 3; ++k) { pl.x1[k] = p->coord[k]; pl.x2[k] = p->coord[3 + k]; }
  pl.d1 = p->dplane[0]; pl.d2 = p->dplane[1];
  sba::JointParams& prm = cp->prm;
  prm = sba::JointParams{};
  sba::fill_sweep_params(n, SBA_DEPTH_PER_MATCH, rot, tran, 1.0, 1.0, o.huber_delta, &prm.cur, false);
  prm.cand = prm.cur;
  double B[9];
  sba::factored_frame(rot, B, prm.J);
  prm.small_angle = !(rot[0] * rot[0] + rot[1] * rot[1] + rot[2] * rot[2] > DBL_EPSILON) ? 1 : 0;
  prm.inv_radius = 0.0;               // radius = inf: the undamped system
  prm.min_diagonal = o.min_lm_diagonal; prm.max_diagonal = o.max_lm_diagonal;
  prm.first = 1; prm.jacobi_scaling = o.jacobi_scaling ? 1 : 0;

  SBA_TRY_HIP(sba::launch_cov_reduce(p->store, pl, p->dplane[0], p->dplane[1], prm, min_sin2_parallax, partials, grid, out_dev, p->stream));
  double row[sba::COV_ROW] = {0};
  SBA_TRY_HIP(hipMemcpyAsync(row, out_dev, sba::COV_OUT_COUNT * sizeof(double), hipMemcpyDeviceToHost, p->stream));
  { const int rc = sba::stream_wait(p->stream, "covariance reduce pass", &p->poisoned); if (rc) return rc; }

  sba_joint_cov res;
  std::memset(&res, 0, sizeof(res));
  const long long n_used = static_cast<long long>(row[sba::COV_OUT_NUSED]);
  if (!sba::cov_finish(row + sba::COV_OUT_S, o.tran_param, tran, n_used, res.cov, &res.dim))
    return sba::set_error(SBA_ERR_NUMERIC, "joint covariance: the reduced camera system of the %lld used matches is not finite or "
                                           "rank-deficient in the gauge's tangent space", n_used);
  res.cost = row[sba::COV_OUT_COST]; res.sum_w = row[sba::COV_OUT_SW];
  res.n_used = n_used; res.n_degenerate = static_cast<long long>(row[sba::COV_OUT_NDEG]);
  res.dof = static_cast<int>(n_used - res.dim);
  cp->res = res;
  cp->grid = grid;
  cp->front = dd_dev;
  return SBA_OK;
}

}  // namespace shim
}  // namespace sba

extern "C" {

int sba_problem_covariance_joint(sba_problem* p, const double rot[3], const double tran[3], const sba_lm_options* opt,
                                 double min_sin2_parallax, sba_joint_cov* out, double* depth_cov) {
  if (!out) return sba::set_error(SBA_ERR_INVALID_ARG, "null argument");
  sba::shim::CovPass cp;
  const size_t n = p ? p->n : 0;
  { const int rc = sba::shim::cov_first_pass(p, rot, tran, opt, min_sin2_parallax, 6 * ((n + 1) / 2), &cp); if (rc) return rc; }
  if (depth_cov && n > 0) {
    SBA_TRY_HIP(sba::launch_cov_depth(p->store, cp.pl, p->dplane[0], p->dplane[1], cp.prm, min_sin2_parallax, cp.res.cov, cp.front, cp.grid, p->stream));
    SBA_TRY_HIP(hipMemcpyAsync(depth_cov, cp.front, 3 * n * sizeof(double), hipMemcpyDeviceToHost, p->stream));
    { const int rc = sba::stream_wait(p->stream, "covariance depth pass", &p->poisoned); if (rc) return rc; }
  }
  *out = cp.res;
  return SBA_OK;
}

}  // extern "C"
