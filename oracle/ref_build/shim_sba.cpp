// TEST INFRASTRUCTURE: C entry point onto the four static add_residual functions of the reference's
// spherical_bundle_adjuster.cpp (compiled unchanged next to this file).  Each one fills the stand-in ceres::Problem
// (include/ceres/ceres.h), which records the residual blocks; this file then evaluates every recorded block at the recorded
// parameter pointers and reports what was recorded.  Which depths reach the rot-only and tran-only functors (init_d[0][0] and
// init_d[1][0]), which loss each block carries and which bounds are set is therefore decided by the reference's text alone.
#include <array>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <vector>

#include "spherical_bundle_adjuster.hpp"

namespace {
inline void split(long double x, double* hi, double* lo) {
  *hi = static_cast<double>(x);
  *lo = static_cast<double>(x - static_cast<long double>(*hi));
}
}  // namespace

extern "C" {

enum { REF_JOINT = 0, REF_ROT = 1, REF_TRAN = 2, REF_DEPTH = 3 };

// which: REF_JOINT (3 residuals, blocks 2 + 3 + 3), REF_ROT (3, 3), REF_TRAN (3, 3), REF_DEPTH (5, 2).  With R residuals and P
// parameters per block:
//   res, jac            n x R, n x R x P : the functor through Jet<double> (what AutoDiffCostFunction hands Ceres)
//   res_hi/lo, jac_hi/lo                   : the same through Jet<long double>, each value as hi + lo doubles
//   meta                n x 8 int32      : loss kind (0 none, 1 Huber), number of parameter blocks, their sizes (3), and per block what
//                                          the pointer is (1 init_rot, 2 init_tran, 3 init_d[i].data() of the block's own match, 0 other)
//   loss_delta          n                : Huber delta (0 without a loss)
//   lower               n x 2            : lower bound set on init_d[i][0], init_d[i][1]; NaN where none was set
// Returns the number of lower bounds set, or -1 where T = long double residuals differ from the value part of the long-double
// Jets (they run the same operations and must not), -2 on a block the layout above cannot hold.
int ref_sba_blocks(int which, int n, const double* x1, const double* x2, const double* rot, const double* tran, const double* d12,
                   double* res, double* jac, double* res_hi, double* res_lo, double* jac_hi, double* jac_lo, int32_t* meta,
                   double* loss_delta, double* lower) {
  if (n < 2 && (which == REF_ROT || which == REF_TRAN)) return -2;   // those two read init_d[1][0] (.cpp:942, :999)
  std::vector<cv::Point3d> left(n), right(n);
  std::vector<std::array<double, 2>> init_d(n);
  for (int i = 0; i < n; ++i) {
    left[i] = cv::Point3d(x1[3 * i], x1[3 * i + 1], x1[3 * i + 2]);
    right[i] = cv::Point3d(x2[3 * i], x2[3 * i + 1], x2[3 * i + 2]);
    init_d[i] = {{d12[2 * i], d12[2 * i + 1]}};
  }
  double init_rot[3] = {rot[0], rot[1], rot[2]}, init_tran[3] = {tran[0], tran[1], tran[2]};
  ceres::Problem problem;
  switch (which) {
    case REF_JOINT: ba_spherical_costfunctor::add_residual(problem, left, right, init_rot, init_tran, init_d, n); break;
    case REF_ROT: ba_spherical_costfunctor_rot_only::add_residual(problem, left, right, init_rot, init_tran, init_d, n); break;
    case REF_TRAN: ba_spherical_costfunctor_tran_only::add_residual(problem, left, right, init_rot, init_tran, init_d, n); break;
    default: ba_spherical_costfunctor_d_only::add_residual(problem, left, right, init_rot, init_tran, init_d, n); break;
  }
  if (static_cast<int>(problem.blocks.size()) != n) return -2;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (int i = 0; i < 2 * n; ++i) lower[i] = nan;
  for (int i = 0; i < n; ++i) {
    const ceres::Problem::Block& b = problem.blocks[i];
    const int R = b.cost->standin_num_residuals();
    const std::vector<int> sizes = b.cost->standin_block_sizes();
    int P = 0;
    for (int s : sizes) P += s;
    if (sizes.size() != b.params.size() || sizes.size() > 3 || R > 5 || P > 8) return -2;
    int32_t* m = meta + 8 * i;
    for (int k = 0; k < 8; ++k) m[k] = 0;
    m[0] = b.loss ? 1 : 0;
    m[1] = static_cast<int32_t>(sizes.size());
    for (size_t k = 0; k < sizes.size(); ++k) {
      m[2 + k] = sizes[k];
      m[5 + k] = b.params[k] == init_rot ? 1 : b.params[k] == init_tran ? 2 : b.params[k] == init_d[i].data() ? 3 : 0;
    }
    loss_delta[i] = b.loss ? b.loss->standin_delta() : 0.0;
    long double r_ld[5], j_ld[40], r_plain[5];
    b.cost->standin_evaluate(b.params.data(), res + static_cast<size_t>(i) * R, jac + static_cast<size_t>(i) * R * P);
    b.cost->standin_evaluate_ld(b.params.data(), r_ld, j_ld);
    b.cost->standin_residuals_ld(b.params.data(), r_plain);
    for (int k = 0; k < R; ++k) {
      if (!(r_plain[k] == r_ld[k])) return -1;
      split(r_ld[k], res_hi + static_cast<size_t>(i) * R + k, res_lo + static_cast<size_t>(i) * R + k);
    }
    for (int k = 0; k < R * P; ++k) split(j_ld[k], jac_hi + static_cast<size_t>(i) * R * P + k, jac_lo + static_cast<size_t>(i) * R * P + k);
  }
  int set = 0;
  for (const ceres::Problem::LowerBound& lb : problem.lower)
    for (int i = 0; i < n; ++i)
      if (lb.values == init_d[i].data() && lb.index >= 0 && lb.index < 2) { lower[2 * i + lb.index] = lb.bound; ++set; }
  return set;
}

}  // extern "C"
