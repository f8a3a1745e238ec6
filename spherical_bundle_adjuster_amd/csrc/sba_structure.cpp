// Entry points of the triangulated structure (include/sba_hip.h): one 3-D point per match with its 3 x 3 covariance and a
// dimensionless uncertainty score at a point (rot, tran, the handle's depths), and the cut driven by that score.
// Every call: the covariance's reduce pass and host finish (sba_covariance.cpp: cov_first_pass), then structure_kernel
// (sba_structure.hip; algebra: sba_structure.hpp).  The cut hands the score plane to the selection and compaction of
// sba_quantile.cpp, unchanged.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "sba_problem.hpp"
#include "sba_quantile.hpp"

namespace {

// doubles the pass parameters take at the front of the scratch (whole 256-byte lines: what follows stays aligned)
constexpr size_t kParamElems = (sizeof(sba::StructureParams) / sizeof(double) + 31) / 32 * 32;

// The pass's own grid: joint_grid at structure_kernel's occupancy (its registers allow fewer resident blocks than the reduce
// pass has).  SBA_STRUCTURE_GRID (tests): at most this many blocks -- the results do not depend on the grid.
int structure_grid(sba_problem* p, int* grid) {
  int& occ = p->structure_occ[p->store];
  if (occ == 0) {
    SBA_TRY_HIP(sba::structure_blocks_per_cu(p->store, &occ));
    occ = std::max(1, occ);
  }
  *grid = sba::joint_grid((p->n + 1) / 2, p->num_cus, occ);
  if (const char* env = std::getenv("SBA_STRUCTURE_GRID")) { const int v = std::atoi(env); if (v >= 1) *grid = std::min(*grid, v); }
  return SBA_OK;
}

bool aligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15u) == 0; }

// The reduce pass and the finish, then the pass parameters on their way to the device.  out_elems: doubles the caller wants
// behind them (*area).  *hp stays valid until the caller has waited for the stream.
int first_pass(sba_problem* p, const double rot[3], const double tran[3], const sba_lm_options* opt, double min_sin2_parallax,
               size_t out_elems, sba::shim::CovPass* cp, sba::StructureParams* hp, double** area) {
  const int rc = sba::shim::cov_first_pass(p, rot, tran, opt, min_sin2_parallax, kParamElems + out_elems, cp);
  if (rc) return rc;
  std::memset(hp, 0, sizeof(*hp));
  hp->prm = cp->prm;
  std::memcpy(hp->sigma_c, cp->res.cov, sizeof(hp->sigma_c));
  hp->min_sin2 = min_sin2_parallax;
  SBA_TRY_HIP(hipMemcpyAsync(cp->front, hp, sizeof(*hp), hipMemcpyHostToDevice, p->stream));
  *area = cp->front + kParamElems;
  return SBA_OK;
}

int launch_pass(sba_problem* p, const sba::shim::CovPass& cp, double* xyz, double* cov, double* score) {
  int grid = 0;
  const int rc = structure_grid(p, &grid);
  if (rc) return rc;
  SBA_TRY_HIP(sba::launch_structure(p->store, cp.pl, p->dplane[0], p->dplane[1], reinterpret_cast<const sba::StructureParams*>(cp.front),
                                    xyz, cov, score, grid, p->stream));
  return SBA_OK;
}

}  // namespace

extern "C" {

int sba_problem_structure_joint(sba_problem* p, const double rot[3], const double tran[3], const sba_lm_options* opt,
                                double min_sin2_parallax, sba_joint_cov* out, double* xyz, double* xyz_cov, double* score) {
  if (!out) return sba::set_error(SBA_ERR_INVALID_ARG, "null argument");
  const size_t n = p ? p->n : 0, npairs = (n + 1) / 2;
  sba::shim::CovPass cp;
  sba::StructureParams hp;
  double* area = nullptr;
  int rc = first_pass(p, rot, tran, opt, min_sin2_parallax, 20 * npairs, &cp, &hp, &area);
  if (rc) return rc;
  double *xyz_dev = area, *cov_dev = area + 6 * npairs, *score_dev = area + 18 * npairs;
  rc = launch_pass(p, cp, xyz ? xyz_dev : nullptr, xyz_cov ? cov_dev : nullptr, score ? score_dev : nullptr);
  if (rc) return rc;
  if (xyz) SBA_TRY_HIP(hipMemcpyAsync(xyz, xyz_dev, 3 * n * sizeof(double), hipMemcpyDeviceToHost, p->stream));
  if (xyz_cov) SBA_TRY_HIP(hipMemcpyAsync(xyz_cov, cov_dev, 6 * n * sizeof(double), hipMemcpyDeviceToHost, p->stream));
  if (score) SBA_TRY_HIP(hipMemcpyAsync(score, score_dev, n * sizeof(double), hipMemcpyDeviceToHost, p->stream));
  rc = sba::stream_wait(p->stream, "structure pass", &p->poisoned);
  if (rc) return rc;
  *out = cp.res;
  return SBA_OK;
}

int sba_problem_structure_joint_device(sba_problem* p, const double rot[3], const double tran[3], const sba_lm_options* opt,
                                       double min_sin2_parallax, sba_joint_cov* out, double* xyz, double* xyz_cov, double* score) {
  if (!out) return sba::set_error(SBA_ERR_INVALID_ARG, "null argument");
  if (!aligned16(xyz) || !aligned16(xyz_cov) || !aligned16(score))
    return sba::set_error(SBA_ERR_INVALID_ARG, "the device destinations must be 16-byte aligned");
  sba::shim::CovPass cp;
  sba::StructureParams hp;
  double* area = nullptr;
  int rc = first_pass(p, rot, tran, opt, min_sin2_parallax, 0, &cp, &hp, &area);
  if (rc) return rc;
  rc = launch_pass(p, cp, xyz, xyz_cov, score);
  if (rc) return rc;
  rc = sba::stream_wait(p->stream, "structure pass", &p->poisoned);
  if (rc) return rc;
  *out = cp.res;
  return SBA_OK;
}

int sba_problem_structure_order_stats(sba_problem* p, const double rot[3], const double tran[3], const sba_lm_options* opt,
                                      double min_sin2_parallax, const size_t* ranks, int num_ranks, double* values) {
  if (!ranks || !values) return sba::set_error(SBA_ERR_INVALID_ARG, "ranks/values must not be null");
  if (num_ranks < 1 || num_ranks > sba::kSelectMaxRanks)
    return sba::set_error(SBA_ERR_INVALID_ARG, "num_ranks %d outside 1...%d", num_ranks, sba::kSelectMaxRanks);
  sba::shim::CovPass cp;
  sba::StructureParams hp;
  double* area = nullptr;
  int rc = first_pass(p, rot, tran, opt, min_sin2_parallax, 0, &cp, &hp, &area);
  if (rc) return rc;
  for (int j = 0; j < num_ranks; ++j)
    if (ranks[j] >= p->n) return sba::set_error(SBA_ERR_INVALID_ARG, "rank %zu is not below the %zu matches", ranks[j], p->n);
  sba::SelectScratch s;
  double* plane = nullptr;
  rc = sba::shim::select_plane(p, num_ranks, &s, &plane);
  if (rc) return rc;
  rc = launch_pass(p, cp, nullptr, nullptr, plane);
  if (rc) return rc;
  unsigned long long host_offsets[2];
  rc = sba::shim::select_enqueue(p, s, ranks, num_ranks, nullptr, host_offsets);
  if (rc) return rc;
  return sba::shim::select_values(p, s, num_ranks, values);
}

int sba_problem_structure_keep_below(sba_problem* p, const double rot[3], const double tran[3], const sba_lm_options* opt,
                                     double min_sin2_parallax, size_t rank, double scale, double* threshold, size_t* n_kept,
                                     long long* kept_index) {
  if (!threshold || !n_kept) return sba::set_error(SBA_ERR_INVALID_ARG, "threshold/n_kept must not be null");
  if (!std::isfinite(scale) || scale < 0.0) return sba::set_error(SBA_ERR_INVALID_ARG, "scale must be finite and >= 0");
  sba::shim::CovPass cp;
  sba::StructureParams hp;
  double* area = nullptr;
  int rc = first_pass(p, rot, tran, opt, min_sin2_parallax, 0, &cp, &hp, &area);
  if (rc) return rc;
  if (rank >= p->n) return sba::set_error(SBA_ERR_INVALID_ARG, "rank %zu is not below the %zu matches", rank, p->n);
  sba::SelectScratch s;
  double* plane = nullptr;
  rc = sba::shim::select_plane(p, 1, &s, &plane);
  if (rc) return rc;
  rc = launch_pass(p, cp, nullptr, nullptr, plane);
  if (rc) return rc;
  unsigned long long host_offsets[2];
  rc = sba::shim::select_enqueue(p, s, &rank, 1, &scale, host_offsets);
  if (rc) return rc;
  return sba::shim::select_keep(p, s, threshold, n_kept, kept_index);
}

}  // extern "C"
