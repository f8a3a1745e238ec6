// What the entry points of the spherical resection share (sba_resection.cpp, sba_resection_consensus.cpp): the refusals of a
// handle, the work memory and grids of a pass, the wait for a published row and the reduce pass.  Included by those two
// translation units only; every function is file-local in each.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "sba_problem.hpp"
#include "sba_resection.hpp"

namespace {

struct ResectWork {
  sba::Planes pl;
  double *out_dev = nullptr, *partials = nullptr;
  int grid = 0, moments_grid = 0, depths_grid = 0;
};

// The refusals of the joint family (sba_joint.cpp: joint_check), before any device call.
int resect_check_handle(sba_problem* p) {
  SBA_REFUSE_POISONED(p);
  if (!p->uploaded) return sba::set_error(SBA_ERR_NOT_UPLOADED, "no correspondences uploaded");
  if (sba::shim::is_collective(p) || p->shard_count != 1)
    return sba::set_error(SBA_ERR_UNSUPPORTED, "the resection runs on one unsharded problem: its reduction row (%d doubles) is wider "
                                               "than the %d-double exchange of the transports", int(SBA_RESECT_COUNT), int(SBA_PACK_SIZE));
  if (!p->has_d12 && p->n > 0)
    return sba::set_error(SBA_ERR_UNSUPPORTED, "the resection needs per-match depths: the landmarks are d1 x1 (upload d12 or call "
                                               "sba_problem_set_depths)");
  return SBA_OK;
}

// The mapped host row (shared with the joint solve), the block rows in the handle's d-only scratch, the grids.
int resect_prepare(sba_problem* p, bool loss, ResectWork* w) {
  SBA_TRY_HIP(hipSetDevice(p->device));
  if (!p->joint_host) {
    SBA_TRY_HIP(hipHostMalloc(reinterpret_cast<void**>(&p->joint_host), (sba::JOINT_ROW + 8) * sizeof(double),
                              hipHostMallocMapped | hipHostMallocCoherent));
    std::memset(p->joint_host, 0, (sba::JOINT_ROW + 8) * sizeof(double));
    SBA_TRY_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&p->joint_host_dev), p->joint_host, 0));
  }
  const size_t max_rows = static_cast<size_t>(p->num_cus) * 2 + 1;
  const size_t need = (max_rows + 1) * sba::JOINT_ROW * sizeof(double);
  if (p->depth_scratch_bytes < need) {
    if (p->depth_scratch) SBA_TRY_HIP(hipFree(p->depth_scratch));
    p->depth_scratch = nullptr; p->depth_scratch_bytes = 0;
    SBA_TRY_HIP(hipMalloc(&p->depth_scratch, need));
    p->depth_scratch_bytes = need;
  }
  w->out_dev = static_cast<double*>(p->depth_scratch);
  w->partials = w->out_dev + sba::JOINT_ROW;
  int& occ = p->resect_occ[p->store][loss ? 1 : 0];
  if (occ == 0) {
    SBA_TRY_HIP(sba::resect_blocks_per_cu(p->store, loss, &occ));
    occ = std::max(1, occ);
  }
  const size_t ppt = static_cast<size_t>(sba::points_per_lane(p->store));
  const size_t blocks = ((p->n + ppt - 1) / ppt + 255) / 256;
  int cap = 1 << 30;     // SBA_RESECT_GRID (tests): at most this many blocks, so that small problems take several grid-stride steps
  if (const char* env = std::getenv("SBA_RESECT_GRID")) { const int v = std::atoi(env); if (v >= 1) cap = v; }
  w->grid = static_cast<int>(std::min<size_t>({blocks, static_cast<size_t>(p->num_cus) * std::min(occ, 2), static_cast<size_t>(cap)}));
  w->moments_grid = static_cast<int>(std::min<size_t>({blocks, static_cast<size_t>(p->num_cus), static_cast<size_t>(cap)}));
  w->depths_grid = static_cast<int>(std::min<size_t>({blocks, static_cast<size_t>(p->num_cus) * 8, static_cast<size_t>(cap)}));
  for (int k = 0; k < 3; ++k) { w->pl.x1[k] = p->coord[k]; w->pl.x2[k] = p->coord[3 + k]; }
  w->pl.d1 = p->dplane[0]; w->pl.d2 = nullptr;     // never read
  return SBA_OK;
}

// Wait for the row of the pass enqueued last and copy `count` results out.
int resect_fetch(sba_problem* p, const ResectWork& w, unsigned long long seq, int count, const char* what, double* row) {
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

int resect_reduce_pass(sba_problem* p, const ResectWork& w, const double rot[3], const double tran[3], double huber_delta, double* row) {
  sba::ResectParams prm;
  sba::fill_resect_params(p->n, rot, tran, huber_delta, &prm);
  const unsigned long long seq = ++p->joint_seq;
  SBA_TRY_HIP(sba::launch_resect_reduce(p->store, w.pl, prm, w.partials, w.grid, w.out_dev, p->publish ? p->joint_host_dev : nullptr,
                                        seq, p->stream));
  return resect_fetch(p, w, seq, SBA_RESECT_COUNT, "resection reduce pass", row);
}

}  // namespace
