// Entry points that select among the per-match squared residual norms (include/sba_hip.h): exact order statistics of a
// problem's or of every pair's s = e.e, and the keep-rule s <= scale * s_(rank) followed by the compaction.
// Kernels: sba_quantile.hip (selection, threshold), sba_select.hip (the residual kernels that write s, unchanged).
#include <algorithm>
#include <cmath>
#include <limits>

#include "sba_batch.hpp"
#include "sba_problem.hpp"
#include "sba_quantile.hpp"

static_assert(sizeof(size_t) == sizeof(unsigned long long), "ranks travel as 64-bit words");

using sba::SelectScratch;

namespace {

size_t up256(size_t v) { return (v + 255) & ~size_t(255); }

SelectScratch carve(char* base, size_t pairs, size_t num_ranks, size_t sq_elems) {
  SelectScratch s;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* at = base + off;
    off += up256(bytes);
    return at;
  };
  s.n_inlier = reinterpret_cast<unsigned long long*>(take(pairs * sizeof(unsigned long long)));
  s.kept = reinterpret_cast<unsigned long long*>(take(pairs * sizeof(unsigned long long)));
  s.offsets = reinterpret_cast<unsigned long long*>(take(2 * sizeof(unsigned long long)));
  s.ranks = reinterpret_cast<unsigned long long*>(take(pairs * num_ranks * sizeof(unsigned long long)));
  s.values = reinterpret_cast<double*>(take(pairs * num_ranks * sizeof(double)));
  s.scale = reinterpret_cast<double*>(take(pairs * sizeof(double)));
  s.thr = reinterpret_cast<double*>(take(pairs * sizeof(double)));
  s.state = reinterpret_cast<sba::SelectState*>(take(pairs * sizeof(sba::SelectState)));
  s.hist = reinterpret_cast<unsigned long long*>(take(pairs * num_ranks * sba::kSelectBins * sizeof(unsigned long long)));
  s.sq = reinterpret_cast<double*>(take(sq_elems * sizeof(double)));
  s.bytes = off;
  return s;
}

// The handle's cached scratch, grown (or shrunk when far too large) only once the stream has drained.
int ensure_scratch(void** scratch, size_t* have, size_t need, hipStream_t stream, int* poisoned) {
  if (*have >= need && *have <= 4 * need + (size_t(1) << 20)) return SBA_OK;
  if (*scratch) {
    const int rc = sba::stream_wait(stream, "selection scratch", poisoned);
    if (rc) return rc;
    SBA_TRY_HIP(hipFree(*scratch));
  }
  *scratch = nullptr;
  *have = 0;
  SBA_TRY_HIP(hipMalloc(scratch, need));
  *have = need;
  return SBA_OK;
}

int check_scale(double scale) {
  if (!std::isfinite(scale) || scale < 0.0) return sba::set_error(SBA_ERR_INVALID_ARG, "scale must be finite and >= 0");
  return SBA_OK;
}

// ---- single problem ------------------------------------------------------------------------------------------------------
int check_problem(const sba_problem* p, int depth_mode, const double* rot, const double* tran, const size_t* ranks,
                  int num_ranks) {
  int rc = sba::shim::check_args(p, SBA_MODE_RT, depth_mode, rot, tran);   // the residual does not depend on the mode
  if (rc) return rc;
  if (sba::shim::is_collective(p) || p->shard_count != 1)
    return sba::set_error(SBA_ERR_UNSUPPORTED, "order statistics run on one unsharded problem: the histograms of the shards are not summed");
  if (p->n == 0) return sba::set_error(SBA_ERR_INVALID_ARG, "the problem holds no matches: there is nothing to select");
  for (int j = 0; j < num_ranks; ++j)
    if (ranks[j] >= p->n) return sba::set_error(SBA_ERR_INVALID_ARG, "rank %zu is not below the %zu matches", ranks[j], p->n);
  return SBA_OK;
}

int select_grid(const sba_problem* p) {
  const size_t want = (p->n + 1023) / 1024;   // a block takes 256 x 4 rows per step
  const int per_cu = p->blocks_per_cu_cap > 0 ? p->blocks_per_cu_cap : 8;
  return static_cast<int>(std::min<size_t>(want, static_cast<size_t>(p->num_cus) * per_cu));
}

// Enqueues the s plane (residual_kernel with the sq_norm output alone, exactly what sba_problem_residuals launches for it)
// and the selection.  host_offsets (2 words) and scale stay valid until the caller has waited for the stream.
int enqueue_problem_select(sba_problem* p, int depth_mode, const double rot[3], const double tran[3], double d1, double d2,
                           const size_t* ranks, int num_ranks, const double* scale, unsigned long long* host_offsets,
                           SelectScratch* out) {
  SBA_TRY_HIP(hipSetDevice(p->device));
  const size_t n = p->n;
  sba::Planes pl;
  int kernel_depth = depth_mode;
  int rc = sba::shim::sweep_planes(p, depth_mode, &pl, &kernel_depth);
  if (rc) return rc;
  sba::SweepParams prm;
  sba::make_sweep_params(n, depth_mode, rot, tran, d1, d2, 0.0, &prm);

  double* plane = nullptr;
  rc = sba::shim::select_plane(p, num_ranks, out, &plane);
  if (rc) return rc;
  const SelectScratch& s = *out;

  sba::ResidualOut res;
  res.e = nullptr;
  res.sq = s.sq;
  res.inlier = nullptr;
  res.n_inlier = s.n_inlier;
  SBA_TRY_HIP(hipMemsetAsync(res.n_inlier, 0, sizeof(unsigned long long), p->stream));
  const size_t ppt = static_cast<size_t>(sba::points_per_lane(p->store));
  const size_t want = ((n + ppt - 1) / ppt + sba::kBlock - 1) / sba::kBlock;
  const int per_cu = p->blocks_per_cu_cap > 0 ? p->blocks_per_cu_cap : 2;
  const int grid = static_cast<int>(std::min<size_t>(want, static_cast<size_t>(p->num_cus) * per_cu));
  SBA_TRY_HIP(sba::launch_residuals(kernel_depth, p->store, 2, pl, prm, res, grid, p->stream));
  return sba::shim::select_enqueue(p, s, ranks, num_ranks, scale, host_offsets);
}

}  // namespace

// ---- the selection over a plane that is already on the device (sba_problem.hpp) --------------------------------------------
namespace sba {
namespace shim {

int select_plane(sba_problem* p, int num_ranks, SelectScratch* s, double** plane) {
  const size_t need = carve(nullptr, 1, num_ranks, p->plane_elems).bytes;
  const int rc = ensure_scratch(&p->select_scratch, &p->select_scratch_bytes, need, p->stream, &p->poisoned);
  if (rc) return rc;
  *s = carve(static_cast<char*>(p->select_scratch), 1, num_ranks, p->plane_elems);
  *plane = s->sq;
  return SBA_OK;
}

int select_enqueue(sba_problem* p, const SelectScratch& s, const size_t* ranks, int num_ranks, const double* scale,
                   unsigned long long* host_offsets) {
  host_offsets[0] = 0;
  host_offsets[1] = p->n;
  SBA_TRY_HIP(hipMemcpyAsync(s.offsets, host_offsets, 2 * sizeof(unsigned long long), hipMemcpyHostToDevice, p->stream));
  SBA_TRY_HIP(hipMemcpyAsync(s.ranks, ranks, num_ranks * sizeof(unsigned long long), hipMemcpyHostToDevice, p->stream));
  if (scale) SBA_TRY_HIP(hipMemcpyAsync(s.scale, scale, sizeof(double), hipMemcpyHostToDevice, p->stream));
  SBA_TRY_HIP(sba::launch_order_stats(s.sq, s.offsets, 1, select_grid(p), s.ranks, num_ranks, scale ? s.scale : nullptr, s.state,
                                      s.hist, s.values, s.thr, p->stream));
  return SBA_OK;
}

int select_values(sba_problem* p, const SelectScratch& s, int num_ranks, double* values) {
  SBA_TRY_HIP(hipMemcpyAsync(values, s.values, num_ranks * sizeof(double), hipMemcpyDeviceToHost, p->stream));
  return sba::stream_wait(p->stream, "order statistics", &p->poisoned);
}

int select_keep(sba_problem* p, const SelectScratch& s, double* threshold, size_t* n_kept, long long* kept_index) {
  // The threshold kernel writes the compaction's keep bytes: the mask never leaves the device.
  CompactWork w(&p->poisoned);
  int rc = compact_alloc(p, &w);
  if (rc) return rc;
  SBA_TRY_HIP(sba::launch_keep_below(s.sq, s.offsets, 1, select_grid(p), s.thr, w.keep, s.kept, p->stream));
  double thr = 0.0;
  unsigned long long kept = 0;
  SBA_TRY_HIP(hipMemcpyAsync(&thr, s.thr, sizeof(double), hipMemcpyDeviceToHost, p->stream));
  SBA_TRY_HIP(hipMemcpyAsync(&kept, s.kept, sizeof(kept), hipMemcpyDeviceToHost, p->stream));
  rc = compact_rows(p, w, n_kept, kept_index);   // waits for the stream before it sizes the new planes
  if (rc) return rc;
  *threshold = thr;
  if (kept != *n_kept)
    return sba::set_error(SBA_ERR_NUMERIC, "the threshold kernel kept %llu matches, the compaction %zu", kept, *n_kept);
  return SBA_OK;
}

}  // namespace shim
}  // namespace sba

// ---- the same three steps for a batch (sba_batch.hpp) ------------------------------------------------------------------------
namespace sba {
namespace batch {

int grow_scratch(void** scratch, size_t* have, size_t need, hipStream_t stream, int* poisoned) {
  return ensure_scratch(scratch, have, need, stream, poisoned);
}

int select_plane(sba_batch* b, int num_ranks, SelectScratch* s, double** plane) {
  const size_t B = static_cast<size_t>(b->num_pairs), rows = batch_rows(b);
  const size_t need = carve(nullptr, B, num_ranks, rows).bytes;
  const int rc = ensure_scratch(&b->select_scratch, &b->select_scratch_bytes, need, b->stream, &b->poisoned);
  if (rc) return rc;
  *s = carve(static_cast<char*>(b->select_scratch), B, num_ranks, rows);
  *plane = s->sq;
  return SBA_OK;
}

int select_enqueue(sba_batch* b, const SelectScratch& s, const size_t* ranks, int num_ranks, const double* scale) {
  const size_t B = static_cast<size_t>(b->num_pairs);
  SBA_TRY_HIP(hipMemcpyAsync(s.ranks, ranks, B * num_ranks * sizeof(unsigned long long), hipMemcpyHostToDevice, b->stream));
  if (scale) SBA_TRY_HIP(hipMemcpyAsync(s.scale, scale, B * sizeof(double), hipMemcpyHostToDevice, b->stream));
  SBA_TRY_HIP(sba::launch_order_stats(s.sq, b->offsets_dev, b->num_pairs, b->bpp, s.ranks, num_ranks, scale ? s.scale : nullptr,
                                      s.state, s.hist, s.values, s.thr, b->stream));
  return SBA_OK;
}

int select_keep(sba_batch* b, const SelectScratch& s, double* threshold, size_t* n_kept, long long* kept_index) {
  const size_t B = static_cast<size_t>(b->num_pairs);
  CompactWork w(&b->poisoned);
  int rc = alloc_work(b, batch_rows(b), &w);
  if (rc) return rc;
  SBA_TRY_HIP(sba::launch_keep_below(s.sq, b->offsets_dev, b->num_pairs, b->bpp, s.thr, w.keep, s.kept, b->stream));
  std::vector<unsigned long long> kept(B);
  SBA_TRY_HIP(hipMemcpyAsync(threshold, s.thr, B * sizeof(double), hipMemcpyDeviceToHost, b->stream));
  SBA_TRY_HIP(hipMemcpyAsync(kept.data(), s.kept, B * sizeof(unsigned long long), hipMemcpyDeviceToHost, b->stream));
  rc = compact_rows(b, w, n_kept, kept_index);   // waits for the stream before it lays the batch out afresh
  if (rc) return rc;
  for (size_t g = 0; g < B; ++g)
    if (kept[g] != n_kept[g])
      return sba::set_error(SBA_ERR_NUMERIC, "pair %zu: the threshold kernel kept %llu matches, the compaction %zu", g, kept[g],
                            n_kept[g]);
  return SBA_OK;
}

}  // namespace batch
}  // namespace sba

namespace {

// ---- batch ---------------------------------------------------------------------------------------------------------------
int check_batch(const sba_batch* b, int depth_mode, const double* rot, const double* tran, const size_t* ranks, int num_ranks) {
  int rc = sba::batch::check_batch_args(b, SBA_MODE_RT, depth_mode, rot, tran);
  if (rc) return rc;
  for (int g = 0; g < b->num_pairs; ++g)
    for (int j = 0; j < num_ranks && b->n[g] > 0; ++j)   // an empty pair takes no part: its ranks are not looked at
      if (ranks[static_cast<size_t>(g) * num_ranks + j] >= b->n[g])
        return sba::set_error(SBA_ERR_INVALID_ARG, "pair %d: rank %zu is not below its %zu matches", g,
                              ranks[static_cast<size_t>(g) * num_ranks + j], b->n[g]);
  return SBA_OK;
}

int enqueue_batch_select(sba_batch* b, int depth_mode, const double* rot, const double* tran, const double* d1,
                         const double* d2, const size_t* ranks, int num_ranks, const double* scale, SelectScratch* out) {
  double* plane = nullptr;
  int rc = sba::batch::select_plane(b, num_ranks, out, &plane);
  if (rc) return rc;
  const SelectScratch& s = *out;
  sba::ResidualOut res;
  res.e = nullptr;
  res.sq = plane;
  res.inlier = nullptr;
  res.n_inlier = s.n_inlier;
  rc = sba::batch::residual_pass(b, depth_mode, rot, tran, d1, d2, 0.0, 2, res);
  if (rc) return rc;
  return sba::batch::select_enqueue(b, s, ranks, num_ranks, scale);
}

}  // namespace

extern "C" {

int sba_problem_residual_order_stats(sba_problem* p, int depth_mode, const double rot[3], const double tran[3], double d1,
                                     double d2, const size_t* ranks, int num_ranks, double* values) {
  if (!ranks || !values) return sba::set_error(SBA_ERR_INVALID_ARG, "ranks/values must not be null");
  if (num_ranks < 1 || num_ranks > sba::kSelectMaxRanks)
    return sba::set_error(SBA_ERR_INVALID_ARG, "num_ranks %d outside 1...%d", num_ranks, sba::kSelectMaxRanks);
  int rc = check_problem(p, depth_mode, rot, tran, ranks, num_ranks);
  if (rc) return rc;
  unsigned long long host_offsets[2];
  SelectScratch s;
  rc = enqueue_problem_select(p, depth_mode, rot, tran, d1, d2, ranks, num_ranks, nullptr, host_offsets, &s);
  if (rc) return rc;
  return sba::shim::select_values(p, s, num_ranks, values);
}

int sba_problem_keep_below(sba_problem* p, int depth_mode, const double rot[3], const double tran[3], double d1, double d2,
                           size_t rank, double scale, double* threshold, size_t* n_kept, long long* kept_index) {
  if (!threshold || !n_kept) return sba::set_error(SBA_ERR_INVALID_ARG, "threshold/n_kept must not be null");
  int rc = check_scale(scale);
  if (rc) return rc;
  rc = check_problem(p, depth_mode, rot, tran, &rank, 1);
  if (rc) return rc;
  unsigned long long host_offsets[2];
  SelectScratch s;
  rc = enqueue_problem_select(p, depth_mode, rot, tran, d1, d2, &rank, 1, &scale, host_offsets, &s);
  if (rc) return rc;
  return sba::shim::select_keep(p, s, threshold, n_kept, kept_index);
}

int sba_batch_residual_order_stats(sba_batch* b, int depth_mode, const double* rot, const double* tran, const double* d1,
                                   const double* d2, const size_t* ranks, int num_ranks, double* values) {
  if (!ranks || !values) return sba::set_error(SBA_ERR_INVALID_ARG, "ranks/values must not be null");
  if (num_ranks < 1 || num_ranks > sba::kSelectMaxRanks)
    return sba::set_error(SBA_ERR_INVALID_ARG, "num_ranks %d outside 1...%d", num_ranks, sba::kSelectMaxRanks);
  int rc = check_batch(b, depth_mode, rot, tran, ranks, num_ranks);
  if (rc) return rc;
  const size_t B = static_cast<size_t>(b->num_pairs);
  if (B == 0) return SBA_OK;
  if (sba::batch::batch_rows(b) == 0) {
    std::fill(values, values + B * num_ranks, std::numeric_limits<double>::quiet_NaN());
    return SBA_OK;
  }
  SBA_TRY_HIP(hipSetDevice(b->device));
  SelectScratch s;
  rc = enqueue_batch_select(b, depth_mode, rot, tran, d1, d2, ranks, num_ranks, nullptr, &s);
  if (rc) return rc;
  SBA_TRY_HIP(hipMemcpyAsync(values, s.values, B * num_ranks * sizeof(double), hipMemcpyDeviceToHost, b->stream));
  return sba::stream_wait(b->stream, "batch order statistics", &b->poisoned);
}

int sba_batch_keep_below(sba_batch* b, int depth_mode, const double* rot, const double* tran, const double* d1,
                         const double* d2, const size_t* rank, const double* scale, double* threshold, size_t* n_kept,
                         long long* kept_index) {
  if (!rank || !scale || !threshold || !n_kept)
    return sba::set_error(SBA_ERR_INVALID_ARG, "rank/scale/threshold/n_kept must not be null");
  int rc = check_batch(b, depth_mode, rot, tran, rank, 1);
  if (rc) return rc;
  const size_t B = static_cast<size_t>(b->num_pairs);
  for (size_t g = 0; g < B; ++g) {
    rc = check_scale(scale[g]);
    if (rc) return rc;
  }
  if (B == 0) return SBA_OK;
  SBA_TRY_HIP(hipSetDevice(b->device));
  const size_t rows = sba::batch::batch_rows(b);
  if (rows == 0) {
    std::fill(threshold, threshold + B, std::numeric_limits<double>::quiet_NaN());
    sba::batch::compact_nothing(b, n_kept);
    return SBA_OK;
  }
  SelectScratch s;
  rc = enqueue_batch_select(b, depth_mode, rot, tran, d1, d2, rank, 1, scale, &s);
  if (rc) return rc;
  return sba::batch::select_keep(b, s, threshold, n_kept, kept_index);
}

}  // extern "C"
