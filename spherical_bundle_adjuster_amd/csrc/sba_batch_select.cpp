// Entry points that look at single matches of a batch (include/sba_hip.h): every pair's per-match residuals and the stable
// compaction of every pair's matches.  Kernels: sba_select.hip.
#include <algorithm>
#include <cstring>
#include <vector>

#include "sba_batch.hpp"

using sba::batch::check_batch_args;

#define SBA_BATCH_SYNC(b, what)                                               \
  do {                                                                        \
    const int _rc = sba::stream_wait((b)->stream, what, &(b)->poisoned);      \
    if (_rc) return _rc;                                                      \
  } while (0)

namespace {
size_t up256(size_t v) { return (v + 255) & ~size_t(255); }
}  // namespace

namespace sba {
namespace batch {

size_t batch_rows(const sba_batch* b) { return b->offsets.back() - b->offsets.front(); }

sba::Planes batch_planes(const sba_batch* b) {
  sba::Planes pl;
  for (int k = 0; k < 3; ++k) { pl.x1[k] = b->coord[k]; pl.x2[k] = b->coord[3 + k]; }
  pl.d1 = b->dplane[0];
  pl.d2 = b->dplane[1];
  return pl;
}

// The residual kernel at (rot, tran, d1, d2): every pair's sweep state is built on the device from the same 80-byte record a
// batched step reads, so the residuals carry the sweep's bits.  out.n_inlier: num_pairs device words, zeroed here.
int residual_pass(sba_batch* b, int depth_mode, const double* rot, const double* tran, const double* d1, const double* d2,
                  double huber_delta, int outputs, const sba::ResidualOut& out) {
  sba::batch::write_state(b, rot, tran, d1, d2, nullptr);
  SBA_TRY_HIP(hipMemsetAsync(out.n_inlier, 0, sizeof(unsigned long long) * b->num_pairs, b->stream));
  SBA_TRY_HIP(sba::launch_batch_residuals(depth_mode, b->store, outputs, batch_planes(b), b->desc_dev, b->offsets_dev,
                                          b->state_host_dev, huber_delta, b->num_pairs, b->bpp, out, b->stream));
  return SBA_OK;
}

int alloc_work(sba_batch* b, size_t rows, CompactWork* w) {
  const size_t B = static_cast<size_t>(b->num_pairs);
  w->rows = rows;
  w->ntiles = (rows + sba::kCompactTile - 1) / sba::kCompactTile;
  const size_t keep_bytes = w->ntiles * sba::kCompactTile;
  const size_t off_count = up256(keep_bytes), off_offset = off_count + up256(w->ntiles * sizeof(unsigned int));
  const size_t off_total = off_offset + up256(w->ntiles * sizeof(unsigned long long)), off_kept = off_total + 256;
  const size_t off_inl = off_kept + up256(B * sizeof(unsigned long long)), bytes = off_inl + up256(B * sizeof(unsigned long long));
  SBA_TRY_HIP(w->buf.alloc(bytes));
  char* base = w->buf.as<char>();
  w->keep = reinterpret_cast<unsigned char*>(base);
  w->tile_count = reinterpret_cast<unsigned int*>(base + off_count);
  w->tile_offset = reinterpret_cast<unsigned long long*>(base + off_offset);
  w->total = reinterpret_cast<unsigned long long*>(base + off_total);
  w->pair_kept = reinterpret_cast<unsigned long long*>(base + off_kept);
  w->n_inlier = reinterpret_cast<unsigned long long*>(base + off_inl);
  if (keep_bytes > rows) SBA_TRY_HIP(hipMemsetAsync(w->keep + rows, 0, keep_bytes - rows, b->stream));
  return SBA_OK;
}

// w.keep holds the rows' flags (queued on the stream).  Counts every pair's kept rows -- the one synchronous step: the new
// layout is sized by them -- then lays the batch out afresh for those counts (layout_pairs, as an upload of the kept rows
// would) and moves the kept rows from the old planes into the new ones.  The old planes, descriptors and row offsets leave the
// handle first and are freed once the stream has drained; every other buffer sized by the layout is dropped and re-created
// on first use, as after an upload.
int compact_rows(sba_batch* b, CompactWork& w, size_t* n_kept, long long* kept_index) {
  const int B = b->num_pairs;
  SBA_TRY_HIP(sba::launch_compact_count(w.keep, w.ntiles, w.tile_count, b->stream));
  SBA_TRY_HIP(sba::launch_compact_scan(w.tile_count, w.ntiles, w.tile_offset, w.total, b->stream));
  SBA_TRY_HIP(sba::launch_batch_pair_kept(w.keep, w.tile_offset, w.ntiles, w.total, b->offsets_dev, B, w.pair_kept, b->stream));
  std::vector<unsigned long long> kept(B);
  SBA_TRY_HIP(hipMemcpyAsync(kept.data(), w.pair_kept, sizeof(unsigned long long) * B, hipMemcpyDeviceToHost, b->stream));
  SBA_BATCH_SYNC(b, "batch compaction count");
  std::vector<size_t> offsets(static_cast<size_t>(B) + 1, 0);
  for (int g = 0; g < B; ++g) offsets[g + 1] = offsets[g] + static_cast<size_t>(kept[g]);
  const size_t m = offsets[B];

  const int store = b->store;
  const bool has_d12 = b->has_d12;
  sba::BatchCompactArgs a;
  a.keep = w.keep;
  a.rows = w.rows;
  a.tile_offset = w.tile_offset;
  a.old_offsets = b->offsets_dev;
  a.old_desc = b->desc_dev;
  a.num_pairs = B;
  void* old_base[8];
  for (int k = 0; k < 8; ++k) {
    old_base[k] = b->plane_base[k];
    b->plane_base[k] = nullptr;
    a.src[k] = k < 6 ? b->coord[k] : (has_d12 ? b->dplane[k - 6] : nullptr);
  }
  b->desc_dev = nullptr;
  b->offsets_dev = nullptr;
  auto release_old = [&]() {
    const int rc_wait = sba::stream_wait(b->stream, "batch compaction", &b->poisoned);
    if (!b->poisoned) {     // a poisoned handle leaks them: hipFree would wait for the wedged device
      for (void* p : old_base)
        if (p) (void)hipFree(p);
      (void)hipFree(const_cast<sba::PairDesc*>(a.old_desc));
      (void)hipFree(const_cast<unsigned long long*>(a.old_offsets));
    }
    return rc_wait;
  };
  b->uploaded = false;      // until the scatter is in place
  int rc = sba::batch::free_batch_data(b);
  if (!rc) rc = sba::batch::layout_pairs(b, offsets.data(), B, store, has_d12);
  if (rc) {
    (void)release_old();
    return rc;
  }
  a.new_offsets = b->offsets_dev;
  a.new_desc = b->desc_dev;
  for (int k = 0; k < 8; ++k) a.dst[k] = k < 6 ? b->coord[k] : (has_d12 ? b->dplane[k - 6] : nullptr);
  sba::DeviceBuffer index_dev(&b->poisoned);
  a.kept_index = nullptr;
  hipError_t e = hipSuccess;
  if (kept_index && m > 0) {
    e = index_dev.alloc(m * sizeof(long long));
    a.kept_index = index_dev.as<long long>();
  }
  if (e == hipSuccess) e = sba::launch_batch_compact_scatter(store, a, w.ntiles, b->stream);
  if (e == hipSuccess && a.kept_index)
    e = hipMemcpyAsync(kept_index, a.kept_index, m * sizeof(long long), hipMemcpyDeviceToHost, b->stream);
  rc = release_old();
  if (e != hipSuccess) return sba::set_error(SBA_ERR_HIP, "batch compaction: %s", hipGetErrorString(e));
  if (rc) return rc;
  b->uploaded = true;
  for (int g = 0; g < B; ++g) n_kept[g] = static_cast<size_t>(kept[g]);
  return SBA_OK;
}

// No rows at all: every pair keeps nothing, and the offsets become those of an upload of nothing.
void compact_nothing(sba_batch* b, size_t* n_kept) {
  std::fill(n_kept, n_kept + b->num_pairs, size_t(0));
  b->offsets.assign(static_cast<size_t>(b->num_pairs) + 1, 0);
}

}  // namespace batch
}  // namespace sba

using sba::batch::CompactWork;
using sba::batch::alloc_work;
using sba::batch::batch_rows;
using sba::batch::compact_nothing;
using sba::batch::compact_rows;
using sba::batch::residual_pass;

extern "C" {

int sba_batch_residuals(sba_batch* b, int depth_mode, const double* rot, const double* tran, const double* d1,
                        const double* d2, double huber_delta, double* e_xyz, double* sq_norm, unsigned char* inlier,
                        size_t* n_inlier) {
  int rc = check_batch_args(b, SBA_MODE_RT, depth_mode, rot, tran);   // the residual does not depend on the mode
  if (rc) return rc;
  const int B = b->num_pairs;
  if (B == 0) return SBA_OK;
  SBA_TRY_HIP(hipSetDevice(b->device));
  const size_t rows = batch_rows(b);

  // Scratch in the handle: the per-pair counts, then the requested outputs, row-ordered.
  const int outputs = (e_xyz ? 1 : 0) | (sq_norm ? 2 : 0) | (inlier ? 4 : 0);
  const size_t off_e = up256(sizeof(unsigned long long) * B), off_sq = off_e + (e_xyz ? up256(rows * 3 * sizeof(double)) : 0);
  const size_t off_in = off_sq + (sq_norm ? up256(rows * sizeof(double)) : 0);
  const size_t need = off_in + (inlier ? up256(rows) : 0);
  if (b->select_scratch_bytes < need || b->select_scratch_bytes > 4 * need + (size_t(1) << 20)) {
    if (b->select_scratch) SBA_TRY_HIP(hipFree(b->select_scratch));
    b->select_scratch = nullptr;
    b->select_scratch_bytes = 0;
    SBA_TRY_HIP(hipMalloc(&b->select_scratch, need));
    b->select_scratch_bytes = need;
  }
  char* scratch = static_cast<char*>(b->select_scratch);
  sba::ResidualOut out;
  out.n_inlier = reinterpret_cast<unsigned long long*>(scratch);
  out.e = reinterpret_cast<double*>(scratch + off_e);
  out.sq = reinterpret_cast<double*>(scratch + off_sq);
  out.inlier = reinterpret_cast<unsigned char*>(scratch + off_in);
  rc = residual_pass(b, depth_mode, rot, tran, d1, d2, huber_delta, outputs, out);
  if (rc) return rc;
  if (rows > 0) {
    if (e_xyz) SBA_TRY_HIP(hipMemcpyAsync(e_xyz, out.e, rows * 3 * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    if (sq_norm) SBA_TRY_HIP(hipMemcpyAsync(sq_norm, out.sq, rows * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    if (inlier) SBA_TRY_HIP(hipMemcpyAsync(inlier, out.inlier, rows, hipMemcpyDeviceToHost, b->stream));
  }
  std::vector<unsigned long long> count(B);
  SBA_TRY_HIP(hipMemcpyAsync(count.data(), out.n_inlier, sizeof(unsigned long long) * B, hipMemcpyDeviceToHost, b->stream));
  SBA_BATCH_SYNC(b, "batch residuals");
  if (n_inlier)
    for (int g = 0; g < B; ++g) n_inlier[g] = static_cast<size_t>(count[g]);
  return SBA_OK;
}

int sba_batch_compact(sba_batch* b, const unsigned char* keep, size_t* n_kept, long long* kept_index) {
  if (!b) return sba::set_error(SBA_ERR_INVALID_ARG, "null batch handle");
  SBA_REFUSE_POISONED(b);
  if (!n_kept) return sba::set_error(SBA_ERR_INVALID_ARG, "n_kept is null");
  if (!b->uploaded) return sba::set_error(SBA_ERR_NOT_UPLOADED, "no pairs uploaded");
  if (b->num_pairs == 0) return SBA_OK;
  const size_t rows = batch_rows(b);
  if (rows > 0 && !keep) return sba::set_error(SBA_ERR_INVALID_ARG, "keep is null");
  SBA_TRY_HIP(hipSetDevice(b->device));
  if (rows == 0) {
    compact_nothing(b, n_kept);
    return SBA_OK;
  }
  CompactWork w(&b->poisoned);
  int rc = alloc_work(b, rows, &w);
  if (rc) return rc;
  SBA_TRY_HIP(hipMemcpyAsync(w.keep, keep, rows, hipMemcpyHostToDevice, b->stream));
  return compact_rows(b, w, n_kept, kept_index);
}

int sba_batch_keep_inliers(sba_batch* b, int depth_mode, const double* rot, const double* tran, const double* d1,
                           const double* d2, double huber_delta, size_t* n_kept, long long* kept_index) {
  int rc = check_batch_args(b, SBA_MODE_RT, depth_mode, rot, tran);
  if (rc) return rc;
  if (!n_kept) return sba::set_error(SBA_ERR_INVALID_ARG, "n_kept is null");
  if (b->num_pairs == 0) return SBA_OK;
  SBA_TRY_HIP(hipSetDevice(b->device));
  const size_t rows = batch_rows(b);
  if (rows == 0) {
    compact_nothing(b, n_kept);
    return SBA_OK;
  }
  // The residual kernel writes the inlier flags straight into the compaction's keep bytes: the mask stays on the device.
  CompactWork w(&b->poisoned);
  rc = alloc_work(b, rows, &w);
  if (rc) return rc;
  sba::ResidualOut out;
  out.e = nullptr;
  out.sq = nullptr;
  out.inlier = w.keep;
  out.n_inlier = w.n_inlier;
  rc = residual_pass(b, depth_mode, rot, tran, d1, d2, huber_delta, 4, out);
  if (rc) return rc;
  return compact_rows(b, w, n_kept, kept_index);
}

}  // extern "C"
