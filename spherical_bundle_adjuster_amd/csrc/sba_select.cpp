// Entry points that look at single matches (include/sba_hip.h): the per-match residuals of a problem and the stable
// compaction of its matches.  Kernels: sba_select.hip.
#include <algorithm>
#include <cstring>

#include "sba_problem.hpp"

using sba::shim::alloc_planes;
using sba::shim::check_args;
using sba::shim::ensure_folded;
using sba::shim::sweep_planes;

#define SBA_SELECT_SYNC(p, what)                                              \
  do {                                                                        \
    const int _rc = sba::stream_wait((p)->stream, what, &(p)->poisoned);      \
    if (_rc) return _rc;                                                      \
  } while (0)

extern "C" {

int sba_problem_residuals(sba_problem* p, int depth_mode, const double rot[3], const double tran[3], double d1, double d2,
                          double huber_delta, double* e_xyz, double* sq_norm, unsigned char* inlier, size_t* n_inlier) {
  int rc = check_args(p, SBA_MODE_RT, depth_mode, rot, tran);   // the residual does not depend on the mode
  if (rc) return rc;
  SBA_TRY_HIP(hipSetDevice(p->device));
  const size_t n = p->n;
  if (n == 0) {
    if (n_inlier) *n_inlier = 0;
    return SBA_OK;
  }
  sba::Planes pl;
  int kernel_depth = depth_mode;
  rc = sweep_planes(p, depth_mode, &pl, &kernel_depth);
  if (rc) return rc;
  sba::SweepParams prm;
  sba::make_sweep_params(n, depth_mode, rot, tran, d1, d2, huber_delta, &prm);

  // Scratch in the handle: the count word, then the requested outputs over whole vectors of the planes (plane_elems).
  const int outputs = (e_xyz ? 1 : 0) | (sq_norm ? 2 : 0) | (inlier ? 4 : 0);
  const size_t elems = p->plane_elems;
  auto up = [](size_t b) { return (b + 255) & ~size_t(255); };
  const size_t off_e = 256, off_sq = off_e + (e_xyz ? up(elems * 3 * sizeof(double)) : 0);
  const size_t off_in = off_sq + (sq_norm ? up(elems * sizeof(double)) : 0);
  const size_t need = off_in + (inlier ? up(elems) : 0);
  if (p->select_scratch_bytes < need || p->select_scratch_bytes > 4 * need + (size_t(1) << 20)) {
    if (p->select_scratch) SBA_TRY_HIP(hipFree(p->select_scratch));
    p->select_scratch = nullptr;
    p->select_scratch_bytes = 0;
    SBA_TRY_HIP(hipMalloc(&p->select_scratch, need));
    p->select_scratch_bytes = need;
  }
  char* scratch = static_cast<char*>(p->select_scratch);
  sba::ResidualOut out;
  out.n_inlier = reinterpret_cast<unsigned long long*>(scratch);
  out.e = reinterpret_cast<double*>(scratch + off_e);
  out.sq = reinterpret_cast<double*>(scratch + off_sq);
  out.inlier = reinterpret_cast<unsigned char*>(scratch + off_in);
  SBA_TRY_HIP(hipMemsetAsync(out.n_inlier, 0, sizeof(unsigned long long), p->stream));

  // one resident wave of blocks (SBA_BLOCKS_PER_CU, else two per CU), grid-stride beyond
  const size_t ppt = static_cast<size_t>(sba::points_per_lane(p->store));
  const size_t want = ((n + ppt - 1) / ppt + sba::kBlock - 1) / sba::kBlock;
  const int per_cu = p->blocks_per_cu_cap > 0 ? p->blocks_per_cu_cap : 2;
  const int grid = static_cast<int>(std::min<size_t>(want, static_cast<size_t>(p->num_cus) * per_cu));
  SBA_TRY_HIP(sba::launch_residuals(kernel_depth, p->store, outputs, pl, prm, out, grid, p->stream));

  if (e_xyz) SBA_TRY_HIP(hipMemcpyAsync(e_xyz, out.e, n * 3 * sizeof(double), hipMemcpyDeviceToHost, p->stream));
  if (sq_norm) SBA_TRY_HIP(hipMemcpyAsync(sq_norm, out.sq, n * sizeof(double), hipMemcpyDeviceToHost, p->stream));
  if (inlier) SBA_TRY_HIP(hipMemcpyAsync(inlier, out.inlier, n, hipMemcpyDeviceToHost, p->stream));
  unsigned long long count = 0;
  SBA_TRY_HIP(hipMemcpyAsync(&count, out.n_inlier, sizeof(count), hipMemcpyDeviceToHost, p->stream));
  SBA_SELECT_SYNC(p, "residuals");
  if (n_inlier) *n_inlier = static_cast<size_t>(count);
  return SBA_OK;
}

int sba_problem_compact(sba_problem* p, const unsigned char* keep, size_t* n_kept, long long* kept_index) {
  if (!p) return sba::set_error(SBA_ERR_INVALID_ARG, "null problem handle");
  SBA_REFUSE_POISONED(p);
  if (!n_kept) return sba::set_error(SBA_ERR_INVALID_ARG, "n_kept is null");
  if (!p->uploaded) return sba::set_error(SBA_ERR_NOT_UPLOADED, "no correspondences uploaded");
  const size_t n = p->n;
  if (n > 0 && !keep) return sba::set_error(SBA_ERR_INVALID_ARG, "keep is null");
  SBA_TRY_HIP(hipSetDevice(p->device));
  if (n == 0) {
    *n_kept = 0;
    return SBA_OK;
  }

  sba::shim::CompactWork w(&p->poisoned);
  int rc = sba::shim::compact_alloc(p, &w);
  if (rc) return rc;
  SBA_TRY_HIP(hipMemcpyAsync(w.keep, keep, n, hipMemcpyHostToDevice, p->stream));
  return sba::shim::compact_rows(p, w, n_kept, kept_index);
}

}  // extern "C"

namespace sba {
namespace shim {

// keep bytes (whole tiles, zero beyond n) | tile counts | tile offsets | total
int compact_alloc(sba_problem* p, CompactWork* w) {
  const size_t n = p->n;
  const size_t ntiles = (n + sba::kCompactTile - 1) / sba::kCompactTile;
  auto up = [](size_t b) { return (b + 255) & ~size_t(255); };
  const size_t keep_bytes = ntiles * sba::kCompactTile;
  const size_t off_count = up(keep_bytes), off_offset = off_count + up(ntiles * sizeof(unsigned int));
  const size_t off_total = off_offset + up(ntiles * sizeof(unsigned long long));
  SBA_TRY_HIP(w->buf.alloc(off_total + 256));
  w->ntiles = ntiles;
  w->keep = w->buf.as<unsigned char>();
  w->tile_count = reinterpret_cast<unsigned int*>(w->buf.as<char>() + off_count);
  w->tile_offset = reinterpret_cast<unsigned long long*>(w->buf.as<char>() + off_offset);
  w->total = reinterpret_cast<unsigned long long*>(w->buf.as<char>() + off_total);
  if (keep_bytes > n) SBA_TRY_HIP(hipMemsetAsync(w->keep + n, 0, keep_bytes - n, p->stream));
  return SBA_OK;
}

int compact_rows(sba_problem* p, CompactWork& w, size_t* n_kept, long long* kept_index) {
  const size_t n = p->n, ntiles = w.ntiles;
  unsigned char* keep_dev = w.keep;
  unsigned long long* tile_offset = w.tile_offset;
  SBA_TRY_HIP(sba::launch_compact_count(keep_dev, ntiles, w.tile_count, p->stream));
  SBA_TRY_HIP(sba::launch_compact_scan(w.tile_count, ntiles, tile_offset, w.total, p->stream));
  unsigned long long total = 0;
  SBA_TRY_HIP(hipMemcpyAsync(&total, w.total, sizeof(total), hipMemcpyDeviceToHost, p->stream));
  SBA_SELECT_SYNC(p, "compaction count");   // the one synchronous step: the new planes are sized by it
  const size_t m = static_cast<size_t>(total);

  // Out of place: the current planes leave the handle, alloc_planes lays out fresh zeroed ones for m matches exactly as an
  // upload of m matches does, the scatter fills them, and the old ones are freed once the stream has drained.
  const bool with_d12 = p->has_d12;
  const int store = p->store;
  void* old_base[8];
  sba::CompactArgs a;
  a.keep = keep_dev;
  a.n = n;
  a.tile_offset = tile_offset;
  for (int k = 0; k < 8; ++k) {
    old_base[k] = p->plane_base[k];
    p->plane_base[k] = nullptr;
    p->plane_bytes[k] = 0;
    a.src[k] = k < 6 ? p->coord[k] : (with_d12 ? p->dplane[k - 6] : nullptr);
  }
  auto release_old = [&]() {
    const int rc_wait = sba::stream_wait(p->stream, "compaction", &p->poisoned);
    if (!p->poisoned)       // a poisoned handle leaks them: hipFree would wait for the wedged device
      for (void* b : old_base)
        if (b) (void)hipFree(b);
    return rc_wait;
  };
  int rc = alloc_planes(p, m, with_d12, store);   // the handle is not `uploaded` until the scatter is in place
  if (rc) {
    (void)release_old();
    return rc;
  }
  for (int k = 0; k < 8; ++k) a.dst[k] = k < 6 ? p->coord[k] : (with_d12 ? p->dplane[k - 6] : nullptr);
  sba::DeviceBuffer index_dev(&p->poisoned);
  a.kept_index = nullptr;
  hipError_t e = hipSuccess;
  if (kept_index && m > 0) {
    e = index_dev.alloc(m * sizeof(long long));
    a.kept_index = index_dev.as<long long>();
  }
  if (e == hipSuccess) e = sba::launch_compact_scatter(store, a, ntiles, p->stream);
  if (e == hipSuccess && a.kept_index)
    e = hipMemcpyAsync(kept_index, a.kept_index, m * sizeof(long long), hipMemcpyDeviceToHost, p->stream);
  rc = release_old();
  if (e != hipSuccess) return sba::set_error(SBA_ERR_HIP, "compaction: %s", hipGetErrorString(e));
  if (rc) return rc;
  p->uploaded = true;
  rc = ensure_folded(p);
  if (rc) return rc;
  SBA_SELECT_SYNC(p, "stream synchronisation");
  *n_kept = m;
  return SBA_OK;
}

}  // namespace shim
}  // namespace sba
