// Entry points of the landmark map (include/sba_hip.h: sba_landmarks_*): a handle of its own that keeps n landmarks with their
// 3 x 3 covariances and observation counts on the device as planes, and fuses a registered frame's bearings into them, one
// streaming pass per frame.  Kernels: sba_landmarks.hip; the per-observation code, the state of a pass and the option and
// index checks: sba_landmarks.hpp.  Below them the edits of the map -- scores, prune, append, gather -- with their kernels in
// sba_landmarks_edit.hip and their checks in sba_landmarks_edit.hpp.  Every wait is the bounded stream_wait; a handle whose wait
// gave up is poisoned.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>

#include "sba_internal.hpp"
#include "sba_landmarks.hpp"
#include "sba_landmarks_edit.hpp"

struct sba_landmarks {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  int poisoned = 0;
  int num_cus = 0;
  size_t n = 0;                 // landmarks
  size_t elems = 0;             // per plane: n rounded up to a whole 16-byte vector
  double* planes = nullptr;     // [9][elems] doubles, then [elems] u32 counts
  size_t planes_bytes = 0;
  // One fusion pass's observations, kept across calls: 4 class counters, chi2 [elems], bearings [elems][3], idx [elems].
  void* obs = nullptr;
  size_t obs_bytes = 0;
  int occ_fuse[2][2] = {{0, 0}, {0, 0}};   // resident blocks per CU of landmarks_fuse_kernel per [indexed][apply], 0 = unknown
  int occ_pack[2] = {0, 0};                // ... of the pack and the unpack kernel
  // The edits (scores, prune, append, gather; below sba_landmarks_fuse).  A prune and an append write the other plane allocation
  // and swap the two: the retired one is kept for the next edit.  edit: the scratch of one edit, kept across calls.
  double* planes_alt = nullptr;
  size_t planes_alt_bytes = 0;
  void* edit = nullptr;
  size_t edit_bytes = 0;
  int occ_edit[sba::LANDMARK_EDIT_KERNELS] = {0, 0, 0, 0};
};

namespace {

size_t planes_size(size_t elems) { return (9 * elems * sizeof(double) + elems * sizeof(uint32_t) + 15) / 16 * 16; }

sba::LandmarkPlanes planes_of(const sba_landmarks* h) { return sba::LandmarkPlanes{h->planes, h->elems}; }

// Blocks of a pass over `items` lane items: what fits the device at the reported occupancy, capped by SBA_RESECT_GRID (tests).
int grid_for(const sba_landmarks* h, size_t items, int occ) {
  const size_t blocks = (items + 255) / 256;
  int cap = 1 << 30;
  if (const char* env = std::getenv("SBA_RESECT_GRID")) { const int v = std::atoi(env); if (v >= 1) cap = v; }
  return static_cast<int>(std::min<size_t>({blocks, static_cast<size_t>(h->num_cus) * static_cast<size_t>(std::max(1, occ)), static_cast<size_t>(cap)}));
}

int pack_occ(sba_landmarks* h, bool unpack, int* occ) {
  int& o = h->occ_pack[unpack ? 1 : 0];
  if (o == 0) {
    SBA_TRY_HIP(sba::landmarks_pack_blocks_per_cu(unpack, &o));
    o = std::max(1, o);
  }
  *occ = o;
  return SBA_OK;
}

bool finite3(const double* a) { return std::isfinite(a[0]) && std::isfinite(a[1]) && std::isfinite(a[2]); }

int set_common(sba_landmarks* h, const void* xyz, const void* cov, size_t n, double cov_scale, bool from_device) {
  if (!h) return sba::set_error(SBA_ERR_INVALID_ARG, "null landmark handle");
  SBA_REFUSE_POISONED(h);
  if (n > 0 && (!xyz || !cov)) return sba::set_error(SBA_ERR_INVALID_ARG, "null landmark or covariance array");
  if (from_device && ((reinterpret_cast<uintptr_t>(xyz) | reinterpret_cast<uintptr_t>(cov)) & 15u))
    return sba::set_error(SBA_ERR_INVALID_ARG, "the landmark and covariance rows must be 16-byte aligned");
  if (const char* why = sba::resect_weight_check_scale(cov_scale)) return sba::set_error(SBA_ERR_INVALID_ARG, "%s", why);
  SBA_TRY_HIP(hipSetDevice(h->device));
  const size_t elems = (n + 1) / 2 * 2, bytes = planes_size(elems);
  h->n = 0; h->elems = 0;        // the map is replaced: empty until the new rows are in place
  if (n == 0) return SBA_OK;
  if (h->planes_bytes < bytes) {
    if (h->planes) SBA_TRY_HIP(hipFree(h->planes));
    h->planes = nullptr; h->planes_bytes = 0;
    SBA_TRY_HIP(hipMalloc(reinterpret_cast<void**>(&h->planes), bytes));
    h->planes_bytes = bytes;
  }
  sba::DeviceBuffer staging(&h->poisoned);
  const double *xyz_dev = static_cast<const double*>(xyz), *cov_dev = static_cast<const double*>(cov);
  if (!from_device) {            // covariance rows first: 48 n bytes keep the landmark rows 16-byte aligned
    SBA_TRY_HIP(staging.alloc(9 * n * sizeof(double)));
    double* s = staging.as<double>();
    SBA_TRY_HIP(hipMemcpyAsync(s, cov, 6 * n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    SBA_TRY_HIP(hipMemcpyAsync(s + 6 * n, xyz, 3 * n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    cov_dev = s; xyz_dev = s + 6 * n;
  }
  int occ = 1;
  int rc = pack_occ(h, false, &occ);
  if (rc) return rc;
  const sba::LandmarkPlanes pl{h->planes, elems};
  SBA_TRY_HIP(sba::launch_landmarks_pack(xyz_dev, cov_dev, n, cov_scale, pl, grid_for(h, elems / 2, occ), h->stream));
  rc = sba::stream_wait(h->stream, "landmark pack", &h->poisoned);
  if (rc) return rc;
  h->n = n; h->elems = elems;
  return SBA_OK;
}

int get_common(sba_landmarks* h, void* xyz, void* cov, bool to_device) {
  if (!h) return sba::set_error(SBA_ERR_INVALID_ARG, "null landmark handle");
  SBA_REFUSE_POISONED(h);
  if (to_device && ((reinterpret_cast<uintptr_t>(xyz) | reinterpret_cast<uintptr_t>(cov)) & 15u))
    return sba::set_error(SBA_ERR_INVALID_ARG, "the landmark and covariance rows must be 16-byte aligned");
  if (h->n == 0 || (!xyz && !cov)) return SBA_OK;
  SBA_TRY_HIP(hipSetDevice(h->device));
  const size_t n = h->n;
  int occ = 1;
  int rc = pack_occ(h, true, &occ);
  if (rc) return rc;
  const int grid = grid_for(h, h->elems / 2, occ);
  if (to_device) {
    SBA_TRY_HIP(sba::launch_landmarks_unpack(planes_of(h), n, static_cast<double*>(xyz), static_cast<double*>(cov), grid, h->stream));
    return sba::stream_wait(h->stream, "landmark unpack", &h->poisoned);
  }
  sba::DeviceBuffer staging(&h->poisoned);
  SBA_TRY_HIP(staging.alloc(9 * n * sizeof(double)));
  double* s = staging.as<double>();
  SBA_TRY_HIP(sba::launch_landmarks_unpack(planes_of(h), n, xyz ? s + 6 * n : nullptr, cov ? s : nullptr, grid, h->stream));
  if (cov) SBA_TRY_HIP(hipMemcpyAsync(cov, s, 6 * n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (xyz) SBA_TRY_HIP(hipMemcpyAsync(xyz, s + 6 * n, 3 * n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  return sba::stream_wait(h->stream, "landmark unpack", &h->poisoned);
}

}  // namespace

extern "C" {

int sba_landmarks_create(sba_landmarks** out, int device, void* stream) {
  if (!out) return sba::set_error(SBA_ERR_INVALID_ARG, "out is null");
  *out = nullptr;
  int count = 0;
  const hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0)
    return sba::set_error(SBA_ERR_NO_DEVICE, "no HIP device available (%s); this library has no CPU path",
                          e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
  if (device < 0 || device >= count) return sba::set_error(SBA_ERR_INVALID_ARG, "device %d out of range [0,%d)", device, count);
  SBA_TRY_HIP(hipSetDevice(device));
  struct Guard {
    sba_landmarks* h;
    ~Guard() { if (h) (void)sba_landmarks_destroy(h); }
  } guard{new (std::nothrow) sba_landmarks()};
  sba_landmarks* h = guard.h;
  if (!h) return sba::set_error(SBA_ERR_HIP, "out of host memory");
  h->device = device;
  hipDeviceProp_t prop;
  SBA_TRY_HIP(hipGetDeviceProperties(&prop, device));
  h->num_cus = prop.multiProcessorCount;
  if (stream) {
    h->stream = static_cast<hipStream_t>(stream);
  } else {
    SBA_TRY_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    h->own_stream = true;
  }
  guard.h = nullptr;
  *out = h;
  return SBA_OK;
}

int sba_landmarks_destroy(sba_landmarks* h) {
  if (!h) return SBA_OK;
  (void)hipSetDevice(h->device);
  if (!h->poisoned && h->stream) (void)sba::stream_wait(h->stream, "destroy", &h->poisoned);
  if (h->poisoned) {
    delete h;      // host object only: hipFree and hipStreamDestroy would wait for the wedged device
    return sba::set_error(SBA_ERR_HIP, "landmark map destroyed while poisoned: its device memory and stream were leaked (a device wait "
                                       "timed out or the device faulted); the process should exit non-zero");
  }
  if (h->planes) (void)hipFree(h->planes);
  if (h->obs) (void)hipFree(h->obs);
  if (h->planes_alt) (void)hipFree(h->planes_alt);
  if (h->edit) (void)hipFree(h->edit);
  if (h->own_stream && h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
  return SBA_OK;
}

int sba_landmarks_size(const sba_landmarks* h, size_t* n) {
  if (!h || !n) return sba::set_error(SBA_ERR_INVALID_ARG, "null argument");
  *n = h->n;
  return SBA_OK;
}

int sba_landmarks_set(sba_landmarks* h, const double* xyz, const double* cov, size_t n, double cov_scale) {
  return set_common(h, xyz, cov, n, cov_scale, false);
}

int sba_landmarks_set_device(sba_landmarks* h, const void* xyz_dev, const void* cov_dev, size_t n, double cov_scale) {
  return set_common(h, xyz_dev, cov_dev, n, cov_scale, true);
}

int sba_landmarks_get(sba_landmarks* h, double* xyz, double* cov) { return get_common(h, xyz, cov, false); }

int sba_landmarks_get_device(sba_landmarks* h, void* xyz_dev, void* cov_dev) { return get_common(h, xyz_dev, cov_dev, true); }

int sba_landmarks_counts(sba_landmarks* h, uint32_t* out) {
  if (!h) return sba::set_error(SBA_ERR_INVALID_ARG, "null landmark handle");
  SBA_REFUSE_POISONED(h);
  if (h->n == 0) return SBA_OK;
  if (!out) return sba::set_error(SBA_ERR_INVALID_ARG, "null output array");
  SBA_TRY_HIP(hipSetDevice(h->device));
  SBA_TRY_HIP(hipMemcpyAsync(out, reinterpret_cast<const uint32_t*>(h->planes + 9 * h->elems), h->n * sizeof(uint32_t), hipMemcpyDeviceToHost,
                             h->stream));
  return sba::stream_wait(h->stream, "landmark counts", &h->poisoned);
}

int sba_landmarks_fuse(sba_landmarks* h, const int64_t* idx, const double* bearings, size_t m, const double rot[3], const double tran[3],
                       const sba_landmark_fuse_options* opt, sba_landmark_fuse_result* res, double* chi2_out) {
  if (!h || !rot || !tran || !opt || !res || (m > 0 && !bearings)) return sba::set_error(SBA_ERR_INVALID_ARG, "null argument");
  SBA_REFUSE_POISONED(h);
  if (const char* why = sba::resect_weight_check_sigma(opt->bearing_sigma)) return sba::set_error(SBA_ERR_INVALID_ARG, "%s", why);
  if (const char* why = sba::landmark_check_gate(opt->chi2_gate)) return sba::set_error(SBA_ERR_INVALID_ARG, "%s", why);
  if (const char* why = sba::landmark_check_pose_cov(opt->pose_cov)) return sba::set_error(SBA_ERR_INVALID_ARG, "%s", why);
  if (const char* why = sba::landmark_check_index(idx, m, h->n)) return sba::set_error(SBA_ERR_INVALID_ARG, "%s (m = %zu, n = %zu)", why, m, h->n);
  if (!finite3(rot) || !finite3(tran)) return sba::set_error(SBA_ERR_NUMERIC, "non-finite rot/tran");
  *res = sba_landmark_fuse_result{};
  if (h->n == 0 || m == 0) return SBA_OK;
  SBA_TRY_HIP(hipSetDevice(h->device));
  // counters | chi2 [elems] | bearings [elems][3] | idx [elems]: every part starts 16-byte aligned (elems is even)
  const size_t elems = h->elems, need = 32 + elems * 5 * sizeof(double);
  if (h->obs_bytes < need) {
    if (h->obs) SBA_TRY_HIP(hipFree(h->obs));
    h->obs = nullptr; h->obs_bytes = 0;
    SBA_TRY_HIP(hipMalloc(&h->obs, need));
    h->obs_bytes = need;
  }
  unsigned long long* counters = static_cast<unsigned long long*>(h->obs);
  double* chi2_dev = reinterpret_cast<double*>(counters + 4);
  double* bearings_dev = chi2_dev + elems;
  long long* idx_dev = reinterpret_cast<long long*>(bearings_dev + 3 * elems);
  static_assert(sba::LANDMARK_CLASSES == 4 && sizeof(long long) == sizeof(int64_t), "layout of the observation scratch");
  SBA_TRY_HIP(hipMemcpyAsync(bearings_dev, bearings, 3 * m * sizeof(double), hipMemcpyHostToDevice, h->stream));
  if (idx) SBA_TRY_HIP(hipMemcpyAsync(idx_dev, idx, m * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
  else if (elems > m) SBA_TRY_HIP(hipMemsetAsync(bearings_dev + 3 * m, 0, 3 * (elems - m) * sizeof(double), h->stream));   // the padding row: not seen
  sba::LandmarkFuseParams prm;
  sba::landmark_fuse_fill(h->n, m, rot, tran, opt->pose_cov, opt->bearing_sigma, opt->chi2_gate, &prm);
  const bool indexed = idx != nullptr, apply = opt->apply != 0;
  int& occ = h->occ_fuse[indexed ? 1 : 0][apply ? 1 : 0];
  if (occ == 0) {
    SBA_TRY_HIP(sba::landmarks_fuse_blocks_per_cu(indexed, apply, &occ));
    occ = std::max(1, occ);
  }
  const int grid = grid_for(h, indexed ? m : elems / 2, occ);
  SBA_TRY_HIP(sba::launch_landmarks_fuse(planes_of(h), prm, indexed ? idx_dev : nullptr, bearings_dev, chi2_out ? chi2_dev : nullptr, counters, apply,
                                         grid, h->stream));
  unsigned long long host_counts[4] = {0, 0, 0, 0};
  SBA_TRY_HIP(hipMemcpyAsync(host_counts, counters, sizeof(host_counts), hipMemcpyDeviceToHost, h->stream));
  if (chi2_out) SBA_TRY_HIP(hipMemcpyAsync(chi2_out, chi2_dev, m * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  const int rc = sba::stream_wait(h->stream, "landmark fusion pass", &h->poisoned);
  if (rc) return rc;
  res->n_skipped = static_cast<long long>(host_counts[sba::LANDMARK_SKIPPED]);
  res->n_behind = static_cast<long long>(host_counts[sba::LANDMARK_BEHIND]);
  res->n_gated = static_cast<long long>(host_counts[sba::LANDMARK_GATED]);
  res->n_fused = static_cast<long long>(host_counts[sba::LANDMARK_FUSED]);
  res->n_obs = res->n_skipped + res->n_behind + res->n_gated + res->n_fused;
  return SBA_OK;
}

}  // extern "C"

// ---- the edits: scores, prune, append, gather -------------------------------------------------------------------------------
namespace {

size_t up16(size_t bytes) { return (bytes + 15) / 16 * 16; }

int edit_occ(sba_landmarks* h, int which, int* occ) {
  int& o = h->occ_edit[which];
  if (o == 0) {
    SBA_TRY_HIP(sba::landmarks_edit_blocks_per_cu(which, &o));
    o = std::max(1, o);
  }
  *occ = o;
  return SBA_OK;
}

// The scratch of one edit, at least `bytes`; what it held is lost when it grows.
int edit_scratch(sba_landmarks* h, size_t bytes) {
  if (h->edit_bytes >= bytes) return SBA_OK;
  if (h->edit) SBA_TRY_HIP(hipFree(h->edit));
  h->edit = nullptr; h->edit_bytes = 0;
  SBA_TRY_HIP(hipMalloc(&h->edit, bytes));
  h->edit_bytes = bytes;
  return SBA_OK;
}

// The other plane allocation, at least `bytes`: grown only when it is too small, then by half at least.
int alt_planes(sba_landmarks* h, size_t bytes) {
  if (h->planes_alt_bytes >= bytes) return SBA_OK;
  const size_t cap = std::max(bytes, h->planes_alt_bytes + h->planes_alt_bytes / 2);
  if (h->planes_alt) SBA_TRY_HIP(hipFree(h->planes_alt));
  h->planes_alt = nullptr; h->planes_alt_bytes = 0;
  SBA_TRY_HIP(hipMalloc(reinterpret_cast<void**>(&h->planes_alt), cap));
  h->planes_alt_bytes = cap;
  return SBA_OK;
}

// The other allocation holds the map now: n landmarks at a stride of elems.
void swap_planes(sba_landmarks* h, size_t n, size_t elems) {
  std::swap(h->planes, h->planes_alt);
  std::swap(h->planes_bytes, h->planes_alt_bytes);
  h->n = n; h->elems = elems;
}

int append_common(sba_landmarks* h, const void* xyz, const void* cov, size_t n_add, double cov_scale, bool from_device) {
  if (!h) return sba::set_error(SBA_ERR_INVALID_ARG, "null landmark handle");
  SBA_REFUSE_POISONED(h);
  if (n_add > 0 && (!xyz || !cov)) return sba::set_error(SBA_ERR_INVALID_ARG, "null landmark or covariance array");
  if (from_device && ((reinterpret_cast<uintptr_t>(xyz) | reinterpret_cast<uintptr_t>(cov)) & 15u))
    return sba::set_error(SBA_ERR_INVALID_ARG, "the landmark and covariance rows must be 16-byte aligned");
  if (const char* why = sba::resect_weight_check_scale(cov_scale)) return sba::set_error(SBA_ERR_INVALID_ARG, "%s", why);
  if (const char* why = sba::landmark_check_sizes(h->n, n_add)) return sba::set_error(SBA_ERR_INVALID_ARG, "%s (n = %zu, n_add = %zu)", why, h->n, n_add);
  if (n_add == 0) return SBA_OK;
  SBA_TRY_HIP(hipSetDevice(h->device));
  const size_t n_new = h->n + n_add, elems_new = (n_new + 1) / 2 * 2;
  int rc = alt_planes(h, planes_size(elems_new));
  if (rc) return rc;
  const double *xyz_dev = static_cast<const double*>(xyz), *cov_dev = static_cast<const double*>(cov);
  if (!from_device) {            // covariance rows first: 48 n_add bytes keep the landmark rows 16-byte aligned
    rc = edit_scratch(h, 9 * n_add * sizeof(double));
    if (rc) return rc;
    double* s = static_cast<double*>(h->edit);
    SBA_TRY_HIP(hipMemcpyAsync(s, cov, 6 * n_add * sizeof(double), hipMemcpyHostToDevice, h->stream));
    SBA_TRY_HIP(hipMemcpyAsync(s + 6 * n_add, xyz, 3 * n_add * sizeof(double), hipMemcpyHostToDevice, h->stream));
    cov_dev = s; xyz_dev = s + 6 * n_add;
  }
  int occ = 1;
  rc = edit_occ(h, sba::LANDMARK_EDIT_APPEND, &occ);
  if (rc) return rc;
  SBA_TRY_HIP(sba::launch_landmarks_append(planes_of(h), h->n, xyz_dev, cov_dev, n_add, cov_scale, sba::LandmarkPlanes{h->planes_alt, elems_new},
                                           grid_for(h, elems_new / 2, occ), h->stream));
  rc = sba::stream_wait(h->stream, "landmark append", &h->poisoned);
  if (rc) return rc;
  swap_planes(h, n_new, elems_new);
  return SBA_OK;
}

int gather_common(sba_landmarks* h, const int64_t* idx, size_t m, void* xyz, void* cov, uint32_t* counts, bool to_device) {
  if (!h) return sba::set_error(SBA_ERR_INVALID_ARG, "null landmark handle");
  SBA_REFUSE_POISONED(h);
  if (to_device && ((reinterpret_cast<uintptr_t>(xyz) | reinterpret_cast<uintptr_t>(cov)) & 15u))
    return sba::set_error(SBA_ERR_INVALID_ARG, "the landmark and covariance rows must be 16-byte aligned");
  if (const char* why = sba::landmark_check_sizes(0, m)) return sba::set_error(SBA_ERR_INVALID_ARG, "%s (m = %zu)", why, m);
  if (const char* why = sba::landmark_check_gather_index(idx, m, h->n)) return sba::set_error(SBA_ERR_INVALID_ARG, "%s (m = %zu, n = %zu)", why, m, h->n);
  if (m == 0 || (!xyz && !cov && !counts)) return SBA_OK;
  SBA_TRY_HIP(hipSetDevice(h->device));
  // idx [m] | cov [m][6] | xyz [m][3] | counts [m]: the rows only when they go to the host
  int rc = edit_scratch(h, m * sizeof(int64_t) + (to_device ? 0 : 9 * m * sizeof(double) + m * sizeof(uint32_t)));
  if (rc) return rc;
  static_assert(sizeof(long long) == sizeof(int64_t), "layout of the gather scratch");
  long long* idx_dev = static_cast<long long*>(h->edit);
  double *cov_dev = static_cast<double*>(cov), *xyz_dev = static_cast<double*>(xyz);
  uint32_t* counts_dev = nullptr;
  if (!to_device) {
    double* s = reinterpret_cast<double*>(idx_dev + m);
    cov_dev = cov ? s : nullptr;
    xyz_dev = xyz ? s + 6 * m : nullptr;
    counts_dev = counts ? reinterpret_cast<uint32_t*>(s + 9 * m) : nullptr;
  }
  SBA_TRY_HIP(hipMemcpyAsync(idx_dev, idx, m * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
  int occ = 1;
  rc = edit_occ(h, sba::LANDMARK_EDIT_GATHER, &occ);
  if (rc) return rc;
  SBA_TRY_HIP(sba::launch_landmarks_gather(planes_of(h), idx_dev, m, xyz_dev, cov_dev, counts_dev, grid_for(h, m, occ), h->stream));
  if (!to_device) {
    if (cov) SBA_TRY_HIP(hipMemcpyAsync(cov, cov_dev, 6 * m * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (xyz) SBA_TRY_HIP(hipMemcpyAsync(xyz, xyz_dev, 3 * m * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (counts) SBA_TRY_HIP(hipMemcpyAsync(counts, counts_dev, m * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  }
  return sba::stream_wait(h->stream, "landmark gather", &h->poisoned);
}

}  // namespace

extern "C" {

int sba_landmarks_scores(sba_landmarks* h, double* out) {
  if (!h) return sba::set_error(SBA_ERR_INVALID_ARG, "null landmark handle");
  SBA_REFUSE_POISONED(h);
  if (h->n == 0) return SBA_OK;
  if (!out) return sba::set_error(SBA_ERR_INVALID_ARG, "null output array");
  SBA_TRY_HIP(hipSetDevice(h->device));
  int rc = edit_scratch(h, h->elems * sizeof(double));
  if (rc) return rc;
  int occ = 1;
  rc = edit_occ(h, sba::LANDMARK_EDIT_SCORES, &occ);
  if (rc) return rc;
  double* scores_dev = static_cast<double*>(h->edit);
  SBA_TRY_HIP(sba::launch_landmarks_scores(planes_of(h), scores_dev, grid_for(h, h->elems / 2, occ), h->stream));
  SBA_TRY_HIP(hipMemcpyAsync(out, scores_dev, h->n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  return sba::stream_wait(h->stream, "landmark scores", &h->poisoned);
}

int sba_landmarks_prune(sba_landmarks* h, const sba_landmark_prune_options* opt, sba_landmark_prune_result* res, int64_t* kept) {
  if (!h || !opt || !res) return sba::set_error(SBA_ERR_INVALID_ARG, "null argument");
  SBA_REFUSE_POISONED(h);
  if (const char* why = sba::landmark_check_max_score(opt->max_score)) return sba::set_error(SBA_ERR_INVALID_ARG, "%s", why);
  *res = sba_landmark_prune_result{};
  res->n_before = static_cast<long long>(h->n);
  if (h->n == 0) return SBA_OK;
  SBA_TRY_HIP(hipSetDevice(h->device));
  // class count rows, total | tile offsets [ntiles] | kept indices [n] | tile counts [ntiles] | keep bytes | mask bytes: whole
  // tiles of bytes, every part 16-byte aligned
  const size_t n = h->n, ntiles = (n + sba::kCompactTile - 1) / sba::kCompactTile, tile_bytes = ntiles * sba::kCompactTile;
  constexpr size_t kCounterWords = static_cast<size_t>(sba::kLandmarkCounterRows) * sba::kLandmarkCounterStride;
  const size_t o_offset = up16((kCounterWords + 1) * sizeof(unsigned long long));
  const size_t o_kept = o_offset + up16(ntiles * sizeof(unsigned long long)), o_count = o_kept + up16(n * sizeof(long long));
  const size_t o_keep = o_count + up16(ntiles * sizeof(unsigned int)), o_mask = o_keep + tile_bytes;
  int rc = edit_scratch(h, o_mask + tile_bytes);
  if (rc) return rc;
  char* s = static_cast<char*>(h->edit);
  unsigned long long *counters = reinterpret_cast<unsigned long long*>(s), *total = counters + kCounterWords;
  unsigned long long* tile_offset = reinterpret_cast<unsigned long long*>(s + o_offset);
  long long* kept_dev = reinterpret_cast<long long*>(s + o_kept);
  unsigned int* tile_count = reinterpret_cast<unsigned int*>(s + o_count);
  unsigned char *keep_dev = reinterpret_cast<unsigned char*>(s + o_keep), *mask_dev = reinterpret_cast<unsigned char*>(s + o_mask);
  static_assert(sizeof(long long) == sizeof(int64_t), "layout of the prune scratch");
  if (opt->mask) SBA_TRY_HIP(hipMemcpyAsync(mask_dev, opt->mask, n, hipMemcpyHostToDevice, h->stream));
  int occ = 1;
  rc = edit_occ(h, sba::LANDMARK_EDIT_KEEP, &occ);
  if (rc) return rc;
  SBA_TRY_HIP(sba::launch_landmarks_keep(planes_of(h), n, opt->max_score, opt->min_count, opt->mask ? mask_dev : nullptr, keep_dev, ntiles, counters,
                                         grid_for(h, tile_bytes / 2, occ), h->stream));
  const bool apply = opt->apply != 0, scan = apply || kept != nullptr;
  if (scan) {
    SBA_TRY_HIP(sba::launch_compact_count(keep_dev, ntiles, tile_count, h->stream));
    SBA_TRY_HIP(sba::launch_compact_scan(tile_count, ntiles, tile_offset, total, h->stream));
  }
  unsigned long long host_rows[kCounterWords + 1] = {0};
  SBA_TRY_HIP(hipMemcpyAsync(host_rows, counters, (kCounterWords + (scan ? 1 : 0)) * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
  rc = sba::stream_wait(h->stream, "landmark keep pass", &h->poisoned);   // the one wait in the middle: the new layout is sized by the kept count
  if (rc) return rc;
  unsigned long long host_counts[sba::LANDMARK_PRUNE_CLASSES + 1] = {0, 0, 0, 0, 0, host_rows[kCounterWords]};   // integer sums: any order
  for (int r = 0; r < sba::kLandmarkCounterRows; ++r)
    for (int k = 0; k < sba::LANDMARK_PRUNE_CLASSES; ++k) host_counts[k] += host_rows[static_cast<size_t>(r) * sba::kLandmarkCounterStride + k];
  const size_t n_kept = static_cast<size_t>(host_counts[sba::LANDMARK_KEPT]);
  if (scan && host_counts[sba::LANDMARK_PRUNE_CLASSES] != n_kept)
    return sba::set_error(SBA_ERR_NUMERIC, "the keep pass kept %zu landmarks, the compaction %llu", n_kept, host_counts[sba::LANDMARK_PRUNE_CLASSES]);
  res->n_invalid = static_cast<long long>(host_counts[sba::LANDMARK_INVALID]);
  res->n_uncertain = static_cast<long long>(host_counts[sba::LANDMARK_UNCERTAIN]);
  res->n_unobserved = static_cast<long long>(host_counts[sba::LANDMARK_UNOBSERVED]);
  res->n_masked = static_cast<long long>(host_counts[sba::LANDMARK_MASKED]);
  res->n_kept = static_cast<long long>(n_kept);
  if (!scan) return SBA_OK;
  if (n_kept == 0) {             // an empty map, as set leaves it
    if (apply) { h->n = 0; h->elems = 0; }
    return SBA_OK;
  }
  const size_t elems_new = (n_kept + 1) / 2 * 2;
  sba::LandmarkPlanes dst{nullptr, 0};
  if (apply) {
    rc = alt_planes(h, planes_size(elems_new));
    if (rc) return rc;
    dst = sba::LandmarkPlanes{h->planes_alt, elems_new};
  }
  SBA_TRY_HIP(sba::launch_landmarks_compact_scatter(keep_dev, n, tile_offset, ntiles, planes_of(h), dst, n_kept, kept ? kept_dev : nullptr, h->stream));
  if (kept) SBA_TRY_HIP(hipMemcpyAsync(kept, kept_dev, n_kept * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
  rc = sba::stream_wait(h->stream, "landmark compaction", &h->poisoned);
  if (rc) return rc;
  if (apply) swap_planes(h, n_kept, elems_new);
  return SBA_OK;
}

int sba_landmarks_append(sba_landmarks* h, const double* xyz, const double* cov, size_t n_add, double cov_scale) {
  return append_common(h, xyz, cov, n_add, cov_scale, false);
}

int sba_landmarks_append_device(sba_landmarks* h, const void* xyz_dev, const void* cov_dev, size_t n_add, double cov_scale) {
  return append_common(h, xyz_dev, cov_dev, n_add, cov_scale, true);
}

int sba_landmarks_gather(sba_landmarks* h, const int64_t* idx, size_t m, double* xyz, double* cov, uint32_t* counts) {
  return gather_common(h, idx, m, xyz, cov, counts, false);
}

int sba_landmarks_gather_device(sba_landmarks* h, const int64_t* idx, size_t m, void* xyz_dev, void* cov_dev) {
  return gather_common(h, idx, m, xyz_dev, cov_dev, nullptr, true);
}

}  // extern "C"
