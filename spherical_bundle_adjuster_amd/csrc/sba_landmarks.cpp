// Entry points of the landmark map (include/sba_hip.h: sba_landmarks_*): a handle of its own that keeps n landmarks with their
// 3 x 3 covariances and observation counts on the device as planes, and fuses a registered frame's bearings into them, one
// streaming pass per frame.  Kernels: sba_landmarks.hip; the per-observation code, the state of a pass and the option and
// index checks: sba_landmarks.hpp.  Every wait is the bounded stream_wait; a handle whose wait gave up is poisoned.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>

#include "sba_internal.hpp"
#include "sba_landmarks.hpp"

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
