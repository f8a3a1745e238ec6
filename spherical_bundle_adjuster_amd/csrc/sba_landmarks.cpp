// Entry points of the landmark map (include/sba_hip.h: sba_landmarks_*): a handle of its own that keeps n landmarks with their
// 3 x 3 covariances and observation counts on the device as planes, and fuses a registered frame's bearings into them, one
// streaming pass per frame.  Kernels: sba_landmarks.hip; the per-observation code, the state of a pass and the option and
// index checks: sba_landmarks.hpp.  Below them the edits of the map -- scores, prune, append, gather -- with their kernels in
// sba_landmarks_edit.hip and their checks in sba_landmarks_edit.hpp, and at the end the joint registration of a frame -- its pose
// and its landmarks solved together -- with its kernels in sba_landmarks_register.hip and its per-observation code in
// sba_landmarks_register.hpp, then its robust form (sba_landmarks_register_robust.hpp, sba_landmarks_register_robust.hip) and
// last that form under Hampel's redescending loss (sba_landmarks_register_hampel.hpp, sba_landmarks_register_hampel.hip).  Behind
// them the map's descriptor rows and the association of a frame with the map (sba_landmarks_associate.hpp,
// sba_landmarks_associate.hip); the edits above keep those rows in step with the planes.
// Every wait is the bounded stream_wait; a handle whose wait gave up is poisoned.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "sba_internal.hpp"
#include "sba_landmarks.hpp"
#include "sba_landmarks_associate.hpp"
#include "sba_landmarks_edit.hpp"
#include "sba_landmarks_register.hpp"
#include "sba_landmarks_register_robust.hpp"
#include "sba_landmarks_register_hampel.hpp"
#include "sba_lm.hpp"
#include "sba_match.hpp"

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
  // The joint registration (at the end of this file): the freeze's 4 class counters, the reduce pass's folded row and its block
  // rows [grid][JOINT_ROW], kept across calls.  The noise plane lives behind idx in the observation scratch.
  void* reg = nullptr;
  size_t reg_bytes = 0;
  int occ_reg[sba::LANDMARK_REGISTER_KERNELS][2][2] = {{{0, 0}, {0, 0}}, {{0, 0}, {0, 0}}, {{0, 0}, {0, 0}}};   // per [kernel][indexed][apply]
  int occ_reg_robust[2] = {0, 0};          // ... of landmarks_register_robust_reduce_kernel per [indexed]
  int occ_reg_hampel[2] = {0, 0};          // ... of landmarks_register_hampel_reduce_kernel per [indexed]
  // The descriptors (at the end of this file): one packed f32 row of desc_dim floats per landmark, desc_dim = 0 while the map keeps
  // none.  A prune and an append write the other allocation and swap the two, as the planes do.  assoc: the scratch of one
  // association, kept across calls.  A map that never receives descriptors allocates none of the three.
  float* desc = nullptr;
  size_t desc_bytes = 0;
  float* desc_alt = nullptr;
  size_t desc_alt_bytes = 0;
  int desc_dim = 0;
  void* assoc = nullptr;
  size_t assoc_bytes = 0;
  int occ_assoc[sba::LANDMARK_ASSOC_KERNELS] = {0, 0, 0};
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

// Resident blocks per CU of a kernel, asked once per handle and kernel: *slot is 0 while unknown, at least 1 afterwards.
template <typename Query>
int cached_occ(int* slot, Query query, int* occ) {
  if (*slot == 0) {
    SBA_TRY_HIP(query(slot));
    *slot = std::max(1, *slot);
  }
  *occ = *slot;
  return SBA_OK;
}
int pack_occ(sba_landmarks* h, bool unpack, int* occ) {
  return cached_occ(&h->occ_pack[unpack ? 1 : 0], [&](int* o) { return sba::landmarks_pack_blocks_per_cu(unpack, o); }, occ);
}
int fuse_occ(sba_landmarks* h, bool indexed, bool apply, int* occ) {
  return cached_occ(&h->occ_fuse[indexed ? 1 : 0][apply ? 1 : 0], [&](int* o) { return sba::landmarks_fuse_blocks_per_cu(indexed, apply, o); }, occ);
}
int edit_occ(sba_landmarks* h, int which, int* occ) {
  return cached_occ(&h->occ_edit[which], [&](int* o) { return sba::landmarks_edit_blocks_per_cu(which, o); }, occ);
}
int register_occ(sba_landmarks* h, int which, bool indexed, bool apply, int* occ) {
  return cached_occ(&h->occ_reg[which][indexed ? 1 : 0][apply ? 1 : 0],
                    [&](int* o) { return sba::landmarks_register_blocks_per_cu(which, indexed, apply, o); }, occ);
}
int register_robust_occ(sba_landmarks* h, bool indexed, int* occ) {
  return cached_occ(&h->occ_reg_robust[indexed ? 1 : 0], [&](int* o) { return sba::landmarks_register_robust_blocks_per_cu(indexed, o); }, occ);
}

// Grow-only device scratch of a handle: at least `need` bytes behind *ptr afterwards.  What it held is lost when it grows.
// growth_den = 0: it grows exactly to `need`; d > 0: by 1 / d of its old size at least (an allocation that is outgrown again and
// again; 2 = by half).
template <typename T>
int grow_scratch(T** ptr, size_t* bytes, size_t need, size_t growth_den = 0) {
  if (*bytes >= need) return SBA_OK;
  const size_t cap = growth_den ? std::max(need, *bytes + *bytes / growth_den) : need;
  if (*ptr) SBA_TRY_HIP(hipFree(*ptr));
  *ptr = nullptr; *bytes = 0;
  SBA_TRY_HIP(hipMalloc(reinterpret_cast<void**>(ptr), cap));
  *bytes = cap;
  return SBA_OK;
}

bool finite3(const double* a) { return std::isfinite(a[0]) && std::isfinite(a[1]) && std::isfinite(a[2]); }

// Rows on the device are moved in place as 16-byte vectors; rows on the host are staged and may lie anywhere.
bool rows_unaligned(bool on_device, const void* xyz, const void* cov) {
  return on_device && ((reinterpret_cast<uintptr_t>(xyz) | reinterpret_cast<uintptr_t>(cov)) & 15u) != 0;
}

// n caller rows between the host and 9 n doubles of device staging `s`: covariance rows first, 48 n bytes keep the landmark rows
// 16-byte aligned.  Down: the arrays that are asked for.
int stage_rows_up(sba_landmarks* h, double* s, const void* xyz, const void* cov, size_t n) {
  SBA_TRY_HIP(hipMemcpyAsync(s, cov, 6 * n * sizeof(double), hipMemcpyHostToDevice, h->stream));
  SBA_TRY_HIP(hipMemcpyAsync(s + 6 * n, xyz, 3 * n * sizeof(double), hipMemcpyHostToDevice, h->stream));
  return SBA_OK;
}
int stage_rows_down(sba_landmarks* h, const double* s, size_t n, void* xyz, void* cov) {
  if (cov) SBA_TRY_HIP(hipMemcpyAsync(cov, s, 6 * n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (xyz) SBA_TRY_HIP(hipMemcpyAsync(xyz, s + 6 * n, 3 * n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  return SBA_OK;
}

// The observations of one pass on the device (h->obs, kept across calls):
//   counters (LANDMARK_CLASSES words) | chi2 [elems] | bearings [elems][3] | idx [elems] | noise [elems] (the registration only)
// Every part starts 16-byte aligned (elems is even).
struct ObsScratch {
  unsigned long long* counters = nullptr;
  double *chi2 = nullptr, *bearings = nullptr;
  long long* idx = nullptr;
  double* noise = nullptr;
};
constexpr size_t kCounterBytes = sba::LANDMARK_CLASSES * sizeof(unsigned long long);
static_assert(kCounterBytes % 16 == 0 && sizeof(long long) == sizeof(int64_t), "layout of the observation scratch");

int obs_scratch(sba_landmarks* h, bool with_noise, ObsScratch* s) {
  const size_t elems = h->elems;
  const int rc = grow_scratch(&h->obs, &h->obs_bytes, kCounterBytes + elems * (with_noise ? 6 : 5) * sizeof(double));
  if (rc) return rc;
  s->counters = static_cast<unsigned long long*>(h->obs);
  s->chi2 = reinterpret_cast<double*>(s->counters + sba::LANDMARK_CLASSES);
  s->bearings = s->chi2 + elems;
  s->idx = reinterpret_cast<long long*>(s->bearings + 3 * elems);
  s->noise = with_noise ? reinterpret_cast<double*>(s->idx + elems) : nullptr;
  return SBA_OK;
}

// m bearings and, in the indexed form, their idx into the scratch.  The dense form's padding row is zeroed: loaded, not seen.
int upload_observations(sba_landmarks* h, const ObsScratch& s, const int64_t* idx, const double* bearings, size_t m) {
  SBA_TRY_HIP(hipMemcpyAsync(s.bearings, bearings, 3 * m * sizeof(double), hipMemcpyHostToDevice, h->stream));
  if (idx) SBA_TRY_HIP(hipMemcpyAsync(s.idx, idx, m * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
  else if (h->elems > m) SBA_TRY_HIP(hipMemsetAsync(s.bearings + 3 * m, 0, 3 * (h->elems - m) * sizeof(double), h->stream));
  return SBA_OK;
}

// The class counts of a fusion pass or of a registration's write-back into the result's fields.
template <typename Result>
void counts_to_result(const unsigned long long* c, Result* res) {
  res->n_skipped = static_cast<long long>(c[sba::LANDMARK_SKIPPED]);
  res->n_behind = static_cast<long long>(c[sba::LANDMARK_BEHIND]);
  res->n_gated = static_cast<long long>(c[sba::LANDMARK_GATED]);
  res->n_fused = static_cast<long long>(c[sba::LANDMARK_FUSED]);
  res->n_obs = res->n_skipped + res->n_behind + res->n_gated + res->n_fused;
}

int set_common(sba_landmarks* h, const void* xyz, const void* cov, size_t n, double cov_scale, bool from_device) {
  if (!h) return sba::set_error(SBA_ERR_INVALID_ARG, "null landmark handle");
  SBA_REFUSE_POISONED(h);
  if (n > 0 && (!xyz || !cov)) return sba::set_error(SBA_ERR_INVALID_ARG, "null landmark or covariance array");
  if (rows_unaligned(from_device, xyz, cov)) return sba::set_error(SBA_ERR_INVALID_ARG, "the landmark and covariance rows must be 16-byte aligned");
  if (const char* why = sba::resect_weight_check_scale(cov_scale)) return sba::set_error(SBA_ERR_INVALID_ARG, "%s", why);
  SBA_TRY_HIP(hipSetDevice(h->device));
  const size_t elems = (n + 1) / 2 * 2;
  h->n = 0; h->elems = 0;        // the map is replaced: empty until the new rows are in place
  h->desc_dim = 0;               // ... and its descriptors go with it
  if (n == 0) return SBA_OK;
  int rc = grow_scratch(&h->planes, &h->planes_bytes, planes_size(elems));
  if (rc) return rc;
  sba::DeviceBuffer staging(&h->poisoned);
  const double *xyz_dev = static_cast<const double*>(xyz), *cov_dev = static_cast<const double*>(cov);
  if (!from_device) {
    SBA_TRY_HIP(staging.alloc(9 * n * sizeof(double)));
    rc = stage_rows_up(h, staging.as<double>(), xyz, cov, n);
    if (rc) return rc;
    cov_dev = staging.as<double>(); xyz_dev = cov_dev + 6 * n;
  }
  int occ = 1;
  rc = pack_occ(h, false, &occ);
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
  if (rows_unaligned(to_device, xyz, cov)) return sba::set_error(SBA_ERR_INVALID_ARG, "the landmark and covariance rows must be 16-byte aligned");
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
  rc = stage_rows_down(h, s, n, xyz, cov);
  if (rc) return rc;
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
  if (h->reg) (void)hipFree(h->reg);
  if (h->desc) (void)hipFree(h->desc);
  if (h->desc_alt) (void)hipFree(h->desc_alt);
  if (h->assoc) (void)hipFree(h->assoc);
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
  ObsScratch obs;
  int rc = obs_scratch(h, false, &obs);
  if (rc) return rc;
  rc = upload_observations(h, obs, idx, bearings, m);
  if (rc) return rc;
  sba::LandmarkFuseParams prm;
  sba::landmark_fuse_fill(h->n, m, rot, tran, opt->pose_cov, opt->bearing_sigma, opt->chi2_gate, &prm);
  const bool indexed = idx != nullptr, apply = opt->apply != 0;
  int occ = 1;
  rc = fuse_occ(h, indexed, apply, &occ);
  if (rc) return rc;
  const int grid = grid_for(h, indexed ? m : h->elems / 2, occ);
  SBA_TRY_HIP(sba::launch_landmarks_fuse(planes_of(h), prm, indexed ? obs.idx : nullptr, obs.bearings, chi2_out ? obs.chi2 : nullptr, obs.counters, apply,
                                         grid, h->stream));
  unsigned long long host_counts[sba::LANDMARK_CLASSES] = {0, 0, 0, 0};
  SBA_TRY_HIP(hipMemcpyAsync(host_counts, obs.counters, sizeof(host_counts), hipMemcpyDeviceToHost, h->stream));
  if (chi2_out) SBA_TRY_HIP(hipMemcpyAsync(chi2_out, obs.chi2, m * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  rc = sba::stream_wait(h->stream, "landmark fusion pass", &h->poisoned);
  if (rc) return rc;
  counts_to_result(host_counts, res);
  return SBA_OK;
}

}  // extern "C"

// ---- the edits: scores, prune, append, gather -------------------------------------------------------------------------------
namespace {

size_t up16(size_t bytes) { return (bytes + 15) / 16 * 16; }

// The scratch of one edit, at least `bytes`.
int edit_scratch(sba_landmarks* h, size_t bytes) { return grow_scratch(&h->edit, &h->edit_bytes, bytes); }

// The other plane allocation, at least `bytes`: grown only when it is too small, then by half at least.
int alt_planes(sba_landmarks* h, size_t bytes) { return grow_scratch(&h->planes_alt, &h->planes_alt_bytes, bytes, 2); }

// The other allocation holds the map now: n landmarks at a stride of elems.
void swap_planes(sba_landmarks* h, size_t n, size_t elems) {
  std::swap(h->planes, h->planes_alt);
  std::swap(h->planes_bytes, h->planes_alt_bytes);
  h->n = n; h->elems = elems;
}

// The descriptors through an edit.  The other descriptor allocation, at least `rows` rows of `dim` floats, grown as alt_planes grows.
int alt_desc(sba_landmarks* h, size_t rows, int dim) {
  return grow_scratch(&h->desc_alt, &h->desc_alt_bytes, std::max<size_t>(rows, 1) * static_cast<size_t>(dim) * sizeof(float), 2);
}

// The other descriptor allocation holds the map's rows now.
void swap_desc(sba_landmarks* h, int dim) {
  std::swap(h->desc, h->desc_alt);
  std::swap(h->desc_bytes, h->desc_alt_bytes);
  h->desc_dim = dim;
}

// n_rows caller rows of `dim` floats at a stride of stride_bytes into packed rows on the device, on the handle's stream.
int pack_desc_rows(sba_landmarks* h, float* dst, const void* rows, size_t n_rows, int dim, size_t stride_bytes, bool from_device) {
  const size_t width = static_cast<size_t>(dim) * sizeof(float);
  SBA_TRY_HIP(hipMemcpy2DAsync(dst, width, rows, stride_bytes, width, n_rows, from_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
  return SBA_OK;
}

// The descriptor rows of an append into the other allocation: the map's own rows, then the caller's n_add rows or, when the
// caller has none (desc == null), rows that are all NaN -- a train row the matcher never chooses.
int append_desc_rows(sba_landmarks* h, int dim, const void* desc, size_t n_add, size_t stride_bytes, bool from_device) {
  const size_t n_old = h->n, row = static_cast<size_t>(dim);
  int rc = alt_desc(h, n_old + n_add, dim);
  if (rc) return rc;
  if (n_old) SBA_TRY_HIP(hipMemcpyAsync(h->desc_alt, h->desc, n_old * row * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
  float* added = h->desc_alt + n_old * row;
  if (desc) return pack_desc_rows(h, added, desc, n_add, dim, stride_bytes, from_device);
  SBA_TRY_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(added), 0x7fc00000, n_add * row, h->stream));
  return SBA_OK;
}

// desc == null: a plain append.  Otherwise n_add descriptor rows of `dim` floats come with the landmarks (sba_landmarks_append_described).
int append_common(sba_landmarks* h, const void* xyz, const void* cov, size_t n_add, double cov_scale, bool from_device, const void* desc = nullptr,
                  int dim = 0, size_t row_stride_bytes = 0, bool described = false) {
  if (!h) return sba::set_error(SBA_ERR_INVALID_ARG, "null landmark handle");
  SBA_REFUSE_POISONED(h);
  if (n_add > 0 && (!xyz || !cov)) return sba::set_error(SBA_ERR_INVALID_ARG, "null landmark or covariance array");
  if (rows_unaligned(from_device, xyz, cov)) return sba::set_error(SBA_ERR_INVALID_ARG, "the landmark and covariance rows must be 16-byte aligned");
  if (const char* why = sba::resect_weight_check_scale(cov_scale)) return sba::set_error(SBA_ERR_INVALID_ARG, "%s", why);
  if (const char* why = sba::landmark_check_sizes(h->n, n_add)) return sba::set_error(SBA_ERR_INVALID_ARG, "%s (n = %zu, n_add = %zu)", why, h->n, n_add);
  if (described) {
    if (const char* why = sba::descriptor_check_rows(dim, row_stride_bytes))
      return sba::set_error(SBA_ERR_INVALID_ARG, "%s (dim = %d, row_stride_bytes = %zu)", why, dim, row_stride_bytes);
    if (n_add > 0 && !desc) return sba::set_error(SBA_ERR_INVALID_ARG, "null descriptor array");
    if (from_device && (reinterpret_cast<uintptr_t>(desc) & 3u) != 0) return sba::set_error(SBA_ERR_INVALID_ARG, "device descriptor rows must be 4-byte aligned");
    if (h->n > 0 && h->desc_dim != dim)
      return sba::set_error(SBA_ERR_INVALID_ARG, "the map keeps descriptors of dimension %d (0: none), the new rows have %d", h->desc_dim, dim);
    if (n_add == 0 && h->n == 0) h->desc_dim = dim;      // an empty map takes the dimension, as set + set_descriptors would
  }
  if (n_add == 0) return SBA_OK;
  SBA_TRY_HIP(hipSetDevice(h->device));
  const size_t n_new = h->n + n_add, elems_new = (n_new + 1) / 2 * 2;
  int rc = alt_planes(h, planes_size(elems_new));
  if (rc) return rc;
  const int dim_new = described ? dim : h->desc_dim;     // a plain append to a described map: NaN rows
  if (dim_new) {
    rc = append_desc_rows(h, dim_new, described ? desc : nullptr, n_add, row_stride_bytes, from_device);
    if (rc) return rc;
  }
  const double *xyz_dev = static_cast<const double*>(xyz), *cov_dev = static_cast<const double*>(cov);
  if (!from_device) {
    rc = edit_scratch(h, 9 * n_add * sizeof(double));
    if (rc) return rc;
    rc = stage_rows_up(h, static_cast<double*>(h->edit), xyz, cov, n_add);
    if (rc) return rc;
    cov_dev = static_cast<const double*>(h->edit); xyz_dev = cov_dev + 6 * n_add;
  }
  int occ = 1;
  rc = edit_occ(h, sba::LANDMARK_EDIT_APPEND, &occ);
  if (rc) return rc;
  SBA_TRY_HIP(sba::launch_landmarks_append(planes_of(h), h->n, xyz_dev, cov_dev, n_add, cov_scale, sba::LandmarkPlanes{h->planes_alt, elems_new},
                                           grid_for(h, elems_new / 2, occ), h->stream));
  rc = sba::stream_wait(h->stream, "landmark append", &h->poisoned);
  if (rc) return rc;
  swap_planes(h, n_new, elems_new);
  if (dim_new) swap_desc(h, dim_new);
  return SBA_OK;
}

int gather_common(sba_landmarks* h, const int64_t* idx, size_t m, void* xyz, void* cov, uint32_t* counts, bool to_device) {
  if (!h) return sba::set_error(SBA_ERR_INVALID_ARG, "null landmark handle");
  SBA_REFUSE_POISONED(h);
  if (rows_unaligned(to_device, xyz, cov)) return sba::set_error(SBA_ERR_INVALID_ARG, "the landmark and covariance rows must be 16-byte aligned");
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
  double* s = reinterpret_cast<double*>(idx_dev + m);      // the staged rows, when they go to the host
  if (!to_device) {
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
    rc = stage_rows_down(h, s, m, xyz, cov);
    if (rc) return rc;
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
    if (h->desc_dim) {
      rc = alt_desc(h, n_kept, h->desc_dim);
      if (rc) return rc;
    }
  }
  SBA_TRY_HIP(sba::launch_landmarks_compact_scatter(keep_dev, n, tile_offset, ntiles, planes_of(h), dst, n_kept, kept ? kept_dev : nullptr, h->stream));
  if (apply && h->desc_dim)      // the descriptor rows follow the planes: the same keep bytes, the same tile offsets
    SBA_TRY_HIP(sba::launch_landmarks_desc_compact_scatter(keep_dev, n, tile_offset, ntiles, h->desc, h->desc_alt, h->desc_dim, h->stream));
  if (kept) SBA_TRY_HIP(hipMemcpyAsync(kept, kept_dev, n_kept * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
  rc = sba::stream_wait(h->stream, "landmark compaction", &h->poisoned);
  if (rc) return rc;
  if (apply) {
    swap_planes(h, n_kept, elems_new);
    if (h->desc_dim) swap_desc(h, h->desc_dim);
  }
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

// ---- the joint registration: a frame's pose and its landmarks solved together ----------------------------------------------------
namespace {

// What one registration works on, after the refusals: the observations on the device, the frozen noise, the block rows.
struct RegisterWork {
  bool indexed = false;
  size_t m = 0;
  double bearing_sigma = 0.0;
  ObsScratch obs;                              // its counters: the apply pass's class counts
  unsigned long long* freeze_counters = nullptr;
  double *row_dev = nullptr, *partials = nullptr;
  int grid_freeze = 0, grid_reduce = 0;
  long long freeze_counts[sba::LANDMARK_CLASSES] = {0, 0, 0, 0};
};

// The refusals sba_landmarks_eval_register and sba_landmarks_register share, all before the first device call.
int register_check(sba_landmarks* h, const int64_t* idx, const double* bearings, size_t m, const double* rot, const double* tran,
                   const double* rot_ref, const double* tran_ref, const sba_landmark_register_options* opt, const void* out) {
  if (!h || !rot || !tran || !rot_ref || !tran_ref || !opt || !out || (m > 0 && !bearings)) return sba::set_error(SBA_ERR_INVALID_ARG, "null argument");
  SBA_REFUSE_POISONED(h);
  if (const char* why = sba::resect_weight_check_sigma(opt->bearing_sigma)) return sba::set_error(SBA_ERR_INVALID_ARG, "%s", why);
  if (const char* why = sba::landmark_check_gate(opt->chi2_gate)) return sba::set_error(SBA_ERR_INVALID_ARG, "%s", why);
  if (const char* why = sba::landmark_check_index(idx, m, h->n)) return sba::set_error(SBA_ERR_INVALID_ARG, "%s (m = %zu, n = %zu)", why, m, h->n);
  if (const char* why = sba::landmark_register_check_loss(opt->lm.huber_delta)) return sba::set_error(SBA_ERR_UNSUPPORTED, "%s", why);
  if (!finite3(rot) || !finite3(tran) || !finite3(rot_ref) || !finite3(tran_ref)) return sba::set_error(SBA_ERR_NUMERIC, "non-finite rot/tran");
  return SBA_OK;
}

// Upload bearings and idx as sba_landmarks_fuse does, size the scratch, freeze the noise at (rot_ref, tran_ref) and fetch the
// freeze's class counts.
int register_freeze(sba_landmarks* h, const int64_t* idx, const double* bearings, size_t m, const double rot_ref[3], const double tran_ref[3],
                    double bearing_sigma, RegisterWork* w) {
  SBA_TRY_HIP(hipSetDevice(h->device));
  const size_t elems = h->elems;
  int rc = obs_scratch(h, true, &w->obs);      // sba_landmarks_fuse's layout, then the noise plane; grow_scratch's hipMalloc: after hipSetDevice
  if (rc) return rc;
  w->indexed = idx != nullptr;
  w->m = m;
  w->bearing_sigma = bearing_sigma;
  const size_t items = w->indexed ? m : elems / 2;
  int occ = 1;
  rc = register_occ(h, sba::LANDMARK_REGISTER_FREEZE, w->indexed, false, &occ);
  if (rc) return rc;
  w->grid_freeze = grid_for(h, items, occ);
  // The reduce pass: two observations per lane in both forms and one grid rule for both (the smaller occupancy), so that the
  // indexed form over every landmark folds the dense form's block rows.
  int occ_other = 1;
  rc = register_occ(h, sba::LANDMARK_REGISTER_REDUCE, w->indexed, false, &occ);
  if (rc) return rc;
  rc = register_occ(h, sba::LANDMARK_REGISTER_REDUCE, !w->indexed, false, &occ_other);
  if (rc) return rc;
  w->grid_reduce = grid_for(h, w->indexed ? (m + 1) / 2 : elems / 2, std::min(occ, occ_other));
  // freeze counters | the folded row | block rows [grid]
  rc = grow_scratch(&h->reg, &h->reg_bytes, kCounterBytes + (static_cast<size_t>(w->grid_reduce) + 1) * sba::JOINT_ROW * sizeof(double));
  if (rc) return rc;
  w->freeze_counters = static_cast<unsigned long long*>(h->reg);
  w->row_dev = reinterpret_cast<double*>(w->freeze_counters + sba::LANDMARK_CLASSES);
  w->partials = w->row_dev + sba::JOINT_ROW;
  rc = upload_observations(h, w->obs, idx, bearings, m);
  if (rc) return rc;
  sba::LandmarkRegisterParams prm;
  sba::landmark_register_fill(h->n, m, rot_ref, tran_ref, nullptr, bearing_sigma, INFINITY, &prm);
  SBA_TRY_HIP(sba::launch_landmarks_register_freeze(planes_of(h), prm, w->indexed ? w->obs.idx : nullptr, w->obs.bearings, w->obs.noise,
                                                    w->freeze_counters, w->grid_freeze, h->stream));
  unsigned long long host_counts[sba::LANDMARK_CLASSES] = {0, 0, 0, 0};
  SBA_TRY_HIP(hipMemcpyAsync(host_counts, w->freeze_counters, sizeof(host_counts), hipMemcpyDeviceToHost, h->stream));
  rc = sba::stream_wait(h->stream, "landmark registration freeze", &h->poisoned);
  if (rc) return rc;
  for (int k = 0; k < sba::LANDMARK_CLASSES; ++k) w->freeze_counts[k] = static_cast<long long>(host_counts[k]);
  return SBA_OK;
}

// One evaluation at (rot, tran): the reduce pass, the fold, the row fetched through the bounded wait.
int register_reduce_pass(sba_landmarks* h, const RegisterWork& w, const double rot[3], const double tran[3], double* row) {
  sba::LandmarkRegisterParams prm;
  sba::landmark_register_fill(h->n, w.m, rot, tran, nullptr, w.bearing_sigma, INFINITY, &prm);
  SBA_TRY_HIP(sba::launch_landmarks_register_reduce(planes_of(h), prm, w.indexed ? w.obs.idx : nullptr, w.obs.bearings, w.obs.noise, w.partials,
                                                    w.grid_reduce, w.row_dev, h->stream));
  SBA_TRY_HIP(hipMemcpyAsync(row, w.row_dev, SBA_RESECT_COUNT * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  return sba::stream_wait(h->stream, "landmark registration reduce pass", &h->poisoned);
}

}  // namespace

extern "C" {

int sba_landmarks_eval_register(sba_landmarks* h, const int64_t* idx, const double* bearings, size_t m, const double rot[3], const double tran[3],
                                const double rot_ref[3], const double tran_ref[3], const sba_landmark_register_options* opt,
                                sba_landmark_register_eval* eval) {
  int rc = register_check(h, idx, bearings, m, rot, tran, rot_ref, tran_ref, opt, eval);
  if (rc) return rc;
  *eval = sba_landmark_register_eval{};
  if (h->n == 0 || m == 0) return SBA_OK;
  RegisterWork w;
  rc = register_freeze(h, idx, bearings, m, rot_ref, tran_ref, opt->bearing_sigma, &w);
  if (rc) return rc;
  double row[sba::JOINT_ROW] = {0};
  rc = register_reduce_pass(h, w, rot, tran, row);
  if (rc) return rc;
  if (!sba::resect_row_finite(row)) return sba::set_error(SBA_ERR_NUMERIC, "non-finite registration sums");
  sba_normal_eq ne;
  double n_behind = 0.0;
  sba::resect_expand_row(row, &ne, &n_behind);
  std::memcpy(eval->H, ne.H, sizeof(ne.H));
  std::memcpy(eval->g, ne.g, sizeof(ne.g));
  eval->cost = ne.cost;
  eval->n_used = static_cast<long long>(ne.sum_w);
  eval->n_behind = static_cast<long long>(n_behind);
  return SBA_OK;
}

int sba_landmarks_register(sba_landmarks* h, const int64_t* idx, const double* bearings, size_t m, const double rot0[3], const double tran0[3],
                           const sba_landmark_register_options* opt, sba_landmark_register_result* res, double* chi2_out) {
  int rc = register_check(h, idx, bearings, m, rot0, tran0, rot0, tran0, opt, res);
  if (rc) return rc;
  *res = sba_landmark_register_result{};
  for (int a = 0; a < 3; ++a) { res->rot[a] = rot0[a]; res->tran[a] = tran0[a]; }
  if (h->n == 0 || m == 0) return SBA_OK;
  const auto t_start = std::chrono::steady_clock::now();
  RegisterWork w;
  rc = register_freeze(h, idx, bearings, m, rot0, tran0, opt->bearing_sigma, &w);
  if (rc) return rc;
  if (w.freeze_counts[sba::LANDMARK_LIVE] < 3)
    return sba::set_error(SBA_ERR_NUMERIC, "pose not determined: %lld observations take part after the freeze (%lld skipped, %lld behind), 3 are needed",
                          w.freeze_counts[sba::LANDMARK_LIVE], w.freeze_counts[sba::LANDMARK_SKIPPED], w.freeze_counts[sba::LANDMARK_BEHIND]);
  struct Visit { double rot[3], tran[3], H[36], n_used; };
  std::vector<Visit> visits;
  double seconds_eval = 0.0;
  int eval_rc = SBA_OK;
  auto evaluate = [&](const double r[3], const double t[3], sba_normal_eq* ne) -> bool {
    const auto t0 = std::chrono::steady_clock::now();
    double row[sba::JOINT_ROW] = {0};
    eval_rc = register_reduce_pass(h, w, r, t, row);
    seconds_eval += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (eval_rc) return false;
    if (!sba::resect_row_finite(row)) return false;
    sba::resect_expand_row(row, ne, nullptr);
    Visit v;
    for (int a = 0; a < 3; ++a) { v.rot[a] = r[a]; v.tran[a] = t[a]; }
    std::memcpy(v.H, ne->H, sizeof(v.H));
    v.n_used = ne->sum_w;
    visits.push_back(v);
    return true;
  };
  double r[3] = {rot0[0], rot0[1], rot0[2]}, t[3] = {tran0[0], tran0[1], tran0[2]};
  sba_lm_summary sum;
  std::memset(&sum, 0, sizeof(sum));
  const int status = sba::lm_solve(SBA_MODE_RT, r, t, opt->lm, evaluate, &sum);
  if (eval_rc) return eval_rc;
  sum.seconds_eval = seconds_eval;
  if (status != SBA_OK) return sba::set_error(status, "joint registration solve failed: non-finite sums or 5 consecutive invalid steps");
  const Visit* at = nullptr;
  for (size_t k = visits.size(); k-- > 0;)
    if (std::memcmp(visits[k].rot, r, sizeof(r)) == 0 && std::memcmp(visits[k].tran, t, sizeof(t)) == 0) { at = &visits[k]; break; }
  double cov[36];
  if (!at || !sba::resect_cov_inverse(at->H, cov))
    return sba::set_error(SBA_ERR_NUMERIC, "pose not determined: the reduced normal matrix is not positive definite at the solution");
  // the write-back at the solution
  const bool apply = opt->apply != 0;
  int occ = 1;
  rc = register_occ(h, sba::LANDMARK_REGISTER_APPLY, w.indexed, apply, &occ);
  if (rc) return rc;
  sba::LandmarkRegisterParams prm;
  sba::landmark_register_fill(h->n, m, r, t, cov, opt->bearing_sigma, opt->chi2_gate, &prm);
  SBA_TRY_HIP(sba::launch_landmarks_register_apply(planes_of(h), prm, w.indexed ? w.obs.idx : nullptr, w.obs.bearings, w.obs.noise,
                                                   chi2_out ? w.obs.chi2 : nullptr, w.obs.counters, apply,
                                                   grid_for(h, w.indexed ? m : h->elems / 2, occ), h->stream));
  unsigned long long host_counts[sba::LANDMARK_CLASSES] = {0, 0, 0, 0};
  SBA_TRY_HIP(hipMemcpyAsync(host_counts, w.obs.counters, sizeof(host_counts), hipMemcpyDeviceToHost, h->stream));
  if (chi2_out) SBA_TRY_HIP(hipMemcpyAsync(chi2_out, w.obs.chi2, m * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  rc = sba::stream_wait(h->stream, "landmark registration write-back", &h->poisoned);
  if (rc) return rc;
  for (int a = 0; a < 3; ++a) { res->rot[a] = r[a]; res->tran[a] = t[a]; }
  std::memcpy(res->cov, cov, sizeof(cov));
  counts_to_result(host_counts, res);
  res->n_used = static_cast<long long>(at->n_used);
  sum.seconds_total = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
  res->summary = sum;
  return SBA_OK;
}

}  // extern "C"

// ---- the robust joint registration: the Huber loss on every landmark's block (sba_landmarks_register_robust.hpp) --------------------
namespace {

// The refusals of the four robust entry points, all before the first device call: register_check's with the same codes, the
// loss excepted, then the loss and the gate against delta^2.  on_device: bearings (and chi2_out) are device pointers to doubles.
int robust_check(sba_landmarks* h, const int64_t* idx, const void* bearings, size_t m, const double* rot, const double* tran, const double* rot_ref,
                 const double* tran_ref, const sba_landmark_register_options* opt, const void* out, bool on_device, const void* chi2_out) {
  if (!h || !rot || !tran || !rot_ref || !tran_ref || !opt || !out || (m > 0 && !bearings)) return sba::set_error(SBA_ERR_INVALID_ARG, "null argument");
  SBA_REFUSE_POISONED(h);
  if (const char* why = sba::resect_weight_check_sigma(opt->bearing_sigma)) return sba::set_error(SBA_ERR_INVALID_ARG, "%s", why);
  if (const char* why = sba::landmark_check_gate(opt->chi2_gate)) return sba::set_error(SBA_ERR_INVALID_ARG, "%s", why);
  if (const char* why = sba::landmark_check_index(idx, m, h->n)) return sba::set_error(SBA_ERR_INVALID_ARG, "%s (m = %zu, n = %zu)", why, m, h->n);
  if (const char* why = sba::landmark_register_check_robust(opt->lm.huber_delta, opt->chi2_gate)) return sba::set_error(SBA_ERR_INVALID_ARG, "%s", why);
  if (on_device && ((reinterpret_cast<uintptr_t>(bearings) | reinterpret_cast<uintptr_t>(chi2_out)) & 7u) != 0)
    return sba::set_error(SBA_ERR_INVALID_ARG, "device bearings and chi2_out must be 8-byte aligned");
  if (!finite3(rot) || !finite3(tran) || !finite3(rot_ref) || !finite3(tran_ref)) return sba::set_error(SBA_ERR_NUMERIC, "non-finite rot/tran");
  return SBA_OK;
}

// Whether the dense form's 16-byte vector accesses stay inside a caller's device array of m rows: an even m (no padding row)
// and a 16-byte aligned start.  The indexed form reads and writes single doubles of rows < m and always may.
bool dense_vectors_fit(const void* ptr, size_t m) { return m % 2 == 0 && (reinterpret_cast<uintptr_t>(ptr) & 15u) == 0; }

// register_freeze for the robust pass: the grid of the reduce pass follows landmarks_register_robust_reduce_kernel's two
// occupancies, and bearings may live on the device.  Device bearings are NOT copied: w->obs.bearings becomes the caller's pointer,
// which every kernel takes as an argument of its own.  The one exception is the dense form over an odd n or from a start that
// is not 16-byte aligned: its lanes load whole 16-byte vectors of two rows, the last of which would end 24 bytes behind the
// caller's array, so those rows go device-to-device into the scratch with its zeroed padding row.
int robust_freeze(sba_landmarks* h, const int64_t* idx, const double* bearings, bool on_device, size_t m, const double rot_ref[3],
                  const double tran_ref[3], double bearing_sigma, RegisterWork* w) {
  SBA_TRY_HIP(hipSetDevice(h->device));
  const size_t elems = h->elems;
  int rc = obs_scratch(h, true, &w->obs);
  if (rc) return rc;
  w->indexed = idx != nullptr;
  w->m = m;
  w->bearing_sigma = bearing_sigma;
  const size_t items = w->indexed ? m : elems / 2;
  int occ = 1, occ_other = 1;
  rc = register_occ(h, sba::LANDMARK_REGISTER_FREEZE, w->indexed, false, &occ);
  if (rc) return rc;
  w->grid_freeze = grid_for(h, items, occ);
  rc = register_robust_occ(h, w->indexed, &occ);
  if (rc) return rc;
  rc = register_robust_occ(h, !w->indexed, &occ_other);
  if (rc) return rc;
  w->grid_reduce = grid_for(h, w->indexed ? (m + 1) / 2 : elems / 2, std::min(occ, occ_other));
  rc = grow_scratch(&h->reg, &h->reg_bytes, kCounterBytes + (static_cast<size_t>(w->grid_reduce) + 1) * sba::JOINT_ROW * sizeof(double));
  if (rc) return rc;
  w->freeze_counters = static_cast<unsigned long long*>(h->reg);
  w->row_dev = reinterpret_cast<double*>(w->freeze_counters + sba::LANDMARK_CLASSES);
  w->partials = w->row_dev + sba::JOINT_ROW;
  if (!on_device) {
    rc = upload_observations(h, w->obs, idx, bearings, m);
    if (rc) return rc;
  } else if (w->indexed) {
    SBA_TRY_HIP(hipMemcpyAsync(w->obs.idx, idx, m * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
    w->obs.bearings = const_cast<double*>(bearings);
  } else if (dense_vectors_fit(bearings, m)) {
    w->obs.bearings = const_cast<double*>(bearings);
  } else {
    SBA_TRY_HIP(hipMemcpyAsync(w->obs.bearings, bearings, 3 * m * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    if (elems > m) SBA_TRY_HIP(hipMemsetAsync(w->obs.bearings + 3 * m, 0, 3 * (elems - m) * sizeof(double), h->stream));
  }
  sba::LandmarkRegisterParams prm;
  sba::landmark_register_fill(h->n, m, rot_ref, tran_ref, nullptr, bearing_sigma, INFINITY, &prm);
  SBA_TRY_HIP(sba::launch_landmarks_register_freeze(planes_of(h), prm, w->indexed ? w->obs.idx : nullptr, w->obs.bearings, w->obs.noise,
                                                    w->freeze_counters, w->grid_freeze, h->stream));
  unsigned long long host_counts[sba::LANDMARK_CLASSES] = {0, 0, 0, 0};
  SBA_TRY_HIP(hipMemcpyAsync(host_counts, w->freeze_counters, sizeof(host_counts), hipMemcpyDeviceToHost, h->stream));
  rc = sba::stream_wait(h->stream, "robust landmark registration freeze", &h->poisoned);
  if (rc) return rc;
  for (int k = 0; k < sba::LANDMARK_CLASSES; ++k) w->freeze_counts[k] = static_cast<long long>(host_counts[k]);
  return SBA_OK;
}

int robust_reduce_pass(sba_landmarks* h, const RegisterWork& w, const sba::LandmarkRegisterRobust& loss, const double rot[3], const double tran[3],
                       double* row) {
  sba::LandmarkRegisterParams prm;
  sba::landmark_register_fill(h->n, w.m, rot, tran, nullptr, w.bearing_sigma, INFINITY, &prm);
  SBA_TRY_HIP(sba::launch_landmarks_register_robust_reduce(planes_of(h), prm, loss, w.indexed ? w.obs.idx : nullptr, w.obs.bearings, w.obs.noise,
                                                           w.partials, w.grid_reduce, w.row_dev, h->stream));
  SBA_TRY_HIP(hipMemcpyAsync(row, w.row_dev, SBA_RESECT_COUNT * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  return sba::stream_wait(h->stream, "robust landmark registration reduce pass", &h->poisoned);
}

int eval_register_robust_common(sba_landmarks* h, const int64_t* idx, const double* bearings, bool on_device, size_t m, const double rot[3],
                                const double tran[3], const double rot_ref[3], const double tran_ref[3], const sba_landmark_register_options* opt,
                                sba_landmark_register_robust_eval* eval) {
  int rc = robust_check(h, idx, bearings, m, rot, tran, rot_ref, tran_ref, opt, eval, on_device, nullptr);
  if (rc) return rc;
  *eval = sba_landmark_register_robust_eval{};
  if (h->n == 0 || m == 0) return SBA_OK;
  RegisterWork w;
  rc = robust_freeze(h, idx, bearings, on_device, m, rot_ref, tran_ref, opt->bearing_sigma, &w);
  if (rc) return rc;
  sba::LandmarkRegisterRobust loss;
  sba::landmark_register_robust_fill(opt->lm.huber_delta, &loss);
  double row[sba::JOINT_ROW] = {0};
  rc = robust_reduce_pass(h, w, loss, rot, tran, row);
  if (rc) return rc;
  if (!sba::resect_row_finite(row)) return sba::set_error(SBA_ERR_NUMERIC, "non-finite registration sums");
  sba_normal_eq ne;
  double n_behind = 0.0;
  sba::resect_expand_row(row, &ne, &n_behind);
  std::memcpy(eval->H, ne.H, sizeof(ne.H));
  std::memcpy(eval->g, ne.g, sizeof(ne.g));
  eval->cost = ne.cost;
  eval->n_used = static_cast<long long>(ne.sum_w);
  eval->n_behind = static_cast<long long>(n_behind);
  eval->n_outlier = static_cast<long long>(ne.n_outlier);
  return SBA_OK;
}

int register_robust_common(sba_landmarks* h, const int64_t* idx, const double* bearings, bool on_device, size_t m, const double rot0[3],
                           const double tran0[3], const sba_landmark_register_options* opt, sba_landmark_register_robust_result* res,
                           double* chi2_out) {
  int rc = robust_check(h, idx, bearings, m, rot0, tran0, rot0, tran0, opt, res, on_device, chi2_out);
  if (rc) return rc;
  *res = sba_landmark_register_robust_result{};
  for (int a = 0; a < 3; ++a) { res->rot[a] = rot0[a]; res->tran[a] = tran0[a]; }
  if (h->n == 0 || m == 0) return SBA_OK;
  const auto t_start = std::chrono::steady_clock::now();
  RegisterWork w;
  rc = robust_freeze(h, idx, bearings, on_device, m, rot0, tran0, opt->bearing_sigma, &w);
  if (rc) return rc;
  if (w.freeze_counts[sba::LANDMARK_LIVE] < 3)
    return sba::set_error(SBA_ERR_NUMERIC, "pose not determined: %lld observations take part after the freeze (%lld skipped, %lld behind), 3 are needed",
                          w.freeze_counts[sba::LANDMARK_LIVE], w.freeze_counts[sba::LANDMARK_SKIPPED], w.freeze_counts[sba::LANDMARK_BEHIND]);
  sba::LandmarkRegisterRobust loss;
  sba::landmark_register_robust_fill(opt->lm.huber_delta, &loss);
  struct Visit { double rot[3], tran[3], H[36], n_used, n_outlier; };
  std::vector<Visit> visits;
  double seconds_eval = 0.0;
  int eval_rc = SBA_OK;
  auto evaluate = [&](const double r[3], const double t[3], sba_normal_eq* ne) -> bool {
    const auto t0 = std::chrono::steady_clock::now();
    double row[sba::JOINT_ROW] = {0};
    eval_rc = robust_reduce_pass(h, w, loss, r, t, row);
    seconds_eval += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (eval_rc) return false;
    if (!sba::resect_row_finite(row)) return false;
    sba::resect_expand_row(row, ne, nullptr);
    Visit v;
    for (int a = 0; a < 3; ++a) { v.rot[a] = r[a]; v.tran[a] = t[a]; }
    std::memcpy(v.H, ne->H, sizeof(v.H));
    v.n_used = ne->sum_w;
    v.n_outlier = ne->n_outlier;
    visits.push_back(v);
    return true;
  };
  double r[3] = {rot0[0], rot0[1], rot0[2]}, t[3] = {tran0[0], tran0[1], tran0[2]};
  sba_lm_summary sum;
  std::memset(&sum, 0, sizeof(sum));
  const int status = sba::lm_solve(SBA_MODE_RT, r, t, opt->lm, evaluate, &sum);
  if (eval_rc) return eval_rc;
  sum.seconds_eval = seconds_eval;
  if (status != SBA_OK) return sba::set_error(status, "robust joint registration solve failed: non-finite sums or 5 consecutive invalid steps");
  const Visit* at = nullptr;
  for (size_t k = visits.size(); k-- > 0;)
    if (std::memcmp(visits[k].rot, r, sizeof(r)) == 0 && std::memcmp(visits[k].tran, t, sizeof(t)) == 0) { at = &visits[k]; break; }
  double cov[36];
  if (!at || !sba::resect_cov_inverse(at->H, cov))
    return sba::set_error(SBA_ERR_NUMERIC, "pose not determined: the reduced normal matrix is not positive definite at the solution");
  // the write-back at the solution: sba_landmarks_register's, with Sigma_c = H_rho^-1
  const bool apply = opt->apply != 0;
  int occ = 1;
  rc = register_occ(h, sba::LANDMARK_REGISTER_APPLY, w.indexed, apply, &occ);
  if (rc) return rc;
  // chi2 on the device goes straight to the caller where the pass's stores fit (dense_vectors_fit), else through the scratch
  const bool chi2_direct = on_device && chi2_out && (w.indexed || dense_vectors_fit(chi2_out, m));
  double* chi2_dev = !chi2_out ? nullptr : (chi2_direct ? chi2_out : w.obs.chi2);
  sba::LandmarkRegisterParams prm;
  sba::landmark_register_fill(h->n, m, r, t, cov, opt->bearing_sigma, opt->chi2_gate, &prm);
  SBA_TRY_HIP(sba::launch_landmarks_register_apply(planes_of(h), prm, w.indexed ? w.obs.idx : nullptr, w.obs.bearings, w.obs.noise, chi2_dev,
                                                   w.obs.counters, apply, grid_for(h, w.indexed ? m : h->elems / 2, occ), h->stream));
  unsigned long long host_counts[sba::LANDMARK_CLASSES] = {0, 0, 0, 0};
  SBA_TRY_HIP(hipMemcpyAsync(host_counts, w.obs.counters, sizeof(host_counts), hipMemcpyDeviceToHost, h->stream));
  if (chi2_out && !chi2_direct)
    SBA_TRY_HIP(hipMemcpyAsync(chi2_out, w.obs.chi2, m * sizeof(double), on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream));
  rc = sba::stream_wait(h->stream, "robust landmark registration write-back", &h->poisoned);
  if (rc) return rc;
  for (int a = 0; a < 3; ++a) { res->rot[a] = r[a]; res->tran[a] = t[a]; }
  std::memcpy(res->cov, cov, sizeof(cov));
  counts_to_result(host_counts, res);
  res->n_used = static_cast<long long>(at->n_used);
  res->n_outlier = static_cast<long long>(at->n_outlier);
  sum.seconds_total = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
  res->summary = sum;
  return SBA_OK;
}

}  // namespace

extern "C" {

int sba_landmarks_eval_register_robust(sba_landmarks* h, const int64_t* idx, const double* bearings, size_t m, const double rot[3],
                                       const double tran[3], const double rot_ref[3], const double tran_ref[3],
                                       const sba_landmark_register_options* opt, sba_landmark_register_robust_eval* eval) {
  return eval_register_robust_common(h, idx, bearings, false, m, rot, tran, rot_ref, tran_ref, opt, eval);
}

int sba_landmarks_register_robust(sba_landmarks* h, const int64_t* idx, const double* bearings, size_t m, const double rot0[3], const double tran0[3],
                                  const sba_landmark_register_options* opt, sba_landmark_register_robust_result* res, double* chi2_out) {
  return register_robust_common(h, idx, bearings, false, m, rot0, tran0, opt, res, chi2_out);
}

int sba_landmarks_eval_register_robust_device(sba_landmarks* h, const int64_t* idx, const void* bearings_dev, size_t m, const double rot[3],
                                              const double tran[3], const double rot_ref[3], const double tran_ref[3],
                                              const sba_landmark_register_options* opt, sba_landmark_register_robust_eval* eval) {
  return eval_register_robust_common(h, idx, static_cast<const double*>(bearings_dev), true, m, rot, tran, rot_ref, tran_ref, opt, eval);
}

int sba_landmarks_register_robust_device(sba_landmarks* h, const int64_t* idx, const void* bearings_dev, size_t m, const double rot0[3],
                                         const double tran0[3], const sba_landmark_register_options* opt, sba_landmark_register_robust_result* res,
                                         void* chi2_out_dev) {
  return register_robust_common(h, idx, static_cast<const double*>(bearings_dev), true, m, rot0, tran0, opt, res, static_cast<double*>(chi2_out_dev));
}

}  // extern "C"

// ---- the joint registration under Hampel's redescending loss (sba_landmarks_register_hampel.hpp) -------------------------------------
namespace {

int register_hampel_occ(sba_landmarks* h, bool indexed, int* occ) {
  return cached_occ(&h->occ_reg_hampel[indexed ? 1 : 0], [&](int* o) { return sba::landmarks_register_hampel_blocks_per_cu(indexed, o); }, occ);
}

// The refusals of the four Hampel entry points, all before the first device call: robust_check's with the same codes, then the
// thresholds b and c.
int hampel_check(sba_landmarks* h, const int64_t* idx, const void* bearings, size_t m, const double* rot, const double* tran, const double* rot_ref,
                 const double* tran_ref, const sba_landmark_register_hampel_options* opt, const void* out, bool on_device, const void* chi2_out) {
  if (!opt) return sba::set_error(SBA_ERR_INVALID_ARG, "null argument");
  const int rc = robust_check(h, idx, bearings, m, rot, tran, rot_ref, tran_ref, &opt->base, out, on_device, chi2_out);
  if (rc) return rc;
  if (const char* why = sba::landmark_register_check_hampel(opt->base.lm.huber_delta, opt->b, opt->c, opt->base.chi2_gate))
    return sba::set_error(SBA_ERR_INVALID_ARG, "%s", why);
  return SBA_OK;
}

// robust_freeze, then the grid of the Hampel reduce pass by the same rule from landmarks_register_hampel_reduce_kernel's two
// occupancies.  w->grid_reduce stays the robust pass's, so that the Huber stage runs sba_landmarks_register_robust's very
// launches.  The block rows of both passes share the scratch, which is grown for the larger grid BEFORE robust_freeze lays it out.
int hampel_freeze(sba_landmarks* h, const int64_t* idx, const double* bearings, bool on_device, size_t m, const double rot_ref[3],
                  const double tran_ref[3], double bearing_sigma, RegisterWork* w, int* grid_hampel) {
  SBA_TRY_HIP(hipSetDevice(h->device));
  const bool indexed = idx != nullptr;
  int occ = 1, occ_other = 1;
  int rc = register_hampel_occ(h, indexed, &occ);
  if (rc) return rc;
  rc = register_hampel_occ(h, !indexed, &occ_other);
  if (rc) return rc;
  *grid_hampel = grid_for(h, indexed ? (m + 1) / 2 : h->elems / 2, std::min(occ, occ_other));
  rc = grow_scratch(&h->reg, &h->reg_bytes, kCounterBytes + (static_cast<size_t>(*grid_hampel) + 1) * sba::JOINT_ROW * sizeof(double));
  if (rc) return rc;
  return robust_freeze(h, idx, bearings, on_device, m, rot_ref, tran_ref, bearing_sigma, w);
}

int hampel_reduce_pass(sba_landmarks* h, const RegisterWork& w, int grid, const sba::LandmarkRegisterHampel& loss, const double rot[3],
                       const double tran[3], double* row) {
  sba::LandmarkRegisterParams prm;
  sba::landmark_register_fill(h->n, w.m, rot, tran, nullptr, w.bearing_sigma, INFINITY, &prm);
  SBA_TRY_HIP(sba::launch_landmarks_register_hampel_reduce(planes_of(h), prm, loss, w.indexed ? w.obs.idx : nullptr, w.obs.bearings, w.obs.noise,
                                                           w.partials, grid, w.row_dev, h->stream));
  SBA_TRY_HIP(hipMemcpyAsync(row, w.row_dev, sba::SBA_HAMPEL_COUNT * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  return sba::stream_wait(h->stream, "Hampel landmark registration reduce pass", &h->poisoned);
}

int eval_register_hampel_common(sba_landmarks* h, const int64_t* idx, const double* bearings, bool on_device, size_t m, const double rot[3],
                                const double tran[3], const double rot_ref[3], const double tran_ref[3],
                                const sba_landmark_register_hampel_options* opt, sba_landmark_register_hampel_eval* eval) {
  int rc = hampel_check(h, idx, bearings, m, rot, tran, rot_ref, tran_ref, opt, eval, on_device, nullptr);
  if (rc) return rc;
  *eval = sba_landmark_register_hampel_eval{};
  if (h->n == 0 || m == 0) return SBA_OK;
  RegisterWork w;
  int grid = 0;
  rc = hampel_freeze(h, idx, bearings, on_device, m, rot_ref, tran_ref, opt->base.bearing_sigma, &w, &grid);
  if (rc) return rc;
  sba::LandmarkRegisterHampel loss;
  sba::landmark_register_hampel_fill(opt->base.lm.huber_delta, opt->b, opt->c, &loss);
  double row[sba::JOINT_ROW] = {0};
  rc = hampel_reduce_pass(h, w, grid, loss, rot, tran, row);
  if (rc) return rc;
  if (!sba::resect_row_finite(row)) return sba::set_error(SBA_ERR_NUMERIC, "non-finite registration sums");
  sba_normal_eq ne;
  double n_behind = 0.0;
  sba::resect_expand_row(row, &ne, &n_behind);
  std::memcpy(eval->H, ne.H, sizeof(ne.H));
  std::memcpy(eval->g, ne.g, sizeof(ne.g));
  eval->cost = ne.cost;
  eval->n_used = static_cast<long long>(ne.sum_w);
  eval->n_behind = static_cast<long long>(n_behind);
  eval->n_outlier = static_cast<long long>(ne.n_outlier);
  eval->n_rejected = static_cast<long long>(row[sba::SBA_HAMPEL_NREJ]);
  return SBA_OK;
}

int register_hampel_common(sba_landmarks* h, const int64_t* idx, const double* bearings, bool on_device, size_t m, const double rot0[3],
                           const double tran0[3], const sba_landmark_register_hampel_options* opt, sba_landmark_register_hampel_result* res,
                           double* chi2_out) {
  int rc = hampel_check(h, idx, bearings, m, rot0, tran0, rot0, tran0, opt, res, on_device, chi2_out);
  if (rc) return rc;
  *res = sba_landmark_register_hampel_result{};
  for (int a = 0; a < 3; ++a) { res->rot[a] = res->rot_huber[a] = rot0[a]; res->tran[a] = res->tran_huber[a] = tran0[a]; }
  if (h->n == 0 || m == 0) return SBA_OK;
  const auto t_start = std::chrono::steady_clock::now();
  const sba_landmark_register_options& base = opt->base;
  RegisterWork w;
  int grid = 0;
  rc = hampel_freeze(h, idx, bearings, on_device, m, rot0, tran0, base.bearing_sigma, &w, &grid);
  if (rc) return rc;
  if (w.freeze_counts[sba::LANDMARK_LIVE] < 3)
    return sba::set_error(SBA_ERR_NUMERIC, "pose not determined: %lld observations take part after the freeze (%lld skipped, %lld behind), 3 are needed",
                          w.freeze_counts[sba::LANDMARK_LIVE], w.freeze_counts[sba::LANDMARK_SKIPPED], w.freeze_counts[sba::LANDMARK_BEHIND]);
  sba::LandmarkRegisterRobust huber_loss;
  sba::landmark_register_robust_fill(base.lm.huber_delta, &huber_loss);
  sba::LandmarkRegisterHampel loss;
  sba::landmark_register_hampel_fill(base.lm.huber_delta, opt->b, opt->c, &loss);
  struct Visit { double rot[3], tran[3], H[36], n_used, n_outlier, n_rejected; };
  std::vector<Visit> visits;
  double seconds_eval = 0.0;
  int eval_rc = SBA_OK;
  bool hampel_stage = false;
  auto evaluate = [&](const double r[3], const double t[3], sba_normal_eq* ne) -> bool {
    const auto t0 = std::chrono::steady_clock::now();
    double row[sba::JOINT_ROW] = {0};
    eval_rc = hampel_stage ? hampel_reduce_pass(h, w, grid, loss, r, t, row) : robust_reduce_pass(h, w, huber_loss, r, t, row);
    seconds_eval += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (eval_rc) return false;
    if (!sba::resect_row_finite(row)) return false;
    sba::resect_expand_row(row, ne, nullptr);
    Visit v;
    for (int a = 0; a < 3; ++a) { v.rot[a] = r[a]; v.tran[a] = t[a]; }
    std::memcpy(v.H, ne->H, sizeof(v.H));
    v.n_used = ne->sum_w;
    v.n_outlier = ne->n_outlier;
    v.n_rejected = row[sba::SBA_HAMPEL_NREJ];
    visits.push_back(v);
    return true;
  };
  double r[3] = {rot0[0], rot0[1], rot0[2]}, t[3] = {tran0[0], tran0[1], tran0[2]};
  sba_lm_summary sum;
  int huber_iterations = 0;
  if (opt->huber_first) {
    // stage 1: sba_landmarks_register_robust's solve -- its kernel, its grid, its options -- from the start pose
    std::memset(&sum, 0, sizeof(sum));
    const int status = sba::lm_solve(SBA_MODE_RT, r, t, base.lm, evaluate, &sum);
    if (eval_rc) return eval_rc;
    if (status != SBA_OK) return sba::set_error(status, "Hampel joint registration: the Huber stage failed: non-finite sums or 5 consecutive invalid steps");
    huber_iterations = sum.num_iterations;
    visits.clear();
  }
  const double r_huber[3] = {r[0], r[1], r[2]}, t_huber[3] = {t[0], t[1], t[2]};
  // stage 2: the Hampel solve from there, on the same frozen noise
  hampel_stage = true;
  seconds_eval = 0.0;
  std::memset(&sum, 0, sizeof(sum));
  const int status = sba::lm_solve(SBA_MODE_RT, r, t, base.lm, evaluate, &sum);
  if (eval_rc) return eval_rc;
  sum.seconds_eval = seconds_eval;
  if (status != SBA_OK) return sba::set_error(status, "Hampel joint registration solve failed: non-finite sums or 5 consecutive invalid steps");
  const Visit* at = nullptr;
  for (size_t k = visits.size(); k-- > 0;)
    if (std::memcmp(visits[k].rot, r, sizeof(r)) == 0 && std::memcmp(visits[k].tran, t, sizeof(t)) == 0) { at = &visits[k]; break; }
  if (at && at->n_used - at->n_rejected < 3.0)
    return sba::set_error(SBA_ERR_NUMERIC, "pose not determined: %lld of the %lld observations at the solution lie beyond c and carry no weight, 3 with weight are needed",
                          static_cast<long long>(at->n_rejected), static_cast<long long>(at->n_used));
  double cov[36];
  if (!at || !sba::resect_cov_inverse(at->H, cov))
    return sba::set_error(SBA_ERR_NUMERIC, "pose not determined: the reduced normal matrix is not positive definite at the solution");
  // the write-back at the solution: sba_landmarks_register's, with Sigma_c = H_rho^-1
  const bool apply = base.apply != 0;
  int occ = 1;
  rc = register_occ(h, sba::LANDMARK_REGISTER_APPLY, w.indexed, apply, &occ);
  if (rc) return rc;
  // chi2 on the device goes straight to the caller where the pass's stores fit (dense_vectors_fit), else through the scratch
  const bool chi2_direct = on_device && chi2_out && (w.indexed || dense_vectors_fit(chi2_out, m));
  double* chi2_dev = !chi2_out ? nullptr : (chi2_direct ? chi2_out : w.obs.chi2);
  sba::LandmarkRegisterParams prm;
  sba::landmark_register_fill(h->n, m, r, t, cov, base.bearing_sigma, base.chi2_gate, &prm);
  SBA_TRY_HIP(sba::launch_landmarks_register_apply(planes_of(h), prm, w.indexed ? w.obs.idx : nullptr, w.obs.bearings, w.obs.noise, chi2_dev,
                                                   w.obs.counters, apply, grid_for(h, w.indexed ? m : h->elems / 2, occ), h->stream));
  unsigned long long host_counts[sba::LANDMARK_CLASSES] = {0, 0, 0, 0};
  SBA_TRY_HIP(hipMemcpyAsync(host_counts, w.obs.counters, sizeof(host_counts), hipMemcpyDeviceToHost, h->stream));
  if (chi2_out && !chi2_direct)
    SBA_TRY_HIP(hipMemcpyAsync(chi2_out, w.obs.chi2, m * sizeof(double), on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream));
  rc = sba::stream_wait(h->stream, "Hampel landmark registration write-back", &h->poisoned);
  if (rc) return rc;
  for (int a = 0; a < 3; ++a) { res->rot[a] = r[a]; res->tran[a] = t[a]; res->rot_huber[a] = r_huber[a]; res->tran_huber[a] = t_huber[a]; }
  std::memcpy(res->cov, cov, sizeof(cov));
  counts_to_result(host_counts, res);
  res->n_used = static_cast<long long>(at->n_used);
  res->n_outlier = static_cast<long long>(at->n_outlier);
  res->n_rejected = static_cast<long long>(at->n_rejected);
  res->huber_iterations = huber_iterations;
  sum.seconds_total = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
  res->summary = sum;
  return SBA_OK;
}

}  // namespace

extern "C" {

int sba_landmarks_eval_register_hampel(sba_landmarks* h, const int64_t* idx, const double* bearings, size_t m, const double rot[3],
                                       const double tran[3], const double rot_ref[3], const double tran_ref[3],
                                       const sba_landmark_register_hampel_options* opt, sba_landmark_register_hampel_eval* eval) {
  return eval_register_hampel_common(h, idx, bearings, false, m, rot, tran, rot_ref, tran_ref, opt, eval);
}

int sba_landmarks_register_hampel(sba_landmarks* h, const int64_t* idx, const double* bearings, size_t m, const double rot0[3], const double tran0[3],
                                  const sba_landmark_register_hampel_options* opt, sba_landmark_register_hampel_result* res, double* chi2_out) {
  return register_hampel_common(h, idx, bearings, false, m, rot0, tran0, opt, res, chi2_out);
}

int sba_landmarks_eval_register_hampel_device(sba_landmarks* h, const int64_t* idx, const void* bearings_dev, size_t m, const double rot[3],
                                              const double tran[3], const double rot_ref[3], const double tran_ref[3],
                                              const sba_landmark_register_hampel_options* opt, sba_landmark_register_hampel_eval* eval) {
  return eval_register_hampel_common(h, idx, static_cast<const double*>(bearings_dev), true, m, rot, tran, rot_ref, tran_ref, opt, eval);
}

int sba_landmarks_register_hampel_device(sba_landmarks* h, const int64_t* idx, const void* bearings_dev, size_t m, const double rot0[3],
                                         const double tran0[3], const sba_landmark_register_hampel_options* opt, sba_landmark_register_hampel_result* res,
                                         void* chi2_out_dev) {
  return register_hampel_common(h, idx, static_cast<const double*>(bearings_dev), true, m, rot0, tran0, opt, res, static_cast<double*>(chi2_out_dev));
}

}  // extern "C"

// ---- the descriptors: a row per landmark, and the association of a frame with the map (sba_landmarks_associate.hpp) ----------------
namespace {

int associate_occ(sba_landmarks* h, int which, int* occ) {
  return cached_occ(&h->occ_assoc[which], [&](int* o) { return sba::landmarks_associate_blocks_per_cu(which, o); }, occ);
}

int set_descriptors_common(sba_landmarks* h, const void* desc, size_t n_rows, int dim, size_t row_stride_bytes, bool from_device) {
  if (!h) return sba::set_error(SBA_ERR_INVALID_ARG, "null landmark handle");
  SBA_REFUSE_POISONED(h);
  if (dim == 0) { h->desc_dim = 0; return SBA_OK; }       // the map keeps none from here on; the allocations stay for the next set
  if (const char* why = sba::descriptor_check_rows(dim, row_stride_bytes))
    return sba::set_error(SBA_ERR_INVALID_ARG, "%s (dim = %d, row_stride_bytes = %zu)", why, dim, row_stride_bytes);
  if (n_rows != h->n) return sba::set_error(SBA_ERR_INVALID_ARG, "one descriptor row per landmark: n_rows = %zu, the map holds %zu", n_rows, h->n);
  if (n_rows > 0 && !desc) return sba::set_error(SBA_ERR_INVALID_ARG, "null descriptor array");
  if (from_device && (reinterpret_cast<uintptr_t>(desc) & 3u) != 0) return sba::set_error(SBA_ERR_INVALID_ARG, "device descriptor rows must be 4-byte aligned");
  SBA_TRY_HIP(hipSetDevice(h->device));
  // into the other allocation, swapped in once the rows are in place: a failed call leaves the old rows
  int rc = alt_desc(h, n_rows, dim);
  if (rc) return rc;
  if (n_rows) {
    rc = pack_desc_rows(h, h->desc_alt, desc, n_rows, dim, row_stride_bytes, from_device);
    if (rc) return rc;
    rc = sba::stream_wait(h->stream, "landmark descriptors", &h->poisoned);
    if (rc) return rc;
  }
  swap_desc(h, dim);
  return SBA_OK;
}

// What one association works on, carved from h->assoc; every part starts 256-byte aligned.
struct AssociateScratch {
  float* frame = nullptr;                    // packed frame rows [m][dim], when they are not read in place
  double* bearings = nullptr;                // the frame's bearings [m][3], when they come from the host
  int *match_row = nullptr, *match_landmark = nullptr;
  float* match_dist = nullptr;
  unsigned long long *slots = nullptr, *tile_offset = nullptr, *counters = nullptr;   // counters: accepted, associated
  unsigned char* keep = nullptr;
  unsigned int* tile_count = nullptr;
  long long* idx = nullptr;
  int* row = nullptr;
  float* dist = nullptr;
  double* bearings_out = nullptr;            // [cap][3], when they go to the host
};

int associate_scratch(sba_landmarks* h, size_t m, int dim, bool stage_frame, bool stage_bearings, bool stage_bearings_out, size_t ntiles,
                      AssociateScratch* s) {
  const size_t n = h->n, cap = std::min(n, m);
  size_t off = 0;
  auto carve = [&](size_t bytes) { const size_t o = off; off += (std::max<size_t>(bytes, 1) + 255) / 256 * 256; return o; };
  const size_t o_frame = carve(stage_frame ? m * static_cast<size_t>(dim) * sizeof(float) : 0);
  const size_t o_bear = carve(stage_bearings ? 3 * m * sizeof(double) : 0);
  const size_t o_mr = carve(m * sizeof(int)), o_ml = carve(m * sizeof(int)), o_md = carve(m * sizeof(float));
  const size_t o_slots = carve(n * sizeof(unsigned long long)), o_toff = carve(ntiles * sizeof(unsigned long long));
  const size_t o_cnt = carve(2 * sizeof(unsigned long long)), o_keep = carve(ntiles * sba::kCompactTile), o_tcount = carve(ntiles * sizeof(unsigned int));
  const size_t o_idx = carve(cap * sizeof(long long)), o_row = carve(cap * sizeof(int)), o_dist = carve(cap * sizeof(float));
  const size_t o_bout = carve(stage_bearings_out ? 3 * cap * sizeof(double) : 0);
  const int rc = grow_scratch(&h->assoc, &h->assoc_bytes, off, 2);
  if (rc) return rc;
  char* w = static_cast<char*>(h->assoc);
  s->frame = reinterpret_cast<float*>(w + o_frame);
  s->bearings = reinterpret_cast<double*>(w + o_bear);
  s->match_row = reinterpret_cast<int*>(w + o_mr);
  s->match_landmark = reinterpret_cast<int*>(w + o_ml);
  s->match_dist = reinterpret_cast<float*>(w + o_md);
  s->slots = reinterpret_cast<unsigned long long*>(w + o_slots);
  s->tile_offset = reinterpret_cast<unsigned long long*>(w + o_toff);
  s->counters = reinterpret_cast<unsigned long long*>(w + o_cnt);
  s->keep = reinterpret_cast<unsigned char*>(w + o_keep);
  s->tile_count = reinterpret_cast<unsigned int*>(w + o_tcount);
  s->idx = reinterpret_cast<long long*>(w + o_idx);
  s->row = reinterpret_cast<int*>(w + o_row);
  s->dist = reinterpret_cast<float*>(w + o_dist);
  s->bearings_out = reinterpret_cast<double*>(w + o_bout);
  return SBA_OK;
}

// Both forms.  on_device: frame_desc, frame_bearings and bearings_out are device pointers; idx_out, row_out and dist_out are on
// the host in both.  Two waits: the matcher's count, then the associated count with the outputs.  The claim reads the matcher's
// compacted list of accepted rows, which is on the device when the first wait returns, so no wait stands between them.
int associate_common(sba_landmarks* h, const void* frame_desc, size_t m, int dim, size_t row_stride_bytes, const void* frame_bearings,
                     const sba_landmark_associate_options* opt, sba_landmark_associate_result* res, int64_t* idx_out, int32_t* row_out, float* dist_out,
                     void* bearings_out, bool on_device) {
  if (!h || !opt || !res || (m > 0 && !frame_desc)) return sba::set_error(SBA_ERR_INVALID_ARG, "null argument");
  SBA_REFUSE_POISONED(h);
  if (const char* why = sba::associate_check_options(opt->ratio, opt->max_distance))
    return sba::set_error(SBA_ERR_INVALID_ARG, "%s (ratio = %g, max_distance = %g)", why, opt->ratio, opt->max_distance);
  if (h->desc_dim == 0) return sba::set_error(SBA_ERR_INVALID_ARG, "the map keeps no descriptors: sba_landmarks_set_descriptors comes first");
  if (dim != h->desc_dim) return sba::set_error(SBA_ERR_INVALID_ARG, "the map keeps descriptors of dimension %d, the frame has %d", h->desc_dim, dim);
  if (const char* why = sba::descriptor_check_rows(dim, row_stride_bytes))
    return sba::set_error(SBA_ERR_INVALID_ARG, "%s (dim = %d, row_stride_bytes = %zu)", why, dim, row_stride_bytes);
  if (const char* why = sba::associate_check_sizes(h->n, m)) return sba::set_error(SBA_ERR_INVALID_ARG, "%s (n = %zu, m_frame = %zu)", why, h->n, m);
  if (on_device && ((reinterpret_cast<uintptr_t>(frame_desc) & 3u) != 0 || (reinterpret_cast<uintptr_t>(frame_bearings) & 7u) != 0 ||
                    (reinterpret_cast<uintptr_t>(bearings_out) & 15u) != 0))
    return sba::set_error(SBA_ERR_INVALID_ARG, "device rows: descriptors 4-byte, bearings 8-byte, bearings_out 16-byte aligned");
  *res = sba_landmark_associate_result{};
  res->n_frame = static_cast<long long>(m);
  const size_t n = h->n;
  if (n < 2 || m == 0) return SBA_OK;            // the matcher's rule: with fewer than two train rows nothing matches
  SBA_TRY_HIP(hipSetDevice(h->device));
  const bool gather = frame_bearings != nullptr && bearings_out != nullptr;
  const bool packed = row_stride_bytes == static_cast<size_t>(dim) * sizeof(float);
  const size_t ntiles = (n + sba::kCompactTile - 1) / sba::kCompactTile;
  AssociateScratch s;
  int rc = associate_scratch(h, m, dim, !on_device || !packed, gather && !on_device, gather && !on_device, ntiles, &s);
  if (rc) return rc;
  // the frame's rows as the map's are: packed, so that one stride serves both sides of the matcher
  const float* frame_dev = static_cast<const float*>(frame_desc);
  if (!on_device || !packed) {
    rc = pack_desc_rows(h, s.frame, frame_desc, m, dim, row_stride_bytes, on_device);
    if (rc) return rc;
    frame_dev = s.frame;
  }
  const double* bearings_dev = static_cast<const double*>(frame_bearings);
  double* bearings_out_dev = static_cast<double*>(bearings_out);
  if (gather && !on_device) {
    SBA_TRY_HIP(hipMemcpyAsync(s.bearings, frame_bearings, 3 * m * sizeof(double), hipMemcpyHostToDevice, h->stream));
    bearings_dev = s.bearings;
    bearings_out_dev = s.bearings_out;
  }
  size_t n_matched = 0;
  rc = sba::match::match_pair_on_stream(h->stream, &h->poisoned, h->num_cus, frame_dev, m, h->desc, n, dim, static_cast<size_t>(dim) * sizeof(float),
                                        opt->ratio, nullptr, nullptr, &n_matched, s.match_row, s.match_landmark, s.match_dist);   // the first wait
  if (rc) return rc;
  if (n_matched == 0) return SBA_OK;
  if (n_matched > m) return sba::set_error(SBA_ERR_NUMERIC, "the matcher accepted %zu of %zu frame rows", n_matched, m);
  SBA_TRY_HIP(hipMemsetAsync(s.slots, 0xff, n * sizeof(unsigned long long), h->stream));       // kAssociateUnclaimed
  SBA_TRY_HIP(hipMemsetAsync(s.counters, 0, 2 * sizeof(unsigned long long), h->stream));
  int occ = 1;
  rc = associate_occ(h, sba::LANDMARK_ASSOC_CLAIM, &occ);
  if (rc) return rc;
  SBA_TRY_HIP(sba::launch_landmarks_claim(s.match_row, s.match_landmark, s.match_dist, n_matched, opt->max_distance, s.slots, s.counters,
                                          grid_for(h, n_matched, occ), h->stream));
  rc = associate_occ(h, sba::LANDMARK_ASSOC_KEEP, &occ);
  if (rc) return rc;
  SBA_TRY_HIP(sba::launch_landmarks_associate_keep(s.slots, n, s.keep, ntiles, grid_for(h, ntiles * sba::kCompactTile, occ), h->stream));
  SBA_TRY_HIP(sba::launch_compact_count(s.keep, ntiles, s.tile_count, h->stream));
  SBA_TRY_HIP(sba::launch_compact_scan(s.tile_count, ntiles, s.tile_offset, s.counters + 1, h->stream));
  SBA_TRY_HIP(sba::launch_landmarks_associate_scatter(s.keep, n, s.tile_offset, ntiles, s.slots, gather ? bearings_dev : nullptr, s.idx, s.row, s.dist,
                                                      gather ? bearings_out_dev : nullptr, h->stream));
  // No more landmarks are claimed than rows were accepted: that many rows of every output come back with the counts, and the
  // caller's arrays receive the associated ones after the wait.
  const size_t fetch = std::min(n_matched, n);
  unsigned long long host_counts[2] = {0, 0};
  std::vector<int64_t> idx_host(idx_out ? fetch : 0);
  std::vector<int32_t> row_host(row_out ? fetch : 0);
  std::vector<float> dist_host(dist_out ? fetch : 0);
  std::vector<double> bearings_host(gather && !on_device ? 3 * fetch : 0);
  SBA_TRY_HIP(hipMemcpyAsync(host_counts, s.counters, sizeof(host_counts), hipMemcpyDeviceToHost, h->stream));
  if (idx_out) SBA_TRY_HIP(hipMemcpyAsync(idx_host.data(), s.idx, fetch * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
  if (row_out) SBA_TRY_HIP(hipMemcpyAsync(row_host.data(), s.row, fetch * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  if (dist_out) SBA_TRY_HIP(hipMemcpyAsync(dist_host.data(), s.dist, fetch * sizeof(float), hipMemcpyDeviceToHost, h->stream));
  if (gather && !on_device) SBA_TRY_HIP(hipMemcpyAsync(bearings_host.data(), s.bearings_out, 3 * fetch * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  rc = sba::stream_wait(h->stream, "landmark association", &h->poisoned);                      // the second wait
  if (rc) return rc;
  const size_t n_accepted = static_cast<size_t>(host_counts[0]), n_associated = static_cast<size_t>(host_counts[1]);
  if (n_accepted > n_matched || n_associated > std::min(n_accepted, n))
    return sba::set_error(SBA_ERR_NUMERIC, "the claim accepted %zu of %zu matched rows and %zu landmarks were claimed", n_accepted, n_matched, n_associated);
  if (idx_out) std::memcpy(idx_out, idx_host.data(), n_associated * sizeof(int64_t));
  if (row_out) std::memcpy(row_out, row_host.data(), n_associated * sizeof(int32_t));
  if (dist_out) std::memcpy(dist_out, dist_host.data(), n_associated * sizeof(float));
  if (gather && !on_device) std::memcpy(bearings_out, bearings_host.data(), 3 * n_associated * sizeof(double));
  res->n_accepted = static_cast<long long>(n_accepted);
  res->n_associated = static_cast<long long>(n_associated);
  res->n_contested = res->n_accepted - res->n_associated;
  return SBA_OK;
}

}  // namespace

extern "C" {

int sba_landmarks_set_descriptors(sba_landmarks* h, const float* desc, size_t n_rows, int dim, size_t row_stride_bytes) {
  return set_descriptors_common(h, desc, n_rows, dim, row_stride_bytes, false);
}

int sba_landmarks_set_descriptors_device(sba_landmarks* h, const void* desc_dev, size_t n_rows, int dim, size_t row_stride_bytes) {
  return set_descriptors_common(h, desc_dev, n_rows, dim, row_stride_bytes, true);
}

int sba_landmarks_descriptor_dim(const sba_landmarks* h, int* dim) {
  if (!h || !dim) return sba::set_error(SBA_ERR_INVALID_ARG, "null argument");
  *dim = h->desc_dim;
  return SBA_OK;
}

int sba_landmarks_get_descriptors(sba_landmarks* h, const int64_t* idx, size_t m, float* out, size_t out_stride_bytes) {
  if (!h) return sba::set_error(SBA_ERR_INVALID_ARG, "null landmark handle");
  SBA_REFUSE_POISONED(h);
  if (h->desc_dim == 0) return sba::set_error(SBA_ERR_INVALID_ARG, "the map keeps no descriptors");
  if (const char* why = sba::descriptor_check_rows(h->desc_dim, out_stride_bytes))
    return sba::set_error(SBA_ERR_INVALID_ARG, "%s (dim = %d, out_stride_bytes = %zu)", why, h->desc_dim, out_stride_bytes);
  const size_t rows = idx ? m : h->n;
  if (const char* why = sba::landmark_check_sizes(0, rows)) return sba::set_error(SBA_ERR_INVALID_ARG, "%s (m = %zu)", why, rows);
  if (const char* why = sba::landmark_check_gather_index(idx, idx ? m : 0, h->n)) return sba::set_error(SBA_ERR_INVALID_ARG, "%s (m = %zu, n = %zu)", why, m, h->n);
  if (rows == 0) return SBA_OK;
  if (!out) return sba::set_error(SBA_ERR_INVALID_ARG, "null output array");
  SBA_TRY_HIP(hipSetDevice(h->device));
  const size_t width = static_cast<size_t>(h->desc_dim) * sizeof(float);
  const float* rows_dev = h->desc;
  if (idx) {                     // idx [m] | rows [m][dim] in the edit scratch
    const size_t o_rows = up16(m * sizeof(int64_t));
    int rc = edit_scratch(h, o_rows + m * width);
    if (rc) return rc;
    long long* idx_dev = static_cast<long long*>(h->edit);
    float* gathered = reinterpret_cast<float*>(static_cast<char*>(h->edit) + o_rows);
    SBA_TRY_HIP(hipMemcpyAsync(idx_dev, idx, m * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
    int occ = 1;
    rc = associate_occ(h, sba::LANDMARK_ASSOC_DESC_GATHER, &occ);
    if (rc) return rc;
    SBA_TRY_HIP(sba::launch_landmarks_desc_gather(h->desc, h->desc_dim, idx_dev, m, gathered, grid_for(h, m * 16, occ), h->stream));
    rows_dev = gathered;
  }
  SBA_TRY_HIP(hipMemcpy2DAsync(out, out_stride_bytes, rows_dev, width, width, rows, hipMemcpyDeviceToHost, h->stream));
  return sba::stream_wait(h->stream, "landmark descriptors", &h->poisoned);
}

int sba_landmarks_append_described(sba_landmarks* h, const double* xyz, const double* cov, const float* desc, size_t n_add, int dim,
                                   size_t row_stride_bytes, double cov_scale) {
  return append_common(h, xyz, cov, n_add, cov_scale, false, desc, dim, row_stride_bytes, true);
}

int sba_landmarks_append_described_device(sba_landmarks* h, const void* xyz_dev, const void* cov_dev, const void* desc_dev, size_t n_add, int dim,
                                          size_t row_stride_bytes, double cov_scale) {
  return append_common(h, xyz_dev, cov_dev, n_add, cov_scale, true, desc_dev, dim, row_stride_bytes, true);
}

int sba_landmarks_associate(sba_landmarks* h, const float* frame_desc, size_t m_frame, int dim, size_t row_stride_bytes, const double* frame_bearings,
                            const sba_landmark_associate_options* opt, sba_landmark_associate_result* res, int64_t* idx_out, int32_t* row_out,
                            float* dist_out, double* bearings_out) {
  return associate_common(h, frame_desc, m_frame, dim, row_stride_bytes, frame_bearings, opt, res, idx_out, row_out, dist_out, bearings_out, false);
}

int sba_landmarks_associate_device(sba_landmarks* h, const void* frame_desc_dev, size_t m_frame, int dim, size_t row_stride_bytes,
                                   const void* frame_bearings_dev, const sba_landmark_associate_options* opt, sba_landmark_associate_result* res,
                                   int64_t* idx_out, int32_t* row_out, float* dist_out, void* bearings_out_dev) {
  return associate_common(h, frame_desc_dev, m_frame, dim, row_stride_bytes, frame_bearings_dev, opt, res, idx_out, row_out, dist_out,
                          bearings_out_dev, true);
}

}  // extern "C"
