// Entry points of the descriptor match (include/sba_hip.h): exact L2 2-NN with the reference's ratio test for one pair or
// a batch of ragged pairs, and the uploads of a problem / batch straight from the matched key-points.  Kernels:
// sba_match_kernels.hip (match), sba_side.hip (key-point gather).  DESIGN.md section 3.10.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "sba_batch.hpp"
#include "sba_match.hpp"
#include "sba_problem.hpp"

namespace sba {
namespace match {
namespace {

int require_device(int device) {
  int count = 0;
  const hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0)
    return set_error(SBA_ERR_NO_DEVICE, "no HIP device available (%s); this library has no CPU path",
                     e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
  if (device < 0 || device >= count) return set_error(SBA_ERR_INVALID_ARG, "device %d out of range [0,%d)", device, count);
  SBA_TRY_HIP(hipSetDevice(device));
  return SBA_OK;
}

// The argument checks every match entry point shares; all of them run before any device call.
int check_match_args(int dim, size_t row_stride_bytes, float ratio) {
  if (dim < 1 || dim > 256) return set_error(SBA_ERR_INVALID_ARG, "descriptor dimension %d out of range [1, 256]", dim);
  if (row_stride_bytes < 4 * static_cast<size_t>(dim) || row_stride_bytes % 4 != 0)
    return set_error(SBA_ERR_INVALID_ARG, "row_stride_bytes %zu must be a multiple of 4 and >= 4 * dim = %d", row_stride_bytes,
                     4 * dim);
  if (!std::isfinite(ratio) || !(ratio > 0.f)) return set_error(SBA_ERR_INVALID_ARG, "ratio %g must be finite and > 0", ratio);
  return SBA_OK;
}
int check_offsets(const size_t* offsets, int num_pairs, const char* what) {
  if (num_pairs < 0) return set_error(SBA_ERR_INVALID_ARG, "num_pairs %d < 0", num_pairs);
  if (num_pairs > 0 && !offsets) return set_error(SBA_ERR_INVALID_ARG, "%s offsets are null", what);
  for (int g = 0; g < num_pairs; ++g)
    if (offsets[g + 1] < offsets[g]) return set_error(SBA_ERR_INVALID_ARG, "%s offsets must be non-decreasing", what);
  return SBA_OK;
}
int check_keypoint_args(size_t stride_bytes, int im_width, int im_height) {
  if (stride_bytes < 8 || stride_bytes % 4 != 0)
    return set_error(SBA_ERR_INVALID_ARG, "stride_bytes must be a multiple of 4 and >= 8");
  if (im_width <= 0 || im_height <= 0) return set_error(SBA_ERR_INVALID_ARG, "bad image size");
  return SBA_OK;
}
size_t rows_bytes(size_t rows, size_t stride, size_t last_row_bytes) { return rows == 0 ? 0 : (rows - 1) * stride + last_row_bytes; }

// One match of every pair g: query rows qoff[g] .. qoff[g + 1] against train rows toff[g] .. toff[g + 1] of the device
// arrays `query` / `train` (offsets relative to those pointers).  Optional device outputs (null = not wanted): nn_index /
// nn_dist [total queries][2]; match_q / match_t / match_d (capacity: total queries) and rows_q / rows_t, the absolute rows
// of the accepted matches.  n_matched[g] (host) and *total: the accepted queries.  One synchronisation: the counts.
struct Args {
  hipStream_t stream = nullptr;
  int* poisoned = nullptr;
  int num_cus = 256;
  const uint8_t* query = nullptr;
  const uint8_t* train = nullptr;
  const size_t* qoff = nullptr;
  const size_t* toff = nullptr;
  int num_pairs = 0;
  int dim = 0;
  size_t stride = 0;
  float ratio = 0.3f;
  int* nn_index = nullptr;
  float* nn_dist = nullptr;
  int* match_q = nullptr;
  int* match_t = nullptr;
  float* match_d = nullptr;
  unsigned long long* rows_q = nullptr;
  unsigned long long* rows_t = nullptr;
  size_t* n_matched = nullptr;
  size_t* total = nullptr;
};

int run(const Args& a) {
  const int B = a.num_pairs;
  const size_t total_q = B > 0 ? a.qoff[B] - a.qoff[0] : 0;
  if (a.total) *a.total = 0;
  for (int g = 0; g < B; ++g) a.n_matched[g] = 0;
  if (total_q == 0) return SBA_OK;
  const int dp = match_padded_dim(a.dim), qb = match_query_block(dp);

  // layout of the packed copies and the split of the train rows
  std::vector<MatchPair> pairs(B);
  std::vector<unsigned long long> qoff_rel(B + 1), toff_rel(B + 1);
  size_t q_pack = 0, t_pack = 0, qblocks = 0, max_tiles = 0;
  for (int g = 0; g < B; ++g) {
    MatchPair& P = pairs[g];
    P.q_row0 = a.qoff[g];
    P.t_row0 = a.toff[g];
    P.q_out0 = a.qoff[g] - a.qoff[0];
    P.nq = static_cast<unsigned>(a.qoff[g + 1] - a.qoff[g]);
    P.nt = static_cast<unsigned>(a.toff[g + 1] - a.toff[g]);
    P.t_tiles = (P.nt + kMatchTile - 1) / kMatchTile;
    P.pad_ = 0;
    P.q_pack = q_pack;
    P.t_pack = t_pack;
    const size_t nqb = (P.nq + qb - 1) / qb;
    q_pack += nqb * qb;
    t_pack += static_cast<size_t>(P.t_tiles) * kMatchTile;
    qblocks += nqb;
    max_tiles = std::max<size_t>(max_tiles, P.t_tiles);
    qoff_rel[g] = a.qoff[g] - a.qoff[0];
    toff_rel[g] = a.toff[g] - a.toff[0];
  }
  qoff_rel[B] = a.qoff[B] - a.qoff[0];
  toff_rel[B] = a.toff[B] - a.toff[0];
  const size_t total_t = toff_rel[B];
  // Split policy: few query blocks (few queries, e.g. C1's 2 k) cannot fill the device, so the train tiles of every pair are
  // cut into `splits` ranges, each its own block, until there are about four blocks per CU -- never below 4 tiles (128 train
  // rows) per range, never above 64 ranges.  The per-range top-2 lists merge lexicographically: the result does not depend on it.
  size_t splits = 1;
  const size_t target = 4 * static_cast<size_t>(std::max(a.num_cus, 1));
  if (qblocks > 0 && qblocks < target) splits = (target + qblocks - 1) / qblocks;
  splits = std::max<size_t>(1, std::min<size_t>({splits, std::max<size_t>(1, max_tiles / 4), 64}));
  std::vector<MatchItem> items;
  items.reserve(qblocks * splits);
  for (int g = 0; g < B; ++g) {
    const unsigned nqb = (pairs[g].nq + qb - 1) / qb;
    for (unsigned k = 0; k < nqb; ++k)
      for (unsigned s = 0; s < splits; ++s) items.push_back(MatchItem{static_cast<unsigned>(g), k, s, 0u});
  }

  // one workspace allocation
  const size_t ntiles = (total_q + kCompactTile - 1) / kCompactTile;
  auto up = [](size_t b) { return (b + 255) & ~size_t(255); };
  size_t off = 0;
  auto carve = [&](size_t bytes) { const size_t o = off; off += up(std::max<size_t>(bytes, 1)); return o; };
  const size_t o_pairs = carve(sizeof(MatchPair) * B), o_qoff = carve(8 * (B + 1)), o_toff = carve(8 * (B + 1));
  const size_t o_items = carve(sizeof(MatchItem) * items.size());
  const size_t o_qpack = carve(q_pack * dp * 4), o_tpack = carve(t_pack * dp * 4), o_tnorm = carve(t_pack * 4);
  const size_t o_part = carve(q_pack * splits * sizeof(float4));
  const size_t o_nn_i = carve(total_q * 2 * sizeof(int)), o_nn_d = carve(total_q * 2 * sizeof(float));
  const size_t o_keep = carve(ntiles * kCompactTile), o_count = carve(4 * static_cast<size_t>(B));
  const size_t o_tcount = carve(4 * ntiles), o_toffset = carve(8 * ntiles), o_total = carve(8);
  const size_t o_mq = carve(a.match_q ? 0 : 4 * total_q), o_mt = carve(a.match_t ? 0 : 4 * total_q);
  const size_t o_md = carve(a.match_d ? 0 : 4 * total_q);
  DeviceBuffer work(a.poisoned);
  SBA_TRY_HIP(work.alloc(off));
  char* w = work.as<char>();
  MatchPair* pairs_dev = reinterpret_cast<MatchPair*>(w + o_pairs);
  auto* qoff_dev = reinterpret_cast<unsigned long long*>(w + o_qoff);
  auto* toff_dev = reinterpret_cast<unsigned long long*>(w + o_toff);
  MatchItem* items_dev = reinterpret_cast<MatchItem*>(w + o_items);
  float* qpack = reinterpret_cast<float*>(w + o_qpack);
  float* tpack = reinterpret_cast<float*>(w + o_tpack);
  float* tnorm = reinterpret_cast<float*>(w + o_tnorm);
  float4* part = reinterpret_cast<float4*>(w + o_part);
  int* nn_index = reinterpret_cast<int*>(w + o_nn_i);
  float* nn_dist = reinterpret_cast<float*>(w + o_nn_d);
  unsigned char* keep = reinterpret_cast<unsigned char*>(w + o_keep);
  unsigned int* count_dev = reinterpret_cast<unsigned int*>(w + o_count);
  unsigned int* tile_count = reinterpret_cast<unsigned int*>(w + o_tcount);
  unsigned long long* tile_offset = reinterpret_cast<unsigned long long*>(w + o_toffset);
  unsigned long long* total_dev = reinterpret_cast<unsigned long long*>(w + o_total);
  int* match_q = a.match_q ? a.match_q : reinterpret_cast<int*>(w + o_mq);
  int* match_t = a.match_t ? a.match_t : reinterpret_cast<int*>(w + o_mt);
  float* match_d = a.match_d ? a.match_d : reinterpret_cast<float*>(w + o_md);

  // Everything below is enqueued on the stream, then the stream is drained once -- also after a failed enqueue, so that no
  // copy still in flight reads or writes the host vectors of this frame, and no kernel the workspace once it is freed.
  hipStream_t s = a.stream;
  std::vector<unsigned int> counts(B);
  unsigned long long total = 0;
  const char* failed = nullptr;
  auto enqueue = [&]() -> hipError_t {
#define SBA_MATCH_ENQ(expr)                       \
  do {                                            \
    const hipError_t _e = (expr);                 \
    if (_e != hipSuccess) { failed = #expr; return _e; } \
  } while (0)
    SBA_MATCH_ENQ(hipMemcpyAsync(pairs_dev, pairs.data(), sizeof(MatchPair) * B, hipMemcpyHostToDevice, s));
    SBA_MATCH_ENQ(hipMemcpyAsync(qoff_dev, qoff_rel.data(), 8 * (B + 1), hipMemcpyHostToDevice, s));
    SBA_MATCH_ENQ(hipMemcpyAsync(toff_dev, toff_rel.data(), 8 * (B + 1), hipMemcpyHostToDevice, s));
    if (!items.empty())
      SBA_MATCH_ENQ(hipMemcpyAsync(items_dev, items.data(), sizeof(MatchItem) * items.size(), hipMemcpyHostToDevice, s));
    SBA_MATCH_ENQ(hipMemsetAsync(qpack, 0, q_pack * dp * 4, s));
    if (t_pack) {
      SBA_MATCH_ENQ(hipMemsetAsync(tpack, 0, t_pack * dp * 4, s));
      SBA_MATCH_ENQ(hipMemsetAsync(tnorm, 0xff, t_pack * 4, s));        // all-ones: a NaN norm, the padding rows never rank
    }
    SBA_MATCH_ENQ(hipMemsetAsync(keep, 0, ntiles * kCompactTile, s));
    SBA_MATCH_ENQ(hipMemsetAsync(count_dev, 0, 4 * static_cast<size_t>(B), s));
    SBA_MATCH_ENQ(launch_match_pack(a.query, a.stride, a.dim, dp, pairs_dev, B, qoff_dev, total_q, 0, qpack, nullptr, s));
    SBA_MATCH_ENQ(launch_match_pack(a.train, a.stride, a.dim, dp, pairs_dev, B, toff_dev, total_t, 1, tpack, tnorm, s));
    SBA_MATCH_ENQ(launch_match_tiles(dp, qpack, tpack, tnorm, pairs_dev, items_dev, items.size(), static_cast<int>(splits), part, s));
    SBA_MATCH_ENQ(launch_match_finish(a.query, a.train, a.stride, a.dim, a.ratio, pairs_dev, B, qoff_dev, total_q,
                                      static_cast<int>(splits), part, nn_index, nn_dist, keep, count_dev, s));
    SBA_MATCH_ENQ(launch_compact_count(keep, ntiles, tile_count, s));
    SBA_MATCH_ENQ(launch_compact_scan(tile_count, ntiles, tile_offset, total_dev, s));
    SBA_MATCH_ENQ(launch_match_scatter(keep, total_q, ntiles, tile_offset, pairs_dev, B, qoff_dev, nn_index, nn_dist, match_q,
                                       match_t, match_d, a.rows_q, a.rows_t, s));
    if (a.nn_index) SBA_MATCH_ENQ(hipMemcpyAsync(a.nn_index, nn_index, total_q * 2 * sizeof(int), hipMemcpyDeviceToDevice, s));
    if (a.nn_dist) SBA_MATCH_ENQ(hipMemcpyAsync(a.nn_dist, nn_dist, total_q * 2 * sizeof(float), hipMemcpyDeviceToDevice, s));
    SBA_MATCH_ENQ(hipMemcpyAsync(counts.data(), count_dev, 4 * static_cast<size_t>(B), hipMemcpyDeviceToHost, s));
    SBA_MATCH_ENQ(hipMemcpyAsync(&total, total_dev, sizeof(total), hipMemcpyDeviceToHost, s));
#undef SBA_MATCH_ENQ
    return hipSuccess;
  };
  const hipError_t e = enqueue();
  const int rc = stream_wait(s, "descriptor match", a.poisoned);      // the one synchronisation; the workspace lives until here
  if (e != hipSuccess) return set_error(SBA_ERR_HIP, "%s failed: %s", failed, hipGetErrorString(e));
  if (rc) return rc;
  for (int g = 0; g < B; ++g) a.n_matched[g] = counts[g];
  if (a.total) *a.total = static_cast<size_t>(total);
  return SBA_OK;
}

int device_cus(int device, int* cus) {
  SBA_TRY_HIP(hipDeviceGetAttribute(cus, hipDeviceAttributeMultiprocessorCount, device));
  return SBA_OK;
}

// Host arrays of a whole batch -> device copies, the match, the outputs back.  Offsets are rebased to the first row.
int match_host(int device, const float* query, const size_t* qoff, const float* train, const size_t* toff, int num_pairs, int dim,
               size_t stride, float ratio, int* nn_index, float* nn_dist, size_t* n_matched, int* match_query, int* match_train,
               float* match_dist) {
  int rc = require_device(device);
  if (rc) return rc;
  const size_t nq = num_pairs > 0 ? qoff[num_pairs] - qoff[0] : 0, nt = num_pairs > 0 ? toff[num_pairs] - toff[0] : 0;
  for (int g = 0; g < num_pairs; ++g) n_matched[g] = 0;
  if (nq == 0) return SBA_OK;
  std::vector<size_t> q_rel(num_pairs + 1), t_rel(num_pairs + 1);
  for (int g = 0; g <= num_pairs; ++g) { q_rel[g] = qoff[g] - qoff[0]; t_rel[g] = toff[g] - toff[0]; }
  const size_t qbytes = rows_bytes(nq, stride, 4 * dim), tbytes = rows_bytes(nt, stride, 4 * dim);
  DeviceBuffer q_dev, t_dev, out_dev;
  SBA_TRY_HIP(q_dev.alloc(qbytes));
  SBA_TRY_HIP(t_dev.alloc(tbytes));
  SBA_TRY_HIP(out_dev.alloc(nq * (2 * sizeof(int) + 2 * sizeof(float) + 3 * 4)));
  SBA_TRY_HIP(hipMemcpy(q_dev.ptr, reinterpret_cast<const uint8_t*>(query) + qoff[0] * stride, qbytes, hipMemcpyHostToDevice));
  if (tbytes) SBA_TRY_HIP(hipMemcpy(t_dev.ptr, reinterpret_cast<const uint8_t*>(train) + toff[0] * stride, tbytes, hipMemcpyHostToDevice));
  int* nn_i = out_dev.as<int>();
  float* nn_d = reinterpret_cast<float*>(nn_i + 2 * nq);
  int* mq = reinterpret_cast<int*>(nn_d + 2 * nq);
  int* mt = mq + nq;
  float* md = reinterpret_cast<float*>(mt + nq);
  Args a;
  rc = device_cus(device, &a.num_cus);
  if (rc) return rc;
  a.query = q_dev.as<uint8_t>();
  a.train = t_dev.as<uint8_t>();
  a.qoff = q_rel.data();
  a.toff = t_rel.data();
  a.num_pairs = num_pairs;
  a.dim = dim;
  a.stride = stride;
  a.ratio = ratio;
  a.nn_index = nn_index ? nn_i : nullptr;
  a.nn_dist = nn_dist ? nn_d : nullptr;
  a.match_q = mq;
  a.match_t = mt;
  a.match_d = md;
  a.n_matched = n_matched;
  size_t total = 0;
  a.total = &total;
  rc = run(a);
  if (rc) return rc;
  if (nn_index) SBA_TRY_HIP(hipMemcpy(nn_index, nn_i, nq * 2 * sizeof(int), hipMemcpyDeviceToHost));
  if (nn_dist) SBA_TRY_HIP(hipMemcpy(nn_dist, nn_d, nq * 2 * sizeof(float), hipMemcpyDeviceToHost));
  if (total) {
    if (match_query) SBA_TRY_HIP(hipMemcpy(match_query, mq, total * sizeof(int), hipMemcpyDeviceToHost));
    if (match_train) SBA_TRY_HIP(hipMemcpy(match_train, mt, total * sizeof(int), hipMemcpyDeviceToHost));
    if (match_dist) SBA_TRY_HIP(hipMemcpy(match_dist, md, total * sizeof(float), hipMemcpyDeviceToHost));
  }
  return SBA_OK;
}

}  // namespace

int match_pair_on_stream(hipStream_t stream, int* poisoned, int num_cus, const float* query_dev, size_t n_query, const float* train_dev,
                         size_t n_train, int dim, size_t row_stride_bytes, float ratio, int* nn_index_dev, float* nn_dist_dev, size_t* n_matched,
                         int* match_query_dev, int* match_train_dev, float* match_dist_dev) {
  const size_t qoff[2] = {0, n_query}, toff[2] = {0, n_train};
  Args a;
  a.stream = stream;
  a.poisoned = poisoned;
  a.num_cus = num_cus;
  a.query = reinterpret_cast<const uint8_t*>(query_dev);
  a.train = reinterpret_cast<const uint8_t*>(train_dev);
  a.qoff = qoff;
  a.toff = toff;
  a.num_pairs = 1;
  a.dim = dim;
  a.stride = row_stride_bytes;
  a.ratio = ratio;
  a.nn_index = nn_index_dev;
  a.nn_dist = nn_dist_dev;
  a.match_q = match_query_dev;
  a.match_t = match_train_dev;
  a.match_d = match_dist_dev;
  a.n_matched = n_matched;
  return run(a);
}

}  // namespace match
}  // namespace sba

using sba::match::check_keypoint_args;
using sba::match::check_match_args;
using sba::match::check_offsets;
using sba::match::rows_bytes;

extern "C" {

int sba_match_descriptors(int device, const float* query, size_t n_query, const float* train, size_t n_train, int dim,
                          size_t row_stride_bytes, float ratio, int* nn_index, float* nn_dist, size_t* n_matched, int* match_query,
                          int* match_train, float* match_dist) {
  int rc = check_match_args(dim, row_stride_bytes, ratio);
  if (rc) return rc;
  if (!n_matched) return sba::set_error(SBA_ERR_INVALID_ARG, "n_matched is null");
  if ((n_query > 0 && !query) || (n_train > 0 && !train)) return sba::set_error(SBA_ERR_INVALID_ARG, "null descriptor array");
  const size_t qoff[2] = {0, n_query}, toff[2] = {0, n_train};
  return sba::match::match_host(device, query, qoff, train, toff, 1, dim, row_stride_bytes, ratio, nn_index, nn_dist, n_matched,
                                match_query, match_train, match_dist);
}

int sba_match_descriptors_device(int device, void* stream, const float* query_dev, size_t n_query, const float* train_dev,
                                 size_t n_train, int dim, size_t row_stride_bytes, float ratio, int* nn_index_dev,
                                 float* nn_dist_dev, size_t* n_matched, int* match_query_dev, int* match_train_dev,
                                 float* match_dist_dev) {
  int rc = check_match_args(dim, row_stride_bytes, ratio);
  if (rc) return rc;
  if (!n_matched) return sba::set_error(SBA_ERR_INVALID_ARG, "n_matched is null");
  if ((n_query > 0 && !query_dev) || (n_train > 0 && !train_dev))
    return sba::set_error(SBA_ERR_INVALID_ARG, "null descriptor array");
  rc = sba::match::require_device(device);
  if (rc) return rc;
  int num_cus = 0;
  rc = sba::match::device_cus(device, &num_cus);
  if (rc) return rc;
  return sba::match::match_pair_on_stream(static_cast<hipStream_t>(stream), nullptr, num_cus, query_dev, n_query, train_dev, n_train, dim,
                                          row_stride_bytes, ratio, nn_index_dev, nn_dist_dev, n_matched, match_query_dev, match_train_dev,
                                          match_dist_dev);
}

int sba_batch_match_descriptors(int device, const float* query, const size_t* query_offsets, const float* train,
                                const size_t* train_offsets, int num_pairs, int dim, size_t row_stride_bytes, float ratio,
                                int* nn_index, float* nn_dist, size_t* n_matched, int* match_query, int* match_train,
                                float* match_dist) {
  int rc = check_match_args(dim, row_stride_bytes, ratio);
  if (rc) return rc;
  rc = check_offsets(query_offsets, num_pairs, "query");
  if (rc) return rc;
  rc = check_offsets(train_offsets, num_pairs, "train");
  if (rc) return rc;
  if (num_pairs > 0 && !n_matched) return sba::set_error(SBA_ERR_INVALID_ARG, "n_matched is null");
  const size_t nq = num_pairs > 0 ? query_offsets[num_pairs] - query_offsets[0] : 0;
  const size_t nt = num_pairs > 0 ? train_offsets[num_pairs] - train_offsets[0] : 0;
  if ((nq > 0 && !query) || (nt > 0 && !train)) return sba::set_error(SBA_ERR_INVALID_ARG, "null descriptor array");
  if (num_pairs == 0) return sba::match::require_device(device);
  return sba::match::match_host(device, query, query_offsets, train, train_offsets, num_pairs, dim, row_stride_bytes, ratio,
                                nn_index, nn_dist, n_matched, match_query, match_train, match_dist);
}

int sba_problem_upload_matches(sba_problem* p, const void* left_keypoints, size_t n_left, const void* right_keypoints,
                               size_t n_right, size_t stride_bytes, int im_width, int im_height, const float* left_desc,
                               const float* right_desc, int dim, size_t row_stride_bytes, float ratio, const double* init_depth,
                               int store, size_t* n_matched, int* match_left, int* match_right) {
  if (!p) return sba::set_error(SBA_ERR_INVALID_ARG, "null problem handle");
  SBA_REFUSE_POISONED(p);
  if (store != SBA_STORE_F64 && store != SBA_STORE_F32) return sba::set_error(SBA_ERR_INVALID_ARG, "bad store %d", store);
  int rc = check_match_args(dim, row_stride_bytes, ratio);
  if (rc) return rc;
  rc = check_keypoint_args(stride_bytes, im_width, im_height);
  if (rc) return rc;
  if (!n_matched) return sba::set_error(SBA_ERR_INVALID_ARG, "n_matched is null");
  if ((n_left > 0 && (!left_keypoints || !left_desc)) || (n_right > 0 && (!right_keypoints || !right_desc)))
    return sba::set_error(SBA_ERR_INVALID_ARG, "null key-point or descriptor array");
  if (init_depth && !std::isfinite(*init_depth)) return sba::set_error(SBA_ERR_INVALID_ARG, "init_depth is not finite");
  SBA_TRY_HIP(hipSetDevice(p->device));
  *n_matched = 0;

  const size_t qbytes = rows_bytes(n_left, row_stride_bytes, 4 * dim), tbytes = rows_bytes(n_right, row_stride_bytes, 4 * dim);
  sba::DeviceBuffer q_dev(&p->poisoned), t_dev(&p->poisoned), kl(&p->poisoned), kr(&p->poisoned), out(&p->poisoned);
  SBA_TRY_HIP(q_dev.alloc(qbytes));
  SBA_TRY_HIP(t_dev.alloc(tbytes));
  SBA_TRY_HIP(kl.alloc(n_left * stride_bytes));
  SBA_TRY_HIP(kr.alloc(n_right * stride_bytes));
  SBA_TRY_HIP(out.alloc(n_left * (2 * 4 + 2 * 8)));     // match_q, match_t, rows_q, rows_t
  if (qbytes) SBA_TRY_HIP(hipMemcpyAsync(q_dev.ptr, left_desc, qbytes, hipMemcpyHostToDevice, p->stream));
  if (tbytes) SBA_TRY_HIP(hipMemcpyAsync(t_dev.ptr, right_desc, tbytes, hipMemcpyHostToDevice, p->stream));
  if (n_left) SBA_TRY_HIP(hipMemcpyAsync(kl.ptr, left_keypoints, n_left * stride_bytes, hipMemcpyHostToDevice, p->stream));
  if (n_right) SBA_TRY_HIP(hipMemcpyAsync(kr.ptr, right_keypoints, n_right * stride_bytes, hipMemcpyHostToDevice, p->stream));
  unsigned long long* rows_q = out.as<unsigned long long>();
  unsigned long long* rows_t = rows_q + n_left;
  int* mq = reinterpret_cast<int*>(rows_t + n_left);
  int* mt = mq + n_left;

  const size_t qoff[2] = {0, n_left}, toff[2] = {0, n_right};
  sba::match::Args a;
  a.stream = p->stream;
  a.poisoned = &p->poisoned;
  a.num_cus = p->num_cus;
  a.query = q_dev.as<uint8_t>();
  a.train = t_dev.as<uint8_t>();
  a.qoff = qoff;
  a.toff = toff;
  a.num_pairs = 1;
  a.dim = dim;
  a.stride = row_stride_bytes;
  a.ratio = ratio;
  a.match_q = mq;
  a.match_t = mt;
  a.rows_q = rows_q;
  a.rows_t = rows_t;
  size_t m = 0;
  a.n_matched = &m;
  rc = sba::match::run(a);
  if (rc) return rc;

  // sba_problem_upload_keypoints of the matched records, with the records gathered on the device
  rc = sba::shim::alloc_planes(p, m, init_depth != nullptr, store);
  if (rc) return rc;
  if (m > 0) {
    SBA_TRY_HIP(sba::launch_keypoints_to_planes_gather(kl.as<uint8_t>(), kr.as<uint8_t>(), rows_q, rows_t, m, stride_bytes,
                                                       im_width, im_height, p->coord, store, p->stream));
    if (match_left) SBA_TRY_HIP(hipMemcpyAsync(match_left, mq, m * sizeof(int), hipMemcpyDeviceToHost, p->stream));
    if (match_right) SBA_TRY_HIP(hipMemcpyAsync(match_right, mt, m * sizeof(int), hipMemcpyDeviceToHost, p->stream));
    rc = sba::stream_wait(p->stream, "stream synchronisation", &p->poisoned);
    if (rc) return rc;
  }
  p->uploaded = true;
  *n_matched = m;
  if (init_depth) {      // the reference's init_d fill (spherical_bundle_adjuster.cpp:325-326): d12 = (d, d) per match
    std::vector<double> d12(2 * std::max<size_t>(m, 1), *init_depth);
    return sba_problem_set_depths(p, d12.data());
  }
  return SBA_OK;
}

int sba_batch_upload_matches(sba_batch* b, const void* left_keypoints, const size_t* left_offsets, const void* right_keypoints,
                             const size_t* right_offsets, int num_pairs, size_t stride_bytes, int im_width, int im_height,
                             const float* left_desc, const float* right_desc, int dim, size_t row_stride_bytes, float ratio,
                             const double* init_depth, int store, size_t* n_matched, int* match_left, int* match_right) {
  if (!b) return sba::set_error(SBA_ERR_INVALID_ARG, "null batch handle");
  SBA_REFUSE_POISONED(b);
  if (store != SBA_STORE_F64 && store != SBA_STORE_F32) return sba::set_error(SBA_ERR_INVALID_ARG, "bad store %d", store);
  int rc = check_match_args(dim, row_stride_bytes, ratio);
  if (rc) return rc;
  rc = check_keypoint_args(stride_bytes, im_width, im_height);
  if (rc) return rc;
  rc = check_offsets(left_offsets, num_pairs, "left");
  if (rc) return rc;
  rc = check_offsets(right_offsets, num_pairs, "right");
  if (rc) return rc;
  if (num_pairs > 0 && !n_matched) return sba::set_error(SBA_ERR_INVALID_ARG, "n_matched is null");
  const size_t nl = num_pairs > 0 ? left_offsets[num_pairs] - left_offsets[0] : 0;
  const size_t nr = num_pairs > 0 ? right_offsets[num_pairs] - right_offsets[0] : 0;
  if ((nl > 0 && (!left_keypoints || !left_desc)) || (nr > 0 && (!right_keypoints || !right_desc)))
    return sba::set_error(SBA_ERR_INVALID_ARG, "null key-point or descriptor array");
  if (init_depth)
    for (int g = 0; g < num_pairs; ++g)
      if (!std::isfinite(init_depth[g])) return sba::set_error(SBA_ERR_INVALID_ARG, "init_depth[%d] is not finite", g);
  SBA_TRY_HIP(hipSetDevice(b->device));

  std::vector<size_t> l_rel(num_pairs + 1, 0), r_rel(num_pairs + 1, 0);
  for (int g = 0; num_pairs > 0 && g <= num_pairs; ++g) { l_rel[g] = left_offsets[g] - left_offsets[0]; r_rel[g] = right_offsets[g] - right_offsets[0]; }
  const size_t l0 = num_pairs > 0 ? left_offsets[0] : 0, r0 = num_pairs > 0 ? right_offsets[0] : 0;
  const size_t qbytes = rows_bytes(nl, row_stride_bytes, 4 * dim), tbytes = rows_bytes(nr, row_stride_bytes, 4 * dim);
  sba::DeviceBuffer q_dev(&b->poisoned), t_dev(&b->poisoned), kl(&b->poisoned), kr(&b->poisoned), out(&b->poisoned);
  SBA_TRY_HIP(q_dev.alloc(qbytes));
  SBA_TRY_HIP(t_dev.alloc(tbytes));
  SBA_TRY_HIP(kl.alloc(nl * stride_bytes));
  SBA_TRY_HIP(kr.alloc(nr * stride_bytes));
  SBA_TRY_HIP(out.alloc(nl * (2 * 4 + 2 * 8 + 3 * 8)));   // match_q, match_t, rows_q, rows_t, one side's points
  const uint8_t* ld = reinterpret_cast<const uint8_t*>(left_desc), *rd = reinterpret_cast<const uint8_t*>(right_desc);
  const uint8_t* lk = static_cast<const uint8_t*>(left_keypoints), *rk = static_cast<const uint8_t*>(right_keypoints);
  if (qbytes) SBA_TRY_HIP(hipMemcpyAsync(q_dev.ptr, ld + l0 * row_stride_bytes, qbytes, hipMemcpyHostToDevice, b->stream));
  if (tbytes) SBA_TRY_HIP(hipMemcpyAsync(t_dev.ptr, rd + r0 * row_stride_bytes, tbytes, hipMemcpyHostToDevice, b->stream));
  if (nl) SBA_TRY_HIP(hipMemcpyAsync(kl.ptr, lk + l0 * stride_bytes, nl * stride_bytes, hipMemcpyHostToDevice, b->stream));
  if (nr) SBA_TRY_HIP(hipMemcpyAsync(kr.ptr, rk + r0 * stride_bytes, nr * stride_bytes, hipMemcpyHostToDevice, b->stream));
  unsigned long long* rows_q = out.as<unsigned long long>();
  unsigned long long* rows_t = rows_q + nl;
  double* xyz = reinterpret_cast<double*>(rows_t + nl);
  int* mq = reinterpret_cast<int*>(xyz + 3 * nl);
  int* mt = mq + nl;

  std::vector<size_t> counts(std::max(num_pairs, 1), 0);
  size_t m = 0;
  if (num_pairs > 0) {
    sba::match::Args a;
    a.stream = b->stream;
    a.poisoned = &b->poisoned;
    a.num_cus = b->num_cus;
    a.query = q_dev.as<uint8_t>();
    a.train = t_dev.as<uint8_t>();
    a.qoff = l_rel.data();
    a.toff = r_rel.data();
    a.num_pairs = num_pairs;
    a.dim = dim;
    a.stride = row_stride_bytes;
    a.ratio = ratio;
    a.match_q = mq;
    a.match_t = mt;
    a.rows_q = rows_q;
    a.rows_t = rows_t;
    a.n_matched = counts.data();
    a.total = &m;
    rc = sba::match::run(a);
    if (rc) return rc;
  }

  // sba_batch_upload of sba_keypoints_to_sphere of the matched records: offsets = exclusive scan of the counts
  std::vector<size_t> offsets(num_pairs + 1, 0);
  for (int g = 0; g < num_pairs; ++g) offsets[g + 1] = offsets[g] + counts[g];
  rc = sba::batch::free_batch_data(b);
  if (rc) return rc;
  rc = sba::batch::layout_pairs(b, offsets.data(), num_pairs, store, init_depth != nullptr);
  if (rc) return rc;
  if (m > 0) {
    const size_t ppt = static_cast<size_t>(sba::points_per_lane(store));
    const uint8_t* kp[2] = {kl.as<uint8_t>(), kr.as<uint8_t>()};
    const unsigned long long* rows[2] = {rows_q, rows_t};
    for (int side = 0; side < 2; ++side) {      // stream order: the right side's gather waits for the left side's re-layout
      SBA_TRY_HIP(sba::launch_keypoints_to_sphere_gather(kp[side], rows[side], m, stride_bytes, im_width, im_height, xyz, b->stream));
      SBA_TRY_HIP(sba::launch_batch_aos_to_planes(xyz, m, 0, b->offsets_dev, num_pairs, b->desc_dev, ppt, b->coord[3 * side],
                                                  b->coord[3 * side + 1], b->coord[3 * side + 2], store, b->stream));
    }
    if (match_left) SBA_TRY_HIP(hipMemcpyAsync(match_left, mq, m * sizeof(int), hipMemcpyDeviceToHost, b->stream));
    if (match_right) SBA_TRY_HIP(hipMemcpyAsync(match_right, mt, m * sizeof(int), hipMemcpyDeviceToHost, b->stream));
  }
  rc = sba::stream_wait(b->stream, "batch upload", &b->poisoned);
  if (rc) return rc;
  b->uploaded = true;
  for (int g = 0; g < num_pairs; ++g) n_matched[g] = counts[g];
  if (init_depth && num_pairs > 0) {
    std::vector<double> d12(2 * std::max<size_t>(m, 1));
    for (int g = 0; g < num_pairs; ++g)
      for (size_t i = offsets[g]; i < offsets[g + 1]; ++i) d12[2 * i] = d12[2 * i + 1] = init_depth[g];
    return sba_batch_set_depths(b, d12.data());
  }
  return SBA_OK;
}

}  // extern "C"
