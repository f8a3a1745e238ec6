// Exact L2 2-nearest-neighbour matching of f32 descriptors with the reference's ratio test (kernels:
// sba_match_kernels.hip; entry points: sba_match.cpp).  DESIGN.md section 3.10.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace sba {

// One pair of descriptor sets.  Rows are absolute rows of the caller's arrays; q_out0 is the pair's first row of the
// concatenated per-query outputs.  The packed copies start every pair on a whole block of queries and a whole tile of
// train rows.
struct MatchPair {
  unsigned long long q_row0, t_row0;
  unsigned long long q_out0;
  unsigned long long q_pack, t_pack;
  unsigned int nq, nt;
  unsigned int t_tiles;   // ceil(nt / kMatchTile)
  unsigned int pad_;
};
// One block of the product kernel: query block `qblock` of pair `pair` against split `split` of its train tiles.
struct MatchItem {
  unsigned int pair, qblock, split, pad_;
};

constexpr int kMatchTile = 32;    // train rows per MFMA tile (the 32x32 A operand)
constexpr int kMatchBlock = 256;  // threads of the product kernel (4 waves)

// Padded dimension of the packed rows: 64, 128 or 256 (the product kernel's variants); 0 if dim is out of range.
inline int match_padded_dim(int dim) { return dim < 1 ? 0 : dim <= 64 ? 64 : dim <= 128 ? 128 : dim <= 256 ? 256 : 0; }
// Queries per block of the product kernel: 4 waves x 32 queries x (2 query tiles, 1 at 256).
inline int match_query_block(int dp) { return 4 * 32 * (dp == 256 ? 1 : 2); }

// Packs rows [0, total_rows) of one side (concatenated pair rows: pair g = rows off_rel[g] .. off_rel[g + 1]) into
// [row][dp] f32, zero beyond dim: the query side scaled by -2 (exact), the train side unscaled with norm[row] = the fmaf
// chain of its squares in k order, NaN for a row with a non-finite component.
hipError_t launch_match_pack(const uint8_t* src, size_t stride_bytes, int dim, int dp, const MatchPair* pairs, int num_pairs,
                             const unsigned long long* off_rel, size_t total_rows, int side, float* pack, float* norm,
                             hipStream_t stream);
// The dot products on the f32 MFMA and the per-lane top-2 of (score, index): part[(packed query row) * splits + split]
// = (score0, index0, score1, index1), index -1 = none.
hipError_t launch_match_tiles(int dp, const float* qpack, const float* tpack, const float* tnorm, const MatchPair* pairs,
                              const MatchItem* items, size_t n_items, int splits, float4* part, hipStream_t stream);
// Per query row: merge of the per-split lists, rescoring of the two winners, the ratio test.  nn_index / nn_dist [rows][2],
// keep[row] = 1 for an accepted query (keep beyond total_rows stays as it is: zero), pair_count[g] += accepted queries.
hipError_t launch_match_finish(const uint8_t* query, const uint8_t* train, size_t stride_bytes, int dim, float ratio,
                               const MatchPair* pairs, int num_pairs, const unsigned long long* qoff_rel, size_t total_rows,
                               int splits, const float4* part, int* nn_index, float* nn_dist, unsigned char* keep,
                               unsigned int* pair_count, hipStream_t stream);
// Stable scatter of the accepted queries (keep, tile offsets of launch_compact_scan) to (query, train, distance) with
// pair-local indices; rows_q / rows_t (may be null): the absolute rows of the caller's arrays, for the key-point gather.
hipError_t launch_match_scatter(const unsigned char* keep, size_t total_rows, size_t ntiles,
                                const unsigned long long* tile_offset, const MatchPair* pairs, int num_pairs,
                                const unsigned long long* qoff_rel, const int* nn_index, const float* nn_dist, int* match_q,
                                int* match_t, float* match_d, unsigned long long* rows_q, unsigned long long* rows_t,
                                hipStream_t stream);

namespace match {
// The code behind sba_match_descriptors_device, for a caller with a stream and a handle of its own (sba_match.cpp): one pair of
// device arrays, the checks done by the caller; a wait that gives up sets *poisoned (may be null).  One synchronisation: the count.
int match_pair_on_stream(hipStream_t stream, int* poisoned, int num_cus, const float* query_dev, size_t n_query, const float* train_dev,
                         size_t n_train, int dim, size_t row_stride_bytes, float ratio, int* nn_index_dev, float* nn_dist_dev, size_t* n_matched,
                         int* match_query_dev, int* match_train_dev, float* match_dist_dev);
}  // namespace match

// sba_side.hip: the pixel -> unit sphere maps of key-point records picked by absolute row (rows[i] * stride_bytes).
hipError_t launch_keypoints_to_planes_gather(const uint8_t* kp_left, const uint8_t* kp_right, const unsigned long long* rows_left,
                                             const unsigned long long* rows_right, size_t n, size_t stride_bytes, double im_w,
                                             double im_h, void* const planes[6], int store, hipStream_t stream);
hipError_t launch_keypoints_to_sphere_gather(const uint8_t* kp, const unsigned long long* rows, size_t n, size_t stride_bytes,
                                             double im_w, double im_h, double* out_xyz, hipStream_t stream);

}  // namespace sba
