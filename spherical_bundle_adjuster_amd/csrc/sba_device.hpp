// Internal interface between the C-ABI translation units (sba_shim / sba_transport / sba_stages / sba_batch .cpp) and the HIP kernels
// (sba_kernels.hip, sba_batch_kernels.hip, sba_side.hip, sba_depth.hip, sba_epipolar.hip).  Nothing here is exported.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>

#include "../../include/sba_hip.h"
#include "sba_depth_solver.hpp"
#include "sba_joint_solver.hpp"
#include "sba_rotation.hpp"

namespace sba {

// Wave-uniform state of one sweep, passed BY VALUE as a kernel argument (kernarg segment ->
// scalar loads), staged in LDS by the kernel prologue.
//   uniform depths  : Rn = -d1 * R,  Gn_j = -d1 * dR/dw_j   (d1 folded in on the host)
//   per-match depths: Rn = -R,       Gn_j = -dR/dw_j        (d1_i applied per match: X1 = d1_i x1, X2 = d2_i x2)
// so that  e = t + d2 x2 + Rn [d1_i] x1   and   A = d(e)/d(rot) = [Gn_0 X1 | Gn_1 X1 | Gn_2 X1].
struct SweepParams {
  double Rn[9];
  double Gn[27];   // Gn[9*j + 3*r + c]
  double t[3];
  double d2;       // uniform depth of the right point (unused with per-match depths)
  double delta;    // Huber a; <= 0: no robustifier
  double delta2;   // a*a
  unsigned long long n;  // correspondences in this shard
};
static_assert(sizeof(SweepParams) == 43 * 8, "SweepParams layout");

// Per-sweep state from (rot, tran, depths, delta).  depth_mode: 0 = uniform (d1 folded into Rn / Gn), 1 = per match.
// with_derivatives = false (the factored kernel never reads Gn): Gn is zeroed, d R / d w is not formed.
SBA_HD inline void fill_sweep_params(unsigned long long n, int depth_mode, const double rot[3], const double tran[3],
                                     double d1, double d2, double huber_delta, SweepParams* prm,
                                     bool with_derivatives = true) {
  double R[9], G[27];
  rotation_and_derivatives(rot, R, with_derivatives ? G : nullptr);
  const double scale = depth_mode == 0 ? -d1 : -1.0;
  for (int i = 0; i < 9; ++i) prm->Rn[i] = scale * R[i];
  for (int i = 0; i < 27; ++i) prm->Gn[i] = with_derivatives ? scale * G[i] : 0.0;
  for (int i = 0; i < 3; ++i) prm->t[i] = tran[i];
  prm->d2 = d2;
  prm->delta = huber_delta > 0.0 ? huber_delta : 0.0;
  prm->delta2 = prm->delta * prm->delta;
  prm->n = n;
}

// Device-resident correspondences as planes (structure of arrays): every lane of a wave reads
// 16 consecutive bytes of one plane, so each wave load instruction covers 1 KiB contiguous.
struct Planes {
  const void* x1[3];  // left unit vectors  x, y, z   (double or float per `store`; folded sweeps: X1 = d1 x1)
  const void* x2[3];  // right unit vectors x, y, z                               (folded sweeps: X2 = d2 x2)
  const double* d1;   // per-match depths (always f64), may be null
  const double* d2;
};

// Determinant a d - b^2 of a match's damped 2 x 2 depth block (joint_block, depth_stream), as Kahan's difference of products:
// the rounding error of b * b is added back, so the result is within 1.5 ulp of the true value and EXACTLY 0 for an exactly
// singular block (a == d == |b|: parallel rays whose damping D / radius fell below half an ulp of the block).  The plain
// a * d - b * b is contracted to fma(a, d, -(b * b)) and leaves that rounding error as the "determinant": 1e-17 of a^2 with
// either sign, a finite reciprocal and a finite, meaningless reduced system or step where the host's step logic is written
// for a non-finite one (a failed Cholesky factorisation, a model that is not > 0: an invalid step).
#if defined(__HIPCC__)
__device__ __forceinline__ double depth_block_det(double a, double d, double b) {
  double w;
  {
#pragma clang fp contract(off)
    w = b * b;
  }
  const double err = __builtin_fma(-b, b, w);      // w - b * b, exact
  return __builtin_fma(a, d, -w) + err;
}
#endif

constexpr int kPackSize = 24;
constexpr int kRow = 32;   // doubles per block-partial row (256 B: two whole 128-byte lines, 24 used)
#ifndef SBA_BLOCK
#define SBA_BLOCK 256
#endif
constexpr int kBlock = SBA_BLOCK;   // threads per sweep block (multiple of 64)

// Sweep: residual + Jacobian + Huber + reduction of every block's partial pack into
// partials[grid][24]; then finalize() folds the partials in a fixed order into pack_out[24].
// Where a sweep leaves its result.  ticket == nullptr: only partials[grid][kRow] are written and
// launch_finalize() must follow.  Otherwise the last-arriving block folds the partials into pack_dev[24] and, if
// pack_host != nullptr (device-visible address of mapped pinned memory, >= 26 doubles), also stores the pack there
// followed by `seq` at pack_host[24] (as a 64-bit integer) for the host to poll.  ticket: 9 counters, one per
// 64-byte line (ticket[16*k]), zero before the first launch; the kernel re-zeroes them.
struct SweepOut {
  double* partials;
  double* pack_dev;
  double* pack_host;
  unsigned int* ticket;
  unsigned long long seq;
};

constexpr int kDepthFolded = 2;   // launch_sweep's depth for per-match depths folded into f64 coordinate planes
// kind: 0 = factored (moment pack, host applies J_l), 1 = explicit per-match Jacobian (SBA_PACK layout).
// depth: 0 uniform, 1 per match (8 planes), 2 per match folded into the coordinates (6 f64 planes, store 0 only).
hipError_t launch_sweep(int mode, int depth, int store, int kind, const Planes& pl, const SweepParams& prm,
                        const SweepOut& out, int grid, hipStream_t stream);
hipError_t sweep_blocks_per_cu(int mode, int depth, int store, int kind, bool loss, int* blocks);
// Direct peer exchange (all-reduce of the pack over IPC-mapped inboxes, see peer_exchange_kernel).
constexpr int kMaxPeers = 8;
constexpr size_t kInboxDoubles = 2 * kMaxPeers * 32;   // [parity][source rank][32] = 4 KiB per rank
struct PeerInboxes {
  double* inbox[kMaxPeers];   // device-visible address of every rank's inbox (index = rank, own included)
  int nranks;
  int rank;
  unsigned long long timeout_ticks;   // longest wait for a peer's slot, in ticks of the constant-rate wall clock
                                      // (wall_clock64, hipDeviceAttributeWallClockRate) -- time, not loop iterations
  unsigned long long* sticky;         // device word, set to 1 by any exchange that timed out and never cleared: a
                                      // later exchange of the same burst publishes it, so no timeout goes unseen
};
hipError_t launch_peer_exchange(const double* pack_local, const PeerInboxes& px, unsigned long long xseq,
                                double* pack_out, double* pack_host_dev, unsigned long long host_seq,
                                hipStream_t stream);
// Folds partials[nblocks][kRow] into pack_out[24].  px != nullptr: the same launch then all-reduces the pack across
// ranks (peer exchange, sequence number xseq).  pack_host_dev != nullptr: ... and publishes it to mapped pinned host
// memory followed by `seq` at [24] for the host to poll.
hipError_t launch_finalize(const double* partials, int nblocks, double* pack_out, double* pack_host_dev,
                           unsigned long long seq, const PeerInboxes* px, unsigned long long xseq,
                           hipStream_t stream);

// pack_dev[24] -> mapped pinned host memory, then `seq` at pack_host[24] (64-bit) for the host to poll.
hipError_t launch_publish(const double* pack_dev, double* pack_host_dev, unsigned long long seq,
                          hipStream_t stream);

// Batched problems (config C5): pair g owns vectors [first_vec, first_vec + ceil(n/PPT)) of the shared planes and
// params[g] (its own R|t; params[g].n = 0 skips the pair).  bpp blocks per pair; partials [num_pairs*bpp][kRow];
// packs [num_pairs][24] in the selected kernel's layout.
// Vector p of a pair (p = 0, 1, ...: 16 bytes of every coordinate plane) sits at plane vector
//     first_vec + (p / 256) * tile_stride + (p % 256):
// tile_stride = 256: the pair's vectors are contiguous; tile_stride = 256 * num_pairs, first_vec = 256 * pair: the pairs are
// INTERLEAVED in 4 KiB tiles (tile t of every pair side by side), so that blocks that sweep their own pairs in step with one
// another read one contiguous window of every plane -- the access pattern of the single-problem grid-stride sweep -- instead of
// num_pairs x 8 separate sequential streams.
struct PairDesc {
  unsigned long long first_vec;
  unsigned long long n;
  unsigned long long tile_stride;
  unsigned long long pad_;
};
constexpr unsigned long long kPairTile = 256;   // vectors per tile = threads per sweep block
SBA_HD inline unsigned long long pair_vector(const PairDesc& d, unsigned long long p) {
  return d.first_vec + (p / kPairTile) * d.tile_stride + (p % kPairTile);
}
// tile_elems == 0: element i -> first + i.  Otherwise (interleaved batch layout, PairDesc): tiles of tile_elems consecutive
// elements sit tile_stride_elems apart.
SBA_HD inline size_t tiled_index(size_t first, size_t i, size_t tile_elems, size_t tile_stride_elems) {
  return tile_elems == 0 ? first + i : first + (i / tile_elems) * tile_stride_elems + i % tile_elems;
}
// The pair of row `row` of a batch's concatenated rows (pair g = rows offsets[g] .. offsets[g + 1]), by bisection of the
// offsets (a few KB, L2-resident); empty pairs repeat an offset: the last one wins.
SBA_HD inline int batch_pair_of(size_t row, const unsigned long long* __restrict__ offsets, int num_pairs) {
  int lo = 0, hi = num_pairs;                 // offsets[lo] <= row < offsets[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (offsets[mid] <= row) lo = mid; else hi = mid;
  }
  return lo;
}
// Element index of element `i` of pair `d` inside the planes (ppt elements per 16-byte vector).
SBA_HD inline size_t pair_element(const PairDesc& d, size_t i, size_t ppt) {
  return tiled_index(d.first_vec * ppt, i, kPairTile * ppt, d.tile_stride * ppt);
}
// Row -> element of the pair's tiles.
SBA_HD inline size_t batch_row_index(size_t row, const unsigned long long* __restrict__ offsets, int num_pairs,
                                     const PairDesc* __restrict__ desc, size_t ppt) {
  const int g = batch_pair_of(row, offsets, num_pairs);
  return pair_element(desc[g], row - offsets[g], ppt);
}
// What the host hands over per pair and step (mapped pinned host memory, 80 B per pair): the point to evaluate at and
// the number of matches that take part (0 = pair already converged).
struct BatchState {
  double rot[3], tran[3];
  double d1, d2;
  unsigned long long n;
  unsigned long long pad_;
};
static_assert(sizeof(BatchState) == 80, "BatchState is copied word by word");
// The same step in ONE launch, for batches with one block per pair (bpp == 1): every block prepares its own pair's
// state, sweeps, folds, converts and publishes its pack; the last one stores `seq` at packs_host[24 * num_pairs].
// ticket: one zeroed device word.
hipError_t launch_batch_step_fused(int mode, int depth, int store, int kind, double huber_delta, const Planes& pl,
                                   const BatchState* state, const PairDesc* desc, int num_pairs, double* packs,
                                   double* packs_host, unsigned int* ticket, unsigned long long seq, hipStream_t stream);

// In / out record of one pair for the one-launch per-pair solve (batch_lm_kernel): start point and uniform depths in,
// result, summary and status out.
struct BatchLmIo {
  double rot[3], tran[3];
  double d1, d2;
  sba_lm_summary summary;
  int status;
  int pad_;
};
// ticket: one zeroed device word; seq_host_dev (may be null): device-visible address of a host word that receives `seq`
// once every pair's record has been written.
// sweep_cap / cont_*: with cont_state != nullptr the kernel runs at most sweep_cap sweeps per pair; a pair that needs more
// leaves its solver (cont_state[pair], batch_lm_dyn_state_bytes() each), the state of its next sweep (cont_params / cont_frames)
// and cont_done[pair] = 0 behind, and its record says pad_ = 1; the launches with dynamic shares below take over.
hipError_t launch_batch_lm(int mode, int depth, int store, int kind, const Planes& pl, const PairDesc* desc,
                           BatchLmIo* io, const sba_lm_options& opt, int num_pairs, unsigned int* ticket,
                           unsigned long long* seq_host_dev, unsigned long long seq, hipStream_t stream, int sweep_cap = 0,
                           void* cont_state = nullptr, SweepParams* cont_params = nullptr, double* cont_frames = nullptr,
                           int* cont_done = nullptr);
hipError_t batch_blocks_per_cu(int mode, int depth, int store, int kind, bool loss, int* blocks);
// Device-resident per-pair solves with DYNAMIC shares (sba_batch_kernels.hip, sba_depth.hip): every iteration / pass is a
// sweep launch whose blocks are dealt out to the pairs that are still iterating, a per-pair step launch and a compaction
// launch -- all enqueued without waiting; pairs that have converged hand their CUs to the others.
struct BatchDynCtl { unsigned int nactive[2]; unsigned int pad_[2]; };
// Shares per active pair of a launch of `grid` blocks: grid / nactive (1 when there are at least as many pairs as blocks).
// Measured alternative: ceil(4 * grid / nactive) shares, several work items per block -- no block idle at 129 ... 255 active
// pairs, but every item pays its own fold and row and the per-pair step folds more rows: rot-only stage 2.50 -> 3.28 ms, d-only
// 7.0 -> 7.5 ms at C5 on the same box (profiles/r03c_dyn_shares_ab.log).  Rows of a launch: nactive * shares <= grid + nactive.
constexpr unsigned kDynOver = 1;
SBA_HD inline unsigned dyn_shares(unsigned nactive, unsigned grid) { return nactive == 0u || nactive >= grid ? 1u : grid / nactive; }
size_t batch_lm_dyn_state_bytes();
hipError_t launch_batch_dyn_first_list(BatchDynCtl* ctl, unsigned int* active, const int* done, int num_pairs, hipStream_t stream);
hipError_t launch_batch_lm_dyn_init(int mode, int depth, int kind, const PairDesc* desc, const BatchLmIo* io, const sba_lm_options& opt,
                                    int num_pairs, void* state, SweepParams* params, double* frames, BatchDynCtl* ctl,
                                    unsigned int* active, int* done, hipStream_t stream);
hipError_t launch_batch_lm_dyn_pass(int mode, int depth, int store, int kind, const Planes& pl, const PairDesc* desc,
                                    const sba_lm_options& opt, int num_pairs, int parity, int sweep_grid, void* state,
                                    SweepParams* params, double* frames, BatchDynCtl* ctl, unsigned int* active, int* done,
                                    double* partials, BatchLmIo* io, unsigned long long* host_words, unsigned long long seq,
                                    hipStream_t stream);

hipError_t launch_batch_sweep(int mode, int depth, int store, int kind, bool loss, const Planes& pl,
                              const SweepParams* params, const PairDesc* desc, int num_pairs, int bpp,
                              double* partials, double* packs, double* packs_host, unsigned long long seq,
                              hipStream_t stream);
// Same, with the per-pair preparation and conversion on the device: batch_prepare_kernel builds every pair's
// SweepParams (and, for the factored kernel, the frame (B, J) of its rotation) from `state`; batch_finalize_kernel folds
// the rows and maps the factored kernel's moments to the SBA_PACK_* layout before publishing.
hipError_t launch_batch_sweep_only(int mode, int depth, int store, int kind, bool loss, const Planes& pl,
                                   const SweepParams* params, const PairDesc* desc, int num_pairs, int bpp,
                                   double* partials, hipStream_t stream);
hipError_t launch_batch_step(int mode, int depth, int store, int kind, double huber_delta, const Planes& pl,
                             const BatchState* state, SweepParams* params, double* frames, const PairDesc* desc,
                             int num_pairs, int bpp, double* partials, double* packs, double* packs_host,
                             unsigned long long seq, hipStream_t stream);

// AoS (cv::Point3d layout, double[3n]) -> planes, element offset `first`, count `n`.  tile_stride_elems != 0 (batched,
// interleaved layout): element i goes to first + (i / tile_elems) * tile_stride_elems + i % tile_elems.
hipError_t launch_aos_to_planes(const double* aos, size_t n, size_t first, void* px, void* py,
                                void* pz, int store, hipStream_t stream, size_t tile_elems = 0, size_t tile_stride_elems = 0);
// d12 (double[2n]) -> two f64 planes.
hipError_t launch_d12_to_planes(const double* d12, size_t n, size_t first, double* d1, double* d2,
                                hipStream_t stream, size_t tile_elems = 0, size_t tile_stride_elems = 0);
// A chunk of the CONCATENATED arrays of a batch (rows first_row .. first_row + m, relative to the batch's first row) to its
// places in the pairs' tiles, one launch: offsets_dev[num_pairs + 1] = first row of every pair (relative likewise).
hipError_t launch_batch_aos_to_planes(const double* aos, size_t m, size_t first_row, const unsigned long long* offsets_dev,
                                      int num_pairs, const PairDesc* desc, size_t ppt, void* px, void* py, void* pz, int store,
                                      hipStream_t stream);
hipError_t launch_batch_d12_to_planes(const double* d12, size_t m, size_t first_row, const unsigned long long* offsets_dev,
                                      int num_pairs, const PairDesc* desc, size_t ppt, double* d1, double* d2,
                                      hipStream_t stream);
hipError_t launch_planes_to_d12(const double* d1, const double* d2, size_t n, double* d12,
                                hipStream_t stream);
// f64 planes of `elems` elements (a multiple of 2): folded[0..2] = d1 * coord[0..2], folded[3..5] = d2 * coord[3..5].
// grid_cap: most blocks of 256 threads (grid-stride beyond).
hipError_t launch_fold_depths(const void* const coord[6], const double* d1, const double* d2, double* const folded[6],
                              size_t elems, int grid_cap, hipStream_t stream);

// Per-match residuals (sba_select.hip: residual_kernel).  e [elems][3], sq [elems], inlier [elems]: whole vectors of the
// planes' element type (f64: 2 matches, f32: 4), written only where `outputs` (bit 0 e, bit 1 sq, bit 2 inlier) asks;
// n_inlier: one zeroed device word that receives the inlier count.  depth as for launch_sweep.
struct ResidualOut {
  double* e;
  double* sq;
  unsigned char* inlier;
  unsigned long long* n_inlier;
};
hipError_t launch_residuals(int depth, int store, int outputs, const Planes& pl, const SweepParams& prm,
                            const ResidualOut& out, int grid, hipStream_t stream);
// Stable compaction of a single problem's planes (sba_select.hip).  keep: ntiles * kCompactTile bytes, zero beyond n.
// count: tile_count[ntiles]; scan (one block): tile_offset[ntiles] exclusive, total[0] = kept matches; scatter: every kept
// match i of src[c] to dst[c][tile_offset + rank] (c < 6 coordinate planes of the store's type, 6 and 7 the f64 depth
// planes when src[6] != null), kept_index (may be null) receives i.
constexpr int kCompactTile = 2048;   // matches per scan tile: 8 rounds of one 256-thread block
struct CompactArgs {
  const unsigned char* keep;
  size_t n;
  const unsigned long long* tile_offset;
  const void* src[8];
  void* dst[8];
  long long* kept_index;
};
hipError_t launch_compact_count(const unsigned char* keep, size_t ntiles, unsigned int* tile_count, hipStream_t stream);
hipError_t launch_compact_scan(const unsigned int* tile_count, size_t ntiles, unsigned long long* tile_offset,
                               unsigned long long* total, hipStream_t stream);
hipError_t launch_compact_scatter(int store, const CompactArgs& args, size_t ntiles, hipStream_t stream);

// The same two for a batch (sba_select.hip).  Residuals: pair g (blocks g * bpp ... g * bpp + bpp - 1, strided over its
// vectors as the batched sweep) builds its SweepParams on the device from state[g] (fill_sweep_params, as the step kernels
// do) and writes the outputs `outputs` asks for to rows offsets[g] + i (e [rows][3], sq [rows], inlier [rows]: element by
// element); n_inlier: num_pairs zeroed device words.
hipError_t launch_batch_residuals(int depth, int store, int outputs, const Planes& pl, const PairDesc* desc,
                                  const unsigned long long* offsets, const BatchState* state, double huber_delta,
                                  int num_pairs, int bpp, const ResidualOut& out, hipStream_t stream);
// Compaction: keep as for a single problem, over the concatenated rows (tile counts and scan: launch_compact_count / _scan);
// pair_kept[g] = kept rows of pair g (one wave per pair, from the tile offsets); the scatter moves every kept row from its
// element of the old layout (old_offsets, old_desc) to its element of the new one.  Offsets relative to the first row.
struct BatchCompactArgs {
  const unsigned char* keep;
  size_t rows;
  const unsigned long long* tile_offset;
  const unsigned long long* old_offsets;
  const PairDesc* old_desc;
  const unsigned long long* new_offsets;
  const PairDesc* new_desc;
  int num_pairs;
  const void* src[8];
  void* dst[8];
  long long* kept_index;
};
hipError_t launch_batch_pair_kept(const unsigned char* keep, const unsigned long long* tile_offset, size_t ntiles,
                                  const unsigned long long* total, const unsigned long long* offsets, int num_pairs,
                                  unsigned long long* pair_kept, hipStream_t stream);
hipError_t launch_batch_compact_scatter(int store, const BatchCompactArgs& args, size_t ntiles, hipStream_t stream);

// d-only stage (spherical_bundle_adjuster.cpp:1004-1063): one LM iteration of the global bounded problem.
struct DepthParams {
  double R[9];
  double t[3];
  double lambda, c;
  double radius, inv_radius;
  double min_diagonal, max_diagonal;
  double alpha;          // line-search step size: the candidate is P(d + alpha * delta); 1.0 for the trust-region step
  int first_iteration;   // compute and store the Jacobi scaling
  int reuse_diagonal;    // previous step was rejected (or a line-search pass): Ceres keeps its LM diagonal -- the pass
                         // recomputes it at the same point (identical bits), nothing is stored
  int jacobi_scaling;
  int stream_stores;     // candidate planes stored non-temporally (1) or with plain stores (0)
  unsigned long long n;
};
// Results of one pass: the DEPTH_OUT_* slots of out / host_out (sba_depth_solver.hpp): seven sums and two maxima.
// gather_slot >= 0 (sharded problem): `out` is a 24-double pack for a SUM all-reduce, the sums in [0..6], this rank's
// two maxima in [8 + gather_slot] and [16 + gather_slot] (gather_slot < 8), zeros elsewhere; nothing is published to
// the host.  Candidates go to (c1, c2); (sc*) hold the per-parameter Jacobi scaling.  partials: [grid][16].
hipError_t depth_blocks_per_cu(int store, int* blocks);   // resident 256-thread blocks per CU of depth_step_kernel
hipError_t launch_depth_step(int store, const Planes& pl, const double* d1, const double* d2, double* c1,
                             double* c2, double* sc1, double* sc2,
                             const DepthParams& prm, double* partials, int grid, double* out, double* host_out,
                             unsigned long long seq, int gather_slot, hipStream_t stream);

// Batched d-only stage (one 512-thread block per pair; sba_depth.hip).  BatchDepthConst: the pair's frozen rotation matrix
// and translation (device array, set once per solve).  BatchDepthPass: what the host hands over per pair and pass (mapped
// pinned host memory, 32 B): radius and step size of the pass, flags (bit 0 first pass, 1 keep diagonal, 2 jacobi scaling,
// 3 flip: current depths in the work planes), n = matches taking part (0: pair finished).  Results: out_host[pair][16]
// (DEPTH_OUT_* slots) in mapped host memory, then `seq` at out_host[num_pairs * 16].
struct BatchDepthConst { double R[9]; double t[3]; };
struct BatchDepthPass { double radius, alpha; unsigned long long n; unsigned int flags, pad_; };
static_assert(sizeof(BatchDepthPass) == 32, "BatchDepthPass layout");
hipError_t launch_batch_depth_step(int store, const Planes& pl, const PairDesc* desc, const BatchDepthConst* cst,
                                   const BatchDepthPass* pass_host_dev, int num_pairs, double lambda, double c, double min_diagonal,
                                   double max_diagonal, double* a1, double* a2, double* b1, double* b2, double* sc1, double* sc2,
                                   double* out_host_dev, unsigned int* ticket, unsigned long long seq, hipStream_t stream);
// pairs with flip_dev[pair] != 0: work planes -> the batch's depth planes; out_dev != nullptr: every pair's depths in init_d
// layout at offsets_dev[pair]
// The whole d-only stage of every pair in one launch (batch_depth_solve_kernel: one DepthStageSolver per pair on the device).
// io: the mapped per-pair records of the batch (summary, status; pad_ = passes run); offsets_dev / out_dev as for
// launch_batch_depth_finish (out_dev may be null); seq_host_dev receives `seq` once every pair has delivered.
hipError_t launch_batch_depth_solve(int store, const Planes& pl, const PairDesc* desc, const BatchDepthConst* cst, int num_pairs,
                                    double lambda, double c, const sba_lm_options& opt, double* a1, double* a2, double* b1, double* b2,
                                    double* sc1, double* sc2, const unsigned long long* offsets_dev, double* out_dev, BatchLmIo* io,
                                    unsigned int* ticket, unsigned long long* seq_host_dev, unsigned long long seq,
                                    hipStream_t stream, int pass_cap = 0, void* cont_state = nullptr, BatchDepthPass* cont_req = nullptr,
                                    int* cont_done = nullptr, unsigned char* cont_finish = nullptr);
// passes a pair can need: per iteration the trust-region pass, up to max_num_line_search_step_size_iterations contractions and
// one pass that restores the full step; a few more detect the iteration limit
inline int batch_depth_pass_bound(const sba_lm_options& opt) {
  const long long its = opt.max_num_iterations > 0 ? opt.max_num_iterations : 0;
  const long long lsn = opt.max_num_line_search_step_size_iterations > 0 ? opt.max_num_line_search_step_size_iterations : 0;
  long long bound = its * (lsn + 2) + 4;
  if (bound > (1ll << 24)) bound = 1ll << 24;
  return static_cast<int>(bound);
}
// With cont_state != nullptr (batch_depth_dyn_state_bytes() per pair) the kernel runs at most pass_cap passes per pair; a pair
// that needs more leaves its solver and next request behind (record.status == 1, cont_done[pair] = 0) for the passes with
// dynamic shares: launch_batch_depth_dyn_pass + launch_batch_dyn_compact per pass.  cont_finish[pair] tells
// launch_batch_depth_finish what is left to do for the pair (bit 0 copy back, bit 1 write out).
size_t batch_depth_dyn_state_bytes();
hipError_t launch_batch_depth_dyn_pass(int store, const Planes& pl, const PairDesc* desc, const BatchDepthConst* cst, int num_pairs,
                                       double lambda, double c, const sba_lm_options& opt, double* a1, double* a2, double* b1, double* b2,
                                       double* sc1, double* sc2, int parity, int sweep_grid, void* state, BatchDepthPass* req,
                                       const BatchDynCtl* ctl, const unsigned int* active, int* done, unsigned char* finish,
                                       double* partials, BatchLmIo* io, hipStream_t stream);
hipError_t launch_batch_dyn_compact(BatchDynCtl* ctl, unsigned int* active, const int* done, int num_pairs, int parity,
                                    unsigned long long* host_words, unsigned long long seq, hipStream_t stream);
hipError_t launch_batch_depth_finish(int store, const PairDesc* desc, const unsigned char* flip_dev, int num_pairs, double* a1,
                                     double* a2, const double* b1, const double* b2, const unsigned long long* offsets_dev,
                                     double* out_dev, hipStream_t stream);

// Joint solve (reference .cpp:843-889; sba_joint.hip, step logic sba_joint_solver.hpp): one pass of either kind.
struct JointParams {
  SweepParams cur;       // the current camera (per-match form: Rn = -R, Gn unused), Huber delta, n
  SweepParams cand;      // step pass: the candidate camera (Rn, t)
  double J[9];           // frame of the rotation Jacobian A = -[a]x J (factored_frame: J_l, or I at small angles)
  double delta_c[6];     // step pass: ambient camera step [rot | tran]
  double inv_radius;     // depth damping D / radius; 0 = none
  double min_diagonal, max_diagonal;
  int small_angle;       // rot.rot <= DBL_EPSILON: a = -d1 x1 instead of v
  int first;             // reduce pass: compute and store the depth Jacobi scaling (else it is read)
  int jacobi_scaling;
  int pad_;
};
// Results: the JOINT_OUT_* / JOINT_STEP_* slots (sba_joint_solver.hpp) in out (device) and, with host_out (mapped host
// memory, JOINT_ROW + 1 words), published there followed by `seq` at host_out[JOINT_ROW].  partials: [grid][JOINT_ROW].
hipError_t joint_blocks_per_cu(int store, int* blocks);   // resident 256-thread blocks per CU of joint_reduce_kernel
// Grid of a grid-stride pass over npairs 16-byte vectors (256 per block) by a kernel of occupancy occ: at most
// SBA_JOINT_BLOCKS_PER_CU (1 .. 16, default 8) resident blocks per CU -- fewer than the occupancy where tests force long
// grid-stride loops -- and no block without a vector.  The joint solve's passes and its covariance share it.
inline int joint_grid(size_t npairs, int num_cus, int occ) {
  int cap = 8;
  if (const char* env = std::getenv("SBA_JOINT_BLOCKS_PER_CU")) { const int v = std::atoi(env); if (v >= 1 && v <= 16) cap = v; }
  return static_cast<int>(std::min<size_t>((npairs + 255) / 256, static_cast<size_t>(num_cus) * std::max(1, std::min(occ, cap))));
}
hipError_t launch_joint_reduce(int store, const Planes& pl, const double* d1, const double* d2, double* sc1, double* sc2,
                               const JointParams& prm, double* partials, int grid, double* out, double* host_out,
                               unsigned long long seq, hipStream_t stream);
hipError_t launch_joint_step(int store, const Planes& pl, const double* d1, const double* d2, double* c1, double* c2,
                             const double* sc1, const double* sc2, const JointParams& prm, double* partials, int grid,
                             double* out, double* host_out, unsigned long long seq, hipStream_t stream);

// The fold of [nblocks][JOINT_ROW] block rows into out[count] (count <= 64; slot max_slot, if >= 0, as a maximum) and their
// publication, for other passes with rows of that stride (sba_resection.hip).
hipError_t launch_joint_finalize(const double* partials, int nblocks, int count, int max_slot, double* out, double* host_out,
                                 unsigned long long seq, hipStream_t stream);

// Spherical resection (sba_resection.hip; algebra, row layouts and host finish: sba_resection.hpp).  pl.d2 is never read.
// ResectParams: the wave-uniform state of a pass, a by-value kernel argument (scalar registers) -- Rn = -R and t as in
// SweepParams, and the frame of the rotation Jacobian A = -[a]x J (factored_frame) instead of the 27 entries of Gn, which
// would not fit the scalar registers beside the rest.
// Reduce: prm.delta > 0 selects the Huber instance, partials [grid][JOINT_ROW],
// the SBA_RESECT_* slots in out (device) and, with host_out, published as by launch_joint_reduce.  Moments: the
// SBA_RESECT_MOM_COUNT sums of the linear starting point likewise.  Depths: d_i* into d2 (whole vectors, zeros in the padding).
struct ResectParams {
  double Rn[9];
  double J[9];
  double t[3];
  double delta, delta2;     // Huber a and a * a; delta <= 0: no robustifier
  unsigned long long n;
  int small_angle;          // rot . rot <= DBL_EPSILON: a = -X, J = I
  int pad_;
};
SBA_HD inline void fill_resect_params(unsigned long long n, const double rot[3], const double tran[3], double huber_delta, ResectParams* prm) {
  SweepParams sp;
  fill_sweep_params(n, 1, rot, tran, 1.0, 1.0, huber_delta, &sp, false);
  double B[9];
  factored_frame(rot, B, prm->J);
  for (int i = 0; i < 9; ++i) prm->Rn[i] = sp.Rn[i];
  for (int i = 0; i < 3; ++i) prm->t[i] = sp.t[i];
  prm->delta = sp.delta; prm->delta2 = sp.delta2; prm->n = n;
  prm->small_angle = !(rot[0] * rot[0] + rot[1] * rot[1] + rot[2] * rot[2] > DBL_EPSILON) ? 1 : 0;
  prm->pad_ = 0;
}
hipError_t resect_blocks_per_cu(int store, bool loss, int* blocks);   // resident 256-thread blocks per CU of resect_reduce_kernel
hipError_t launch_resect_reduce(int store, const Planes& pl, const ResectParams& prm, double* partials, int grid, double* out,
                                double* host_out, unsigned long long seq, hipStream_t stream);
hipError_t launch_resect_moments(int store, const Planes& pl, size_t n, double* partials, int grid, double* out, double* host_out,
                                 unsigned long long seq, hipStream_t stream);
hipError_t launch_resect_depths(int store, const Planes& pl, const ResectParams& prm, double* d2, int grid, hipStream_t stream);

// The robust resection guess (sba_resection_consensus.hip; sampler, trial moments and pick: sba_resection_consensus.hpp).
// Gather: out[rows][6] = (X | y) of the matches index[rows] (each < n), X the rounded product d1 x1 as resect_match forms it.
// Score: counts[k] (zeroed by the launcher) = matches with |r|^2 <= tau2 at candidate k of table[count][12] = Rn | t
// (fill_resect_params), 1 <= count <= 1024; integer adds, the same for every grid.  Inlier moments: launch_resect_moments
// over the matches with |r|^2 <= prm.delta2 at prm only; slot SBA_RESECT_MOM_N is their number.
hipError_t launch_resect_gather(int store, const Planes& pl, const long long* index, int rows, double* out, hipStream_t stream);
hipError_t resect_score_blocks_per_cu(int store, int* blocks);   // resident 256-thread blocks per CU of resect_score_kernel
hipError_t launch_resect_score(int store, const Planes& pl, size_t n, const double* table, int count, double tau2,
                               unsigned long long* counts, int grid, hipStream_t stream);
hipError_t launch_resect_inlier_moments(int store, const Planes& pl, const ResectParams& prm, double* partials, int grid, double* out,
                                        double* host_out, unsigned long long seq, hipStream_t stream);

// The resection weighted by the landmarks' covariances (sba_resection_weighted.hip; algebra and host finish:
// sba_resection_weighted.hpp).  ResectWeightParams: the reference pose's ResectParams (delta unused) and the two scalars of
// S_i, a by-value kernel argument.  ResectWeightPlanes: the three f64 planes of the factored weight, padded to whole
// 16-byte vectors like the d1 plane.  Freeze: sigma [>= whole vectors of matches][6] (zeros beyond n) -> the planes, whole vectors,
// zeros in the padding; *n_zero (zeroed by the launcher, device memory) = matches of zero weight, integer adds.  Reduce: the
// SBA_RESECT_* row exactly as launch_resect_reduce publishes it.  Rows: out [whole vectors of matches][6] = M_i (xx, yy,
// zz, xy, xz, yz), zeros beyond n.
struct ResectWeightParams {
  ResectParams P;
  double cov_scale, bearing_sigma2;
};
struct ResectWeightPlanes {
  const double* q[3];
};
hipError_t resect_wreduce_blocks_per_cu(int store, bool loss, int* blocks);   // resident 256-thread blocks per CU of resect_wreduce_kernel
hipError_t launch_resect_weights(int store, const Planes& pl, const ResectWeightParams& prm, const double* sigma, double* const q[3],
                                 unsigned long long* n_zero, int grid, hipStream_t stream);
hipError_t launch_resect_wreduce(int store, const Planes& pl, const ResectWeightPlanes& wp, const ResectParams& prm, double* partials,
                                 int grid, double* out, double* host_out, unsigned long long seq, hipStream_t stream);
hipError_t launch_resect_weight_rows(int store, const Planes& pl, const ResectWeightPlanes& wp, size_t n, double* out, int grid,
                                     hipStream_t stream);

// The landmark map (sba_landmarks.hip; the per-observation code and LandmarkFuseParams, a by-value kernel argument:
// sba_landmarks.hpp).  LandmarkPlanes: ONE allocation of nine f64 planes of `elems` doubles (X.xyz, Sigma xx yy zz xy xz yz) and
// then one u32 plane of `elems` counts; elems even, zeros beyond n.  Pack: caller rows xyz [n][3], cov [n][6] (device, 16-byte
// aligned, exactly n rows are read) -> the planes, cov_scale applied, counts and padding zeroed.  Unpack: the reverse, exactly n
// rows written, either output may be null.  Fuse: idx null = dense (bearings [elems][3], zeros beyond n; chi2 [elems]), else
// bearings [m][3], chi2 [m] and idx [m] strictly increasing and < n; chi2 may be null; counters: LANDMARK_CLASSES words, zeroed
// by the launcher.  No floating-point reduction: the bytes do not depend on the grid.
struct LandmarkFuseParams;
struct LandmarkPlanes {
  double* base;
  size_t elems;
};
hipError_t landmarks_fuse_blocks_per_cu(bool indexed, bool apply, int* blocks);   // resident 256-thread blocks per CU of landmarks_fuse_kernel
hipError_t landmarks_pack_blocks_per_cu(bool unpack, int* blocks);                // ... of landmarks_pack_kernel / landmarks_unpack_kernel
hipError_t launch_landmarks_pack(const double* xyz, const double* cov, size_t n, double cov_scale, const LandmarkPlanes& pl, int grid,
                                 hipStream_t stream);
hipError_t launch_landmarks_unpack(const LandmarkPlanes& pl, size_t n, double* xyz, double* cov, int grid, hipStream_t stream);
hipError_t launch_landmarks_fuse(const LandmarkPlanes& pl, const LandmarkFuseParams& prm, const long long* idx, const double* bearings,
                                 double* chi2, unsigned long long* counters, bool apply, int grid, hipStream_t stream);

// The joint registration of a frame against the landmark map (sba_landmarks_register.hip; the per-observation code and
// LandmarkRegisterParams, a by-value kernel argument: sba_landmarks_register.hpp).  idx null = dense (bearings [elems][3], zeros
// beyond n; noise and chi2 [elems]), else m observations.  Freeze: the noise plane and the freeze's class counts (slot
// LANDMARK_FUSED: the observations that take part) in `counters` (4 words, zeroed by the launcher).  Reduce: partials
// [grid][JOINT_ROW], grid >= 1, the SBA_RESECT_* slots in out (device).  Apply: the write-back (apply) or the dry run, chi2 may be
// null, the four class counts in `counters` (zeroed by the launcher).
struct LandmarkRegisterParams;
enum { LANDMARK_REGISTER_FREEZE = 0, LANDMARK_REGISTER_REDUCE = 1, LANDMARK_REGISTER_APPLY = 2, LANDMARK_REGISTER_KERNELS = 3 };
hipError_t landmarks_register_blocks_per_cu(int which, bool indexed, bool apply, int* blocks);   // resident 256-thread blocks per CU
hipError_t launch_landmarks_register_freeze(const LandmarkPlanes& pl, const LandmarkRegisterParams& prm, const long long* idx, const double* bearings,
                                            double* noise, unsigned long long* counters, int grid, hipStream_t stream);
hipError_t launch_landmarks_register_reduce(const LandmarkPlanes& pl, const LandmarkRegisterParams& prm, const long long* idx, const double* bearings,
                                            const double* noise, double* partials, int grid, double* out, hipStream_t stream);
hipError_t launch_landmarks_register_apply(const LandmarkPlanes& pl, const LandmarkRegisterParams& prm, const long long* idx, const double* bearings,
                                           const double* noise, double* chi2, unsigned long long* counters, bool apply, int grid, hipStream_t stream);

// The robust joint registration's reduce pass (sba_landmarks_register_robust.hip; the objective, LandmarkRegisterRobust and the
// per-observation code: sba_landmarks_register_robust.hpp): launch_landmarks_register_reduce's arguments and the loss, the
// outlier count in slot SBA_RESECT_NOUT.  Its freeze and its write-back are the two launches above.
struct LandmarkRegisterRobust;
hipError_t landmarks_register_robust_blocks_per_cu(bool indexed, int* blocks);   // resident 256-thread blocks per CU
hipError_t launch_landmarks_register_robust_reduce(const LandmarkPlanes& pl, const LandmarkRegisterParams& prm, const LandmarkRegisterRobust& loss,
                                                   const long long* idx, const double* bearings, const double* noise, double* partials, int grid,
                                                   double* out, hipStream_t stream);

// The same pass under Hampel's redescending loss (sba_landmarks_register_hampel.hip; the loss, LandmarkRegisterHampel and the
// per-observation code: sba_landmarks_register_hampel.hpp): a row of 32 slots, the SBA_RESECT_* ones and the count of the
// observations beyond c in slot SBA_HAMPEL_NREJ.  The freeze and the write-back are again the two launches above.
struct LandmarkRegisterHampel;
hipError_t landmarks_register_hampel_blocks_per_cu(bool indexed, int* blocks);   // resident 256-thread blocks per CU
hipError_t launch_landmarks_register_hampel_reduce(const LandmarkPlanes& pl, const LandmarkRegisterParams& prm, const LandmarkRegisterHampel& loss,
                                                   const long long* idx, const double* bearings, const double* noise, double* partials, int grid,
                                                   double* out, hipStream_t stream);

// Edits of the landmark map (sba_landmarks_edit.hip; the score, the classes of a prune and the checks: sba_landmarks_edit.hpp).
// Scores: out [elems] doubles (device, 16-byte aligned).  Keep: one streaming pass that writes keep[ntiles * kCompactTile] bytes
// (1 = kept, 0 beyond n) and adds the LANDMARK_PRUNE_CLASSES class counts to `counters` (zeroed by the launcher):
// kLandmarkCounterRows rows of kLandmarkCounterStride words, a wave adds to the row its index selects and the caller sums the rows
// per class -- every wave's atomics on the same five words cost 280 us at 10^7 landmarks (tools/landmark_keep_probe.hip).  mask:
// device bytes in whole tiles or null.  Scatter: block b = tile b of the compaction (launch_compact_count / _scan give tile_offset);
// every kept landmark i goes to row tile_offset + rank of dst -- all ten planes, when dst.base is not null -- and i to
// kept_index (may be null); row n_kept of dst is zeroed when n_kept is odd.  src and dst must not overlap.  Append: dst's
// n_old + n_add rows = src's first n_old rows with their counts, then the caller's rows (device, exactly n_add of each are
// read, any 8-byte alignment) with cov_scale applied and count 0; padding zeroed.  Gather: row j of xyz [m][3], cov [m][6],
// counts [m] (each may be null) = landmark idx[j] < n.  No floating-point reduction: the bytes do not depend on the grid.
constexpr int kLandmarkCounterRows = 64, kLandmarkCounterStride = 32;   // rows 256 bytes apart
enum { LANDMARK_EDIT_SCORES = 0, LANDMARK_EDIT_KEEP = 1, LANDMARK_EDIT_APPEND = 2, LANDMARK_EDIT_GATHER = 3, LANDMARK_EDIT_KERNELS = 4 };
hipError_t landmarks_edit_blocks_per_cu(int which, int* blocks);   // resident 256-thread blocks per CU of the grid-stride kernels
hipError_t launch_landmarks_scores(const LandmarkPlanes& pl, double* out, int grid, hipStream_t stream);
hipError_t launch_landmarks_keep(const LandmarkPlanes& pl, size_t n, double max_score, unsigned int min_count, const unsigned char* mask,
                                 unsigned char* keep, size_t ntiles, unsigned long long* counters, int grid, hipStream_t stream);
hipError_t launch_landmarks_compact_scatter(const unsigned char* keep, size_t n, const unsigned long long* tile_offset, size_t ntiles,
                                            const LandmarkPlanes& src, const LandmarkPlanes& dst, size_t n_kept, long long* kept_index,
                                            hipStream_t stream);
hipError_t launch_landmarks_append(const LandmarkPlanes& src, size_t n_old, const double* xyz, const double* cov, size_t n_add,
                                   double cov_scale, const LandmarkPlanes& dst, int grid, hipStream_t stream);
hipError_t launch_landmarks_gather(const LandmarkPlanes& pl, const long long* idx, size_t m, double* xyz, double* cov, unsigned int* counts,
                                   int grid, hipStream_t stream);

// The landmark map's descriptors and the association of a frame (sba_landmarks_associate.hip; the claim key and the checks:
// sba_landmarks_associate.hpp).  Descriptor rows are packed: row i = dim floats at desc + i * dim.  Desc scatter: the kept rows of
// src (keep, tile_offset: the very bytes and offsets launch_landmarks_compact_scatter took) to row tile_offset + rank of dst, which
// must not overlap src.  Desc gather: row j of out = row idx[j] < n.  Claim: matches k < n_matches of the matcher's compacted list
// (frame row, landmark, distance); one with distance <= max_distance puts its key into slots[landmark] by a 64-bit integer atomic
// min (slots preset to all ones by the caller) and counts in counters[0] (zeroed by the caller).  Keep: keep[i] = 1 where slot i
// was claimed, whole tiles, 0 beyond n.  Scatter: block b = tile b; claimed landmark i goes to output tile_offset + rank: idx = i,
// row and dist = the halves of its key, bearings_out row = a bitwise copy of the winner's row of frame_bearings (both or neither
// null).  Integer atomics only and no floating-point reduction: the bytes depend neither on the grid nor on the run.
enum { LANDMARK_ASSOC_CLAIM = 0, LANDMARK_ASSOC_KEEP = 1, LANDMARK_ASSOC_DESC_GATHER = 2, LANDMARK_ASSOC_KERNELS = 3 };
hipError_t landmarks_associate_blocks_per_cu(int which, int* blocks);   // resident 256-thread blocks per CU of the grid-stride kernels
hipError_t launch_landmarks_desc_compact_scatter(const unsigned char* keep, size_t n, const unsigned long long* tile_offset, size_t ntiles,
                                                 const float* src, float* dst, int dim, hipStream_t stream);
hipError_t launch_landmarks_desc_gather(const float* desc, int dim, const long long* idx, size_t m, float* out, int grid, hipStream_t stream);
hipError_t launch_landmarks_claim(const int* match_row, const int* match_landmark, const float* match_dist, size_t n_matches, float max_distance,
                                  unsigned long long* slots, unsigned long long* counters, int grid, hipStream_t stream);
hipError_t launch_landmarks_associate_keep(const unsigned long long* slots, size_t n, unsigned char* keep, size_t ntiles, int grid,
                                           hipStream_t stream);
hipError_t launch_landmarks_associate_scatter(const unsigned char* keep, size_t n, const unsigned long long* tile_offset, size_t ntiles,
                                              const unsigned long long* slots, const double* frame_bearings, long long* idx_out, int* row_out,
                                              float* dist_out, double* bearings_out, hipStream_t stream);

// Covariance of the joint solve (sba_covariance.hip; algebra and host finish: sba_covariance.hpp).  prm: a first reduce
// pass's JointParams with inv_radius = 0.  Reduce: partials [grid][COV_ROW], out (device) the COV_OUT_* slots.  Depth:
// sigma_c the ambient 6 x 6 camera covariance, out [(n + 1) / 2][6] doubles = (var d1, var d2, cov) per match.
hipError_t cov_blocks_per_cu(int store, int* blocks);   // resident 256-thread blocks per CU of cov_reduce_kernel
hipError_t launch_cov_reduce(int store, const Planes& pl, const double* d1, const double* d2, const JointParams& prm,
                             double min_sin2, double* partials, int grid, double* out, hipStream_t stream);
hipError_t launch_cov_depth(int store, const Planes& pl, const double* d1, const double* d2, const JointParams& prm,
                            double min_sin2, const double sigma_c[36], double* out, int grid, hipStream_t stream);

// Triangulated landmarks with their covariances (sba_structure.hip; algebra: sba_structure.hpp).  params_dev: device memory,
// staged in LDS by the kernel -- prm as for launch_cov_reduce, sigma_c the ambient 6 x 6 camera covariance.  xyz [n][3],
// cov [n][6] (xx, yy, zz, xy, xz, yz), score [n]: device pointers, 16-byte aligned, any of them null (that output is compiled
// out); exactly n rows are written.
struct StructureParams {
  JointParams prm;
  double sigma_c[36];
  double min_sin2;
  double pad_;
};
hipError_t structure_blocks_per_cu(int store, int* blocks);   // resident 256-thread blocks per CU of the all-outputs kernel
hipError_t launch_structure(int store, const Planes& pl, const double* d1, const double* d2, const StructureParams* params_dev,
                            double* xyz, double* cov, double* score, int grid, hipStream_t stream);

// Batched joint solve (sba_batch_joint.hip): ONE 256-thread block per pair -- the reduce body's ~350 registers fit one wave per
// SIMD only, a 512-thread block would halve the budget and spill into the hot loop.  BatchJointPass: what the lock-step driver
// hands over per pair and pass (mapped pinned host memory): the pass kind (kJointReduce / kJointStep), the current camera, for a
// step pass the candidate camera and the ambient camera step, the radius of the depth damping, flags (bit 0 first pass: store
// the depth Jacobi scaling, bit 3 flip: the pair's current depths are in the work planes, its candidates go to the batch's depth
// planes), n = matches taking part (0: skip the pair).  Thread 0 of the pair's block turns the record into the pass's
// JointParams ON THE DEVICE (fill_sweep_params, factored_frame) -- as thread 0 of batch_joint_solve_kernel does from its solver's
// request, so both drivers run their passes from the same bits.  Results: out_host[pair][JOINT_ROW] (JOINT_OUT_* / JOINT_STEP_*
// slots; zeros for a skipped pair) in mapped host memory, then `seq` at out_host[num_pairs * JOINT_ROW].
struct BatchJointPass {
  double rot[3], tran[3];
  double rot_cand[3], tran_cand[3];
  double delta_c[6];
  double radius;
  unsigned long long n;
  unsigned int kind, flags;
};
static_assert(sizeof(BatchJointPass) == 168, "BatchJointPass layout");
hipError_t launch_batch_joint_pass(int store, const Planes& pl, const PairDesc* desc, const BatchJointPass* pass_host_dev, int num_pairs,
                                   const sba_lm_options& opt, double* a1, double* a2, double* b1, double* b2, double* sc1, double* sc2,
                                   double* out_host_dev, unsigned int* ticket, unsigned long long seq, hipStream_t stream);
// The whole joint LM of every pair in one launch (batch_joint_solve_kernel: one JointSolver per pair in LDS).  io: the mapped
// per-pair records of the batch -- in: rot, tran, status != 0 marks a pair that must not start (non-finite start); out: rot,
// tran, summary, status, pad_ = passes run.  (a1, a2): the batch's depth planes, (b1, b2): candidate work planes; offsets_dev /
// out_dev as for launch_batch_depth_finish (out_dev may be null); seq_host_dev receives `seq` once every pair has delivered.
hipError_t launch_batch_joint_solve(int store, const Planes& pl, const PairDesc* desc, int num_pairs, const sba_lm_options& opt,
                                    double* a1, double* a2, double* b1, double* b2, double* sc1, double* sc2,
                                    const unsigned long long* offsets_dev, double* out_dev, BatchLmIo* io, unsigned int* ticket,
                                    unsigned long long* seq_host_dev, unsigned long long seq, hipStream_t stream);
// Passes a pair's joint solve can need: in JointSolver::feed_reduce every reduce pass either finishes the solve or increments
// the iteration counter (which max_num_iterations bounds), and an iteration has at most one step pass.
inline int batch_joint_pass_bound(const sba_lm_options& opt) {
  long long its = opt.max_num_iterations > 0 ? opt.max_num_iterations : 0;
  if (its > (1ll << 23)) its = 1ll << 23;
  return static_cast<int>(2 * its + 2);
}

// Batched joint covariance (sba_batch_covariance.hip): ONE 256-thread block per pair runs the pair's whole covariance -- reduce
// (the body of cov_reduce_kernel), finish (cov_finish by thread 0, its arrays and Sigma_c in LDS), depth (the body of
// cov_depth_kernel, rows to out[offsets[pair] + i][3]) -- or, under the lock-step driver, the phases `phases` names.
// BatchCovRec: the pair's record in mapped pinned host memory.  In: rot, tran; refused != 0 marks a pair that must fail (a
// non-finite point); without kCovFinish also sigma and dim_status (the host's finish).  Out: with kCovReduce the COV_OUT_* slots
// in row, with kCovFinish sigma (NaN for a failed pair) and dim_status = dim | failed << 32.
enum { kCovReduce = 1, kCovFinish = 2, kCovDepth = 4 };
struct BatchCovRec {
  double rot[3], tran[3];
  double row[32];               // COV_ROW (sba_covariance.hpp) doubles, COV_OUT_COUNT used
  double sigma[36];
  unsigned long long dim_status;
  unsigned long long refused;
};
static_assert(sizeof(BatchCovRec) == 608, "BatchCovRec layout");
// ticket: one zeroed device word; seq_host_dev receives `seq` once every pair's block has delivered.  out (may be null: no
// depth phase): [total][3] doubles in caller row order, offsets_dev relative to the first row.
hipError_t launch_batch_cov(int store, const Planes& pl, const PairDesc* desc, int num_pairs, const sba_lm_options& opt,
                            double min_sin2, int phases, const unsigned long long* offsets_dev, double* out, BatchCovRec* rec,
                            unsigned int* ticket, unsigned long long* seq_host_dev, unsigned long long seq, hipStream_t stream);

// Batched structure (sba_batch_structure.hip): grid (num_pairs, blocks_per_pair) of 256-thread blocks; follows a
// kCovReduce | kCovFinish launch of launch_batch_cov on the same stream (or the host's finish) and reads every pair's rot, tran,
// sigma and dim_status from rec.  xyz [total][3], cov [total][6], score [total]: device pointers in caller row order
// (offsets_dev relative to the first row), 16-byte aligned, any of them null (that output is compiled out); a pair's own n rows
// are written, `fill` in every row of a pair whose finish failed.  The bits do not depend on blocks_per_pair.
hipError_t launch_batch_structure(int store, const Planes& pl, const PairDesc* desc, int num_pairs, int blocks_per_pair,
                                  const sba_lm_options& opt, double min_sin2, double fill, const unsigned long long* offsets_dev,
                                  const BatchCovRec* rec, double* xyz, double* cov, double* score, hipStream_t stream);

// 8-point initial guess, device part (.cpp:53-68): A^T A of the kron(left, right) rows for 64 interleaved groups.
// groups_dev: [64][45]; partials: [grid][45][64] scratch.
hipError_t launch_epipolar_moments(int store, const Planes& pl, size_t n, double* partials, int grid,
                                   double* groups_dev, hipStream_t stream);

// The 64 x 45 group moments of every pair of a batch: groups_dev[num_pairs][64][45], one block per pair.
hipError_t launch_batch_epipolar_moments(int store, const Planes& pl, const PairDesc* desc, int num_pairs, double* groups_dev,
                                         hipStream_t stream);

// The trials and the consensus pick of every pair on the device (batch_guess_kernel): one block per pair reads the pair's
// group moments and writes its record.  trials <= kGuessMaxTrials.
constexpr int kGuessMaxTrials = 128;
struct BatchGuessOut { double euler[3]; double tran[3]; int num_candidates; int status; };
static_assert(sizeof(BatchGuessOut) == 56, "BatchGuessOut layout");
hipError_t launch_batch_guess(const double* groups_dev, int num_pairs, int trials, double fraction, unsigned long long seed,
                              BatchGuessOut* out_dev, hipStream_t stream);

// ... the same A^T A per TRIAL over explicit index lists (the reference's own random subsets, .cpp:130-141):
// indices_dev [trials][m] int32, moments_dev [trials][45].
hipError_t launch_epipolar_subset_moments(int store, const Planes& pl, size_t n, const int* indices_dev, int trials, int m,
                                          double* moments_dev, hipStream_t stream);

// pixel -> unit sphere (spherical_bundle_adjuster.cpp:271-298)
hipError_t launch_keypoints_to_sphere(const uint8_t* kp, size_t n, size_t stride_bytes, double im_w,
                                      double im_h, double* out_xyz, hipStream_t stream);
// ... fused with the upload: matched key-point records of both images -> the six coordinate planes (x1.xyz, x2.xyz)
hipError_t launch_keypoints_to_planes(const uint8_t* kp_left, const uint8_t* kp_right, size_t n, size_t stride_bytes,
                                      double im_w, double im_h, void* const planes[6], int store, hipStream_t stream);
int points_per_lane(int store);  // 2 for f64 planes, 4 for f32 planes

}  // namespace sba
