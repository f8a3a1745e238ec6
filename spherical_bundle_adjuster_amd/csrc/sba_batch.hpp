// The batch handle (sba_batch.cpp) and what the translation units that work on it share (sba_batch_select.cpp).
#pragma once
#include <vector>

#include "sba_internal.hpp"
#include "sba_quantile.hpp"

struct sba_batch {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  int poisoned = 0;            // a device wait timed out or the device faulted (sba_internal.hpp): the handle is refused
                               // from then on -- its ticket word and sequence numbers are out of step -- destroy leaks
  int num_cus = 0;
  int kind = SBA_KERNEL_FACTORED;

  int num_pairs = 0;
  int store = SBA_STORE_F64;
  bool has_d12 = false;
  bool uploaded = false;
  std::vector<size_t> n;            // matches per pair
  std::vector<size_t> first_vec;    // first 16-byte vector of the pair inside the planes
  size_t tile_stride = 256;         // vectors between consecutive 256-vector tiles of a pair (256 = contiguous pairs; sba_device.hpp: PairDesc)
  size_t total_vecs = 0;
  void* coord[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  double* dplane[2] = {nullptr, nullptr};
  void* plane_base[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // hipMalloc'ed blocks
  size_t plane_stagger = 4352;   // plane k starts k * 4352 B into its allocation (as sba_problem: equal element indices of
                                 // the 8 streams then differ in their low address bits); SBA_PLANE_STAGGER overrides
  sba::PairDesc* desc_dev = nullptr;
  sba::SweepParams* params_dev = nullptr;    // built on the device by batch_prepare_kernel
  sba::BatchState* state_host = nullptr;     // pinned + mapped: what the host hands over per pair and step (80 B)
  sba::BatchState* state_host_dev = nullptr; // device-visible address of state_host
  double* frames_dev = nullptr;              // [pair][18]: (B, J) of the pair's rotation, for the moment conversion
  double* partials = nullptr;
  int bpp = 1;                                // blocks per pair
  double* packs_dev = nullptr;
  double* packs_host = nullptr;               // pinned + mapped: 24 doubles per pair, then the sequence word
  double* packs_host_dev = nullptr;           // device-visible address of packs_host
  unsigned long long seq = 0;                 // launches published so far
  bool publish = true;                        // SBA_PUBLISH=0: D2H copy + stream synchronise instead
  sba::BatchLmIo* lm_io_host = nullptr;       // pinned + mapped: per-pair start point in, result + summary out (batch_lm_kernel)
  sba::BatchLmIo* lm_io_host_dev = nullptr;   // device-visible address of lm_io_host
  unsigned int* lm_ticket = nullptr;          // device: blocks of batch_lm_kernel that have delivered their record
  std::vector<size_t> offsets;                // row offset of every pair in the caller's concatenated arrays (num_pairs + 1)
  size_t plane_elems = 0;                     // elements per plane
  // batched d-only stage (allocated on first use, kept while the batch lives)
  double* depth_work = nullptr;               // 4 planes: candidate depths (2), Jacobi scaling (2)
  sba::BatchDepthConst* depth_const_dev = nullptr;
  sba::BatchDepthPass* depth_pass_host = nullptr;     // pinned + mapped
  sba::BatchDepthPass* depth_pass_host_dev = nullptr;
  double* depth_out_host = nullptr;           // pinned + mapped: [num_pairs][16] results, then the sequence word
  double* depth_out_host_dev = nullptr;
  unsigned long long depth_seq = 0;
  // batched joint solve (allocated on first use; its work planes are the d-only stage's: depth_work)
  sba::BatchJointPass* joint_pass_host = nullptr;     // pinned + mapped: the lock-step driver's per-pair pass records
  sba::BatchJointPass* joint_pass_host_dev = nullptr;
  double* joint_out_host = nullptr;           // pinned + mapped: [num_pairs][JOINT_ROW] rows, then the sequence word
  double* joint_out_host_dev = nullptr;
  unsigned long long joint_seq = 0;
  // batched joint covariance (allocated on first use; its per-match output passes through depth_work)
  sba::BatchCovRec* cov_rec_host = nullptr;           // pinned + mapped: [num_pairs] records, then the sequence word
  sba::BatchCovRec* cov_rec_host_dev = nullptr;
  unsigned long long cov_seq = 0;
  // batched initial guess (allocated on first use): the 64 x 45 group moments of every pair
  double* epi_groups_dev = nullptr;
  double* epi_groups_host = nullptr;          // pinned
  sba::BatchGuessOut* guess_out_dev = nullptr;
  sba::BatchGuessOut* guess_out_host = nullptr;   // pinned
  // device-resident solves with dynamic shares (allocated on first use)
  sba::BatchDynCtl* dyn_ctl = nullptr;
  unsigned int* dyn_active = nullptr;        // [2][num_pairs]
  int* dyn_done = nullptr;                   // [num_pairs]
  void* dyn_state = nullptr;                 // per-pair solver state
  double* dyn_partials = nullptr;            // share rows of one launch
  size_t dyn_partial_rows = 0;
  unsigned long long* dyn_host = nullptr;    // pinned + mapped: [0] pairs still active, [1] sequence word
  unsigned long long* dyn_host_dev = nullptr;
  unsigned long long dyn_seq = 0;
  sba::BatchDepthPass* dyn_depth_req = nullptr;   // [num_pairs]: the next pass of every pair of the d-only stage
  unsigned char* dyn_finish = nullptr;            // [num_pairs]: what batch_depth_finish_kernel has left to do
  // upload: row offsets on the device (relative to the first row), two pinned staging buffers, their DMA-done events
  unsigned long long* offsets_dev = nullptr;
  void* upload_pinned[2] = {nullptr, nullptr};
  hipEvent_t upload_ev[2] = {nullptr, nullptr};
  // per-match residuals (sba_batch_residuals, allocated on first use): the per-pair inlier counts, then the outputs
  void* select_scratch = nullptr;
  size_t select_scratch_bytes = 0;
  // batched structure, host form (sba_batch_structure_joint, grown on demand): the outputs asked for on their way to the host
  void* structure_scratch = nullptr;
  size_t structure_scratch_bytes = 0;
};

namespace sba {
namespace batch {

// Releases every device and mapped buffer of the batch's pairs (not the stream, the upload staging buffers or the kernel kind).
int free_batch_data(sba_batch* b);
int check_batch_args(const sba_batch* b, int mode, int depth_mode, const double* rot, const double* tran);
// The 80-byte per-pair state of one evaluation at (rot, tran, d1, d2) (NULL depths: 1.0) into mapped host memory; a pair with
// active[g] == 0 takes part with n = 0.
void write_state(sba_batch* b, const double* rot, const double* tran, const double* d1, const double* d2,
                 const unsigned char* active);
// Layout and allocation from the row offsets of the pairs (num_pairs + 1, non-decreasing, kept as given): per-pair n, where
// every pair starts (contiguous or interleaved: SBA_BATCH_INTERLEAVE), the zeroed planes, blocks per pair (SBA_BATCH_BPP),
// the descriptors and the row offsets (relative to offsets[0]) on the device, and the per-pair mapped buffers.  The handle
// must hold no pair data (free_batch_data).  An upload and a compaction both lay out a batch through here.
int layout_pairs(sba_batch* b, const size_t* offsets, int num_pairs, int store, bool has_d12);
// The work planes (candidate depths, depth Jacobi scaling: zeroed once) and the per-pair buffers of the batched d-only stage,
// allocated on first use; the batched joint solve shares the planes (the two stages never overlap).
int ensure_depth_work(sba_batch* b);

// sba_batch_joint.cpp -- the whole-call refusals and the default options (the sphere gauge) of the batched joint entry
// points, which the batched joint covariance shares (sba_batch_covariance.cpp).
int joint_check(sba_batch* b, const double* rot, const double* tran);
void joint_options(const sba_lm_options* opt, sba_lm_options* o);

// sba_batch_covariance.cpp -- the batched covariance's reduce pass and finish, which the batched structure shares
// (sba_batch_structure.cpp).  cov_enqueue: every pair's record (rot, tran, refused for a non-finite point) and the launches of
// launch_batch_cov on the batch's stream -- reduce + finish (+ the depth phase into depth_dev, caller row order, when it is not
// null) in one launch, or with SBA_BATCH_DEVICE_COV=0 the reduce launch, a wait, the host's cov_finish per pair and the depth
// launch.  cov_wait: until the records of the launch that has not been waited for are on the host.  cov_read: out[g] (may be
// null) and status[g] (may be null) from the records; returns the number of pairs without a covariance.  cov_failed: that
// count as the call's return value (SBA_OK or SBA_ERR_NUMERIC with its message).
struct CovPass {
  sba_lm_options o;
  sba::Planes pl;
  unsigned long long seq = 0;   // what the records' sequence word reaches; 0: nothing is left to wait for
};
int cov_enqueue(sba_batch* b, const double* rot, const double* tran, const sba_lm_options* opt, double min_sin2_parallax,
                double* depth_dev, CovPass* cp);
int cov_wait(sba_batch* b, CovPass* cp, const char* what);
int cov_read(const sba_batch* b, sba_joint_cov* out, int* status);
int cov_failed(int failures, int num_pairs);

// sba_quantile.cpp -- the batch's selection over a plane that is already on the device, in the three steps the single problem
// has (sba_problem.hpp): the scratch with its plane of batch_rows doubles; ranks (and scales) to the device and the selection;
// the threshold kernel's keep bytes, the compaction and the thresholds.  grow_scratch: a handle's cached device scratch, grown
// (or shrunk when far too large) only once the stream has drained.
int grow_scratch(void** scratch, size_t* have, size_t need, hipStream_t stream, int* poisoned);
int select_plane(sba_batch* b, int num_ranks, sba::SelectScratch* s, double** plane);
int select_enqueue(sba_batch* b, const sba::SelectScratch& s, const size_t* ranks, int num_ranks, const double* scale);
int select_keep(sba_batch* b, const sba::SelectScratch& s, double* threshold, size_t* n_kept, long long* kept_index);

// sba_batch_select.cpp -- what the entry points that look at single matches share (sba_quantile.cpp).
size_t batch_rows(const sba_batch* b);
sba::Planes batch_planes(const sba_batch* b);
// The residual kernel at (rot, tran, d1, d2): every pair's sweep state is built on the device from the same 80-byte record a
// batched step reads, so the residuals carry the sweep's bits.  out.n_inlier: num_pairs device words, zeroed here.
int residual_pass(sba_batch* b, int depth_mode, const double* rot, const double* tran, const double* d1, const double* d2,
                  double huber_delta, int outputs, const sba::ResidualOut& out);
// Device scratch of one compaction: keep bytes (whole tiles, zero beyond the rows) | tile counts | tile offsets | total |
// kept rows per pair | inlier counts per pair (keep_inliers).
struct CompactWork {
  explicit CompactWork(const int* poison) : buf(poison) {}
  sba::DeviceBuffer buf;
  size_t rows = 0, ntiles = 0;
  unsigned char* keep = nullptr;
  unsigned int* tile_count = nullptr;
  unsigned long long* tile_offset = nullptr;
  unsigned long long* total = nullptr;
  unsigned long long* pair_kept = nullptr;
  unsigned long long* n_inlier = nullptr;
};

int alloc_work(sba_batch* b, size_t rows, CompactWork* w);
// w.keep holds the rows' flags (queued on the stream): counts every pair's kept rows, lays the batch out afresh for them and
// moves the kept rows over -- everything sba_batch_compact does after its keep bytes are on the device.
int compact_rows(sba_batch* b, CompactWork& w, size_t* n_kept, long long* kept_index);
// No rows at all: every pair keeps nothing, and the offsets become those of an upload of nothing.
void compact_nothing(sba_batch* b, size_t* n_kept);

}  // namespace batch
}  // namespace sba
