// The problem handle behind the C-ABI and the helpers shared by the translation units that implement it:
//   sba_shim.cpp       errors, handle life cycle, uploads, sweeps, eval / solve entry points, side entry points
//   sba_transport.cpp  multi-GPU transports: RCCL (bound at run time), direct peer exchange, user hook; pack all-reduce
//   sba_stages.cpp     d-only stage and 8-point initial guess entry points
//   sba_select.cpp     per-match residuals and compaction of the matches
//   sba_joint.cpp      joint solve (depths, rotation and translation together) entry points
//   sba_covariance.cpp covariance of the joint solve at a point (pose 6x6, per-match depth blocks)
//   sba_structure.cpp  triangulated landmarks with their covariances at a point, and the cut driven by their score
//   sba_resection.cpp  spherical resection: a further frame's pose from the handle's landmarks d1 x1 and bearings x2
//   sba_resection_consensus.cpp  its robust starting point: sampled DLT trials scored on the device
//   sba_resection_weighted.cpp   the resection weighted by the landmarks' covariances, and the pose covariance
//   sba_quantile.cpp   order statistics of the per-match squared residual norms and the keep-rule built on them
// Internal: nothing here is exported from the library.
#pragma once
#include <cstdlib>
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/sba_hip.h"
#include "sba_device.hpp"
#include "sba_internal.hpp"
#include "sba_quantile.hpp"
#include "sba_resident.hpp"

// ---- the handle ---------------------------------------------------------------------------------
struct sba_problem {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  int poisoned = 0;            // a device wait on `stream` timed out or the device faulted (sba_internal.hpp): every entry
                               // point refuses the handle from then on, destroy leaks the device resources
  int num_cus = 0;
  int blocks_per_cu_cap = 0;   // SBA_BLOCKS_PER_CU: resident blocks per CU used; 0 = the per-variant default of grid_for
                               // (1 or 2: the register double buffer supplies the memory-level parallelism, more
                               // waves only add rows to fold and finish-time spread, profiles/r01_tune_caps.log)
  int kind = SBA_KERNEL_FACTORED;
  int occ_cache[3][3][2][2][2];  // resident blocks/CU per [mode][depth (2 = folded)][store][kind][loss], 0 = unknown
  int depth_occ[2] = {0, 0};     // same for depth_step_kernel per [store]
  double* epi_scratch = nullptr; // 8-point moments: [grid][45][64] block partials + [64][45] groups, kept across calls
  size_t epi_scratch_elems = 0;
  void* upload_pinned[2] = {nullptr, nullptr};   // large uploads: two pinned staging buffers (sba_shim.cpp: upload_common)
  void* depth_scratch = nullptr;   // d-only stage: candidate + scaling planes, block partials, results; kept across calls
  size_t depth_scratch_bytes = 0;
  double* joint_host = nullptr;    // joint solve: mapped pinned row the finalize kernel publishes to (JOINT_ROW doubles + the
  double* joint_host_dev = nullptr;  // sequence word); allocated by the first joint call.  Its device planes share depth_scratch
  unsigned long long joint_seq = 0;
  int joint_occ[2] = {0, 0};       // resident blocks per CU of joint_reduce_kernel per [store]
  int cov_occ[2] = {0, 0};         // ... and of cov_reduce_kernel (sba_covariance.cpp; its rows and outputs share depth_scratch)
  int structure_occ[2] = {0, 0};   // ... and of structure_kernel (sba_structure.cpp; parameters and host-form outputs share depth_scratch)
  int resect_occ[2][2] = {{0, 0}, {0, 0}};   // ... and of resect_reduce_kernel per [store][loss] (sba_resection.cpp; rows share depth_scratch)
  void* consensus_scratch = nullptr;   // robust resection guess (sba_resection_consensus.cpp): candidate table, counts, sampled indices
  size_t consensus_scratch_bytes = 0;  // and gathered rows; allocated by the first call, kept across calls
  int score_occ[2] = {0, 0};           // resident blocks per CU of resect_score_kernel per [store]
  // Weighted resection (sba_resection_weighted.cpp), allocated at first use: a copy of the landmark covariance rows
  // [plane_elems][6] and the three planes of the factored weight [3][plane_elems] followed by the zero-weight counter.
  // alloc_planes (every upload, every compaction) clears the two flags; the allocations are kept for the next use.
  double* wres_cov = nullptr;
  size_t wres_cov_elems = 0;
  double* wres_planes = nullptr;
  size_t wres_plane_elems = 0;
  bool wres_have_cov = false, wres_frozen = false;
  double wres_cov_scale = 1.0;
  long long wres_n_zero = 0;               // of the last freeze
  int wres_occ[2][2] = {{0, 0}, {0, 0}};   // resident blocks per CU of resect_wreduce_kernel per [store][loss]
  void* subset_scratch = nullptr;  // reference sampling: [trials][45] moments, then the [trials][m] index lists; kept across calls
  size_t subset_scratch_bytes = 0;
  void* select_scratch = nullptr;  // per-match residuals: inlier count, then the requested outputs; kept across calls
  size_t select_scratch_bytes = 0;
  double frame_B[9], frame_J[9];  // factored kernel: host-side frame of the last enqueued sweep
  int last_mode = 0;

  size_t n = 0;
  int store = SBA_STORE_F64;
  bool has_d12 = false;
  bool uploaded = false;
  size_t plane_elems = 0;     // allocated elements per plane (n rounded up to a whole vector)
  void* coord[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  double* dplane[2] = {nullptr, nullptr};
  // Per-match depths folded into the coordinates, X1 = d1 x1 and X2 = d2 x2 (f64 planes only): a cache of the raw planes
  // that per-match sweeps stream instead of them -- 48 B per match instead of 64.  The raw planes
  // stay: the d-only stage, the initial guess and the batched / resident paths read them.  Refolded at the end of every
  // upload / set_depths; writers on the device (the d-only stage) only clear folded_valid, and the next per-match sweep
  // refolds first.
  double* folded[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  bool folding = true;         // sba_problem_set_folding
  bool folded_valid = false;   // folded[] hold d1 x1, d2 x2 of the current planes
  bool fold_failed = false;    // their allocation failed for this upload: per-match sweeps read the raw planes
  static constexpr int kPlaneSlots = 14;   // 6 coordinate + 2 depth planes, then the 6 folded planes
  void* plane_base[kPlaneSlots] = {};      // hipMalloc'ed blocks
  size_t plane_bytes[kPlaneSlots] = {};    // their sizes: an upload that fits reuses them (a hipFree + hipMalloc pair per
                                           // plane costs more than the whole upload of a 2 000-match problem)
  size_t plane_stagger = 4352; // SBA_PLANE_STAGGER: plane k starts k * 4352 B (17 x 256 B) into its allocation, so equal
                               // element indices of the 8 streams differ in their low address bits (measured 0-4 %
                               // faster with f64 planes, 3-5 % with f32 planes; never slower)

  double* partials = nullptr;  // [max_grid][24]
  int max_grid = 0;
  double* pack_dev = nullptr;  // 32 doubles
  double* pack_host = nullptr; // pinned + mapped, 32 doubles ([24] = sequence number published by the kernel)
  double* pack_host_dev = nullptr;  // device-visible address of pack_host
  unsigned int* ticket = nullptr;   // arrival counter of the fused final reduction
  unsigned long long seq = 0;       // sweeps launched with host publication
  int fused_mode = 0;               // SBA_FUSED: 0 (default) never, 1 always, 2 only for grids <= kFusedMaxGrid
  bool publish = true;              // SBA_PUBLISH=0: D2H copy + stream sync instead of kernel-side publication
  bool published = false;           // the last enqueued sweep publishes to pack_host itself
  hipEvent_t ev0 = nullptr, ev1 = nullptr;

  // direct peer exchange (IPC-mapped inboxes, sba_problem_peer_*)
  double* inbox = nullptr;
  sba::PeerInboxes peers{};
  void* peer_opened[sba::kMaxPeers] = {nullptr};
  bool peer_ready = false;
  unsigned long long xseq = 0;
  double peer_timeout_s = 20.0;           // longest wait for a peer's slot before SBA_ERR_COMM (SBA_PEER_TIMEOUT_S)
  int wall_clock_khz = 100000;            // rate of the device's constant wall clock (hipDeviceAttributeWallClockRate)
  unsigned long long* peer_sticky = nullptr;   // device word: some exchange timed out (never cleared while connected)

  // resident evaluator for small problems (sba_resident.hpp): command record in mapped pinned host memory
  sba::ResidentRecord* res_rec = nullptr;
  sba::ResidentRecord* res_rec_dev = nullptr;
  // One-launch stages of a small problem (a batch of one pair through batch_depth_solve_kernel / batch_lm_kernel): the pair
  // descriptor, the d-only stage's R | t, the in / out record and the completion word, in ONE mapped host block the kernel
  // reads / writes directly (sba_shim.cpp: SmallRecord).
  void* small_rec = nullptr;
  void* small_rec_dev = nullptr;
  unsigned long long small_seq = 0;
  unsigned long long res_cmd_seq = 0;     // sequence number of the last command written
  // Largest problem the LM stages / the d-only stage drive through a resident single-block kernel; above it every sweep /
  // pass is a launch.  Measured cross-over on MI355X (profiles/r03_c1_pipeline.md): one block sweeps 4 096 matches in less
  // time than two launches cost, but the d-only pass is arithmetic-heavy (4 exp + a reciprocal per match) and one CU falls
  // behind the 4-16 CUs a launch spreads it over from ~3 000 matches on.  SBA_RESIDENT_MAX_N overrides both (0 = never).
  size_t resident_max_n = 4096;
  size_t resident_max_n_depth = 2560;
  size_t one_launch_max_n_depth = 4096;     // d-only stage as ONE launch (batch of one pair): 331 us against 362 us with a launch per pass at
                                            // 4 096 matches, 405 against 344 at 6 144 (tools/small_depth_sizes.py); SBA_RESIDENT_MAX_N sets it too
  double resident_idle_s = 0.25;          // SBA_RESIDENT_IDLE_S: a resident kernel ends itself after this long without a command

  sba_allreduce_fn hook = nullptr;
  void* hook_user = nullptr;
  void* comm = nullptr;        // ncclComm_t
  int nranks = 1;
  int shard_rank = 0, shard_count = 1;   // which shard of the correspondences this problem holds (d-only stage)
};

namespace sba {
namespace shim {

// ---- RCCL, bound at run time -------------------------------------------------------------------
// The library is dlopen'ed instead of linked so that a process which already carries an RCCL
// (torch ships its own librccl.so.1) keeps exactly one copy.
struct Rccl {
  typedef struct { char internal[SBA_COMM_ID_BYTES]; } UniqueId;
  int (*GetUniqueId)(UniqueId*) = nullptr;
  int (*CommInitRank)(void**, int, UniqueId, int) = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
  void* handle = nullptr;
  bool ok = false;
  std::string why;
};
Rccl& rccl();
constexpr int kNcclFloat64 = 8;  // ncclDouble
constexpr int kNcclSum = 0;      // ncclSum

inline bool is_collective(const sba_problem* p) { return p->comm != nullptr || p->hook != nullptr || p->peer_ready; }

// sba_resident.cpp -- one resident kernel serving one solve stage of a small, unsharded problem.  start_*() launches it,
// call() sends a command and waits for its answer (restarting a kernel that ended itself: idle time-out, trip limit),
// end() sends QUIT and waits, bounded, for the stream to drain; the destructor ends a session that is still open.
bool resident_eligible(const sba_problem* p, bool depth_stage);
// The mapped host block of the one-launch stages (sba_problem::small_rec): what the batch kernels read per pair -- descriptor,
// frozen R | t of the d-only stage, the in / out record -- and the completion word they publish.
struct SmallRecord {
  sba::PairDesc desc;
  sba::BatchDepthConst cst;
  sba::BatchLmIo io;
  volatile unsigned long long seq;
  unsigned long long pad_[7];
};
// Which stages of a small problem run as ONE launch with the solver on the device.  Default: the d-only stage (its step
// logic is a few microseconds on a GPU lane: 302 us against 376 us through the resident evaluator at 2 048 matches), NOT the LM
// stages (LmSolver::feed costs 11-16 us on one lane, more than the host's step plus the command round trip: 127 / 89 us against
// 65 / 47 us for rot-only / tran-only).  SBA_SMALL_ONE_LAUNCH=0: no stage; =2: the LM stages too (A/B, tests).
inline bool small_one_launch(bool depth_stage) {
  const char* env = std::getenv("SBA_SMALL_ONE_LAUNCH");
  if (env && env[0] == '0') return false;
  if (env && env[0] == '2') return true;
  return depth_stage;
}
class ResidentSession {
 public:
  explicit ResidentSession(sba_problem* p) : p_(p) {}
  ResidentSession(const ResidentSession&) = delete;
  ResidentSession& operator=(const ResidentSession&) = delete;
  ~ResidentSession() { if (active_) (void)end(); }
  int start_sweep(int mode, int depth_mode, bool loss);
  int start_depth(double* a1, double* a2, double* b1, double* b2, double* sc1, double* sc2);
  int call(const double* payload, int count, double* out, int out_count);
  int end();
  bool active() const { return active_; }

 private:
  int launch();
  sba_problem* p_;
  bool active_ = false;
  bool depth_ = false;
  int mode_ = 0, depth_mode_ = 0;
  bool loss_ = true;
  double *a1_ = nullptr, *a2_ = nullptr, *b1_ = nullptr, *b2_ = nullptr, *sc1_ = nullptr, *sc2_ = nullptr;
  unsigned long long pending_cmd_ = 0, pending_pack_ = 0;   // what the next launched kernel waits for / answers with
};

// sba_shim.cpp -- the plane helpers the other entry points share.
// ensure_plane: slot k holds at least `bytes` bytes, zeroed (enqueued).  alloc_planes: the zeroed, staggered planes of an
// upload of n matches (slots 0..7; the handle is not `uploaded` until the caller says so).  ensure_folded: the folded
// planes brought up to date if the handle sweeps them.  sweep_planes: what a single-problem sweep of `depth_mode` streams
// and the kernel variant that reads them (sba::kDepthFolded for the folded planes).  check_args: the argument checks of
// every sweep entry point.
int ensure_plane(sba_problem* p, int k, size_t bytes);
int alloc_planes(sba_problem* p, size_t n, bool with_d12, int store);
int ensure_folded(sba_problem* p);
int sweep_planes(sba_problem* p, int depth_mode, sba::Planes* pl, int* kernel_depth);
int check_args(const sba_problem* p, int mode, int depth_mode, const double* rot, const double* tran);

// sba_select.cpp -- the compaction behind sba_problem_compact, for callers whose keep bytes are already on the device
// (sba_quantile.cpp).  compact_alloc: the device scratch of one compaction of the handle's n > 0 matches, the keep bytes
// zeroed beyond n (enqueued); the caller then queues the n keep bytes on the handle's stream.  compact_rows: everything
// sba_problem_compact does after that.
struct CompactWork {
  explicit CompactWork(const int* poison) : buf(poison) {}
  sba::DeviceBuffer buf;
  size_t ntiles = 0;
  unsigned char* keep = nullptr;
  unsigned int* tile_count = nullptr;
  unsigned long long* tile_offset = nullptr;
  unsigned long long* total = nullptr;
};
int compact_alloc(sba_problem* p, CompactWork* w);
int compact_rows(sba_problem* p, CompactWork& w, size_t* n_kept, long long* kept_index);

// sba_covariance.cpp -- everything sba_problem_covariance_joint does before its per-match pass, for the entry points that
// follow it with a per-match pass of their own (sba_structure.cpp): argument checks and refusals, the reduce pass, the host
// finish.  front_elems: doubles the caller wants at the front of the handle's d-only scratch (cp->front, 256-byte aligned).
// On success cp holds the planes, the pass's JointParams, the grid and the result record; on failure nothing is enqueued
// beyond the reduce pass and the handle stays usable.
struct CovPass {
  sba::Planes pl;
  sba::JointParams prm;
  int grid = 0;
  sba_joint_cov res;
  double* front = nullptr;
};
int cov_first_pass(sba_problem* p, const double rot[3], const double tran[3], const sba_lm_options* opt, double min_sin2_parallax,
                   size_t front_elems, CovPass* cp);

// sba_quantile.cpp -- the selection over a plane of n per-match values that is already on the device, for callers that
// write the plane themselves (sba_structure.cpp).  select_plane: the handle's select scratch sized for num_ranks ranks,
// *plane = its per-match plane (plane_elems doubles).  select_enqueue: ranks (and, with scale, the threshold scale *
// value[0]) over plane[0 .. n); host_offsets (2 words), ranks and scale stay valid until the caller has waited for the stream.
// select_values / select_keep: what sba_problem_residual_order_stats / sba_problem_keep_below do after their selection.
int select_plane(sba_problem* p, int num_ranks, sba::SelectScratch* s, double** plane);
int select_enqueue(sba_problem* p, const sba::SelectScratch& s, const size_t* ranks, int num_ranks, const double* scale,
                   unsigned long long* host_offsets);
int select_values(sba_problem* p, const sba::SelectScratch& s, int num_ranks, double* values);
int select_keep(sba_problem* p, const sba::SelectScratch& s, double* threshold, size_t* n_kept, long long* kept_index);

// sba_transport.cpp
int allreduce_pack(sba_problem* p);                                  // p->pack_dev (24 doubles), then hand-over to the host
int allreduce_buffer(sba_problem* p, double* dev, size_t count);     // any device buffer, count a multiple of 24
// sba_shim.cpp
int fetch_pack_raw(sba_problem* p, double raw[SBA_PACK_SIZE]);       // wait for the pack handed over by the last sweep / pass

}  // namespace shim
}  // namespace sba
