// Batched joint solve on the device: every pair's depths, rotation and translation free together (the reference's
// ba_spherical_costfunctor, spherical_bundle_adjuster.cpp:843-889, once per pair of a batch).  The passes are those of
// sba_joint.hip: its per-match block and fold, and its two per-match loops (sba_joint_reduce_loop.inc / sba_joint_step_loop.inc,
// the one text both files compile) as joint_reduce_stream / joint_step_stream over a pair layout (sba_joint_core.hpp), run by
// ONE 256-thread block per pair:
//   batch_joint_pass_kernel   one pass (reduce or step) of every pair that takes part, from a per-pair record; the pair's row is
//                             published to mapped host memory, the last block stores the sequence word the host polls
//                             (sba_batch_eval_joint and the lock-step driver of sba_batch_solve_joint)
//   batch_joint_solve_kernel  the whole joint LM of every pair in one launch: the pair's JointSolver (sba_joint_solver.hpp, the
//                             class the host drives) lives in LDS, thread 0 feeds it the folded row and builds the next pass
// Block shape: the reduce body needs ~350 registers, which fits one wave per SIMD only (joint_reduce_kernel is
// __launch_bounds__(256, 1) for that reason); a 512-thread block as the d-only batch kernels use would halve the budget and
// spill into the hot loop.  A pair's sums are formed in an order that depends on the pair's own matches only: lane = vector
// index mod 256, lanes by DPP, the four waves in wave order -- whatever the other pairs of the batch and the pair layout are.
// No atomics on data (the ticket word is the only atomic), no scratch, 16-byte accesses on the f64 planes.
#include <cfloat>
#include <new>

#include "sba_device.hpp"
#include "sba_joint_core.hpp"
#include "sba_publish.hpp"

namespace sba {
namespace {

constexpr int kJointBlock = 256;

// The JointParams of one pass from what a JointPassRequest (or a BatchJointPass record) carries: the device-side twin of
// joint_reduce_pass / joint_step_pass in sba_joint.cpp.  Thread 0 only.
__device__ __forceinline__ void joint_fill_params(int kind, bool first, double radius, const double rot[3], const double tran[3],
                                                  const double rot_cand[3], const double tran_cand[3], const double delta_c[6],
                                                  unsigned long long n, const sba_lm_options& o, JointParams* P) {
  fill_sweep_params(n, SBA_DEPTH_PER_MATCH, rot, tran, 1.0, 1.0, o.huber_delta, &P->cur, false);
  if (kind == kJointStep) fill_sweep_params(n, SBA_DEPTH_PER_MATCH, rot_cand, tran_cand, 1.0, 1.0, o.huber_delta, &P->cand, false);
  double B[9];
  factored_frame(rot, B, P->J);
  P->small_angle = !(rot[0] * rot[0] + rot[1] * rot[1] + rot[2] * rot[2] > DBL_EPSILON) ? 1 : 0;
#pragma unroll
  for (int k = 0; k < 6; ++k) P->delta_c[k] = kind == kJointStep ? delta_c[k] : 0.0;
  P->inv_radius = 1.0 / radius;
  P->min_diagonal = o.min_lm_diagonal; P->max_diagonal = o.max_lm_diagonal;
  P->first = kind == kJointReduce && first ? 1 : 0;
  P->jacobi_scaling = o.jacobi_scaling ? 1 : 0;
  P->pad_ = 0;
}

// What the streams read of a pass's parameters, LDS -> registers (the Gn blocks of the two SweepParams are never read).
__device__ __forceinline__ void joint_take_params(const JointParams& s, JointParams& P) {
#pragma unroll
  for (int k = 0; k < 9; ++k) { P.cur.Rn[k] = s.cur.Rn[k]; P.cand.Rn[k] = s.cand.Rn[k]; P.J[k] = s.J[k]; }
#pragma unroll
  for (int k = 0; k < 3; ++k) { P.cur.t[k] = s.cur.t[k]; P.cand.t[k] = s.cand.t[k]; }
#pragma unroll
  for (int k = 0; k < 6; ++k) P.delta_c[k] = s.delta_c[k];
  P.cur.d2 = s.cur.d2; P.cur.delta = s.cur.delta; P.cur.delta2 = s.cur.delta2; P.cur.n = s.cur.n;
  P.cand.d2 = s.cand.d2; P.cand.delta = s.cand.delta; P.cand.delta2 = s.cand.delta2; P.cand.n = s.cand.n;
  P.inv_radius = s.inv_radius; P.min_diagonal = s.min_diagonal; P.max_diagonal = s.max_diagonal;
  P.small_angle = s.small_angle; P.first = s.first; P.jacobi_scaling = s.jacobi_scaling; P.pad_ = 0;
}

// One pass of the block's pair: stream + fold; res[0 .. count) (LDS) holds the pair's row on threads < count afterwards (each
// of those threads wrote its own slot; a barrier makes the row visible to the others).  kind, flip: block-uniform.
template <typename ST>
__device__ __forceinline__ void batch_joint_run_pass(const Planes& pl, const BatchPairMap<ST>& map, const JointParams& prm_s, int kind,
                                                     bool flip, double* __restrict__ a1, double* __restrict__ a2,
                                                     double* __restrict__ b1, double* __restrict__ b2, double* __restrict__ sc1,
                                                     double* __restrict__ sc2, double (*red_r)[JOINT_OUT_COUNT],
                                                     double (*red_s)[JOINT_STEP_COUNT], double* __restrict__ res) {
  JointParams P;
  joint_take_params(prm_s, P);
  const double *cur1 = flip ? b1 : a1, *cur2 = flip ? b2 : a2;
  if (kind == kJointReduce) {
    double acc[JOINT_OUT_COUNT];
    joint_reduce_stream<ST, BatchPairMap<ST>>(pl, cur1, cur2, sc1, sc2, P, static_cast<size_t>(threadIdx.x), kJointBlock, acc, map);
    joint_block_fold<JOINT_OUT_COUNT, JOINT_OUT_GDMAX>(acc, red_r, res);
  } else {
    double acc[JOINT_STEP_COUNT];
    joint_step_stream<ST, BatchPairMap<ST>>(pl, cur1, cur2, flip ? a1 : b1, flip ? a2 : b2, sc1, sc2, P,
                                            static_cast<size_t>(threadIdx.x), kJointBlock, acc, map);
    joint_block_fold<JOINT_STEP_COUNT, -1>(acc, red_s, res);
  }
}

template <typename ST>
__global__ __launch_bounds__(kJointBlock, 1) void batch_joint_pass_kernel(Planes pl, const PairDesc* __restrict__ desc,
                                                                         const BatchJointPass* __restrict__ pass, sba_lm_options opt,
                                                                         double* __restrict__ a1, double* __restrict__ a2,
                                                                         double* __restrict__ b1, double* __restrict__ b2,
                                                                         double* __restrict__ sc1, double* __restrict__ sc2,
                                                                         double* __restrict__ out_host, unsigned int* __restrict__ ticket,
                                                                         unsigned long long seq) {
  __shared__ double red_r[4][JOINT_OUT_COUNT];
  __shared__ double red_s[4][JOINT_STEP_COUNT];
  __shared__ double res_s[JOINT_ROW];
  __shared__ JointParams prm_s;
  __shared__ int kind_s, flip_s;
  __shared__ unsigned long long n_s;
  const unsigned pair = blockIdx.x;
  const int tid = threadIdx.x;
  const PairDesc dsc = desc[pair];
  if (tid < JOINT_ROW) res_s[tid] = 0.0;
  if (tid == 0) {
    const BatchJointPass ps = pass[pair];                   // mapped host memory: one read of the pair's record
    const unsigned long long n = ps.n < dsc.n ? ps.n : dsc.n;      // never past the pair's own matches, whatever the record says
    n_s = n;
    kind_s = ps.kind == kJointStep ? kJointStep : kJointReduce;
    flip_s = (ps.flags >> 3) & 1;
    if (n > 0) joint_fill_params(kind_s, (ps.flags & 1) != 0, ps.radius, ps.rot, ps.tran, ps.rot_cand, ps.tran_cand, ps.delta_c, n, opt, &prm_s);
  }
  __syncthreads();
  if (n_s > 0)                                              // block-uniform: an LDS word read after the barrier
    batch_joint_run_pass<ST>(pl, BatchPairMap<ST>{dsc}, prm_s, kind_s, flip_s != 0, a1, a2, b1, b2, sc1, sc2, red_r, red_s, res_s);
  if (tid >= 64) return;                  // wave 0 finishes alone: every slot of the row was written by the thread that stores it
  if (tid < JOINT_OUT_COUNT) host_store(out_host + static_cast<size_t>(pair) * JOINT_ROW + tid, res_s[tid]);
  host_release();
  if (tid == 0 && __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1) {
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(out_host + static_cast<size_t>(gridDim.x) * JOINT_ROW), seq,
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}
static_assert(JOINT_OUT_COUNT <= 64 && JOINT_STEP_COUNT <= JOINT_OUT_COUNT && JOINT_OUT_COUNT <= JOINT_ROW, "wave 0 publishes a row");

// The whole joint LM of a pair in ONE launch.  Loop shape as batch_depth_solve_kernel / batch_lm_kernel: the thread-0 region of
// a trip sits between two barriers of that trip, the trip bound is a counter every thread keeps, the exit decision is read from
// LDS after the second barrier.  max_trips = batch_joint_pass_bound(opt): every reduce pass either finishes the solve or
// increments the solver's iteration counter, an iteration has at most one step pass -- at most 2 * max_num_iterations + 2
// passes; a pair whose bound runs out all the same is reported with SBA_ERR_NUMERIC, never silently.
template <typename ST>
__global__ __launch_bounds__(kJointBlock, 1) void batch_joint_solve_kernel(Planes pl, const PairDesc* __restrict__ desc, sba_lm_options opt,
                                                                          double* __restrict__ a1, double* __restrict__ a2,
                                                                          double* __restrict__ b1, double* __restrict__ b2,
                                                                          double* __restrict__ sc1, double* __restrict__ sc2,
                                                                          const unsigned long long* __restrict__ offsets,
                                                                          double* __restrict__ out, BatchLmIo* __restrict__ io,
                                                                          unsigned int* __restrict__ ticket,
                                                                          unsigned long long* __restrict__ seq_host, unsigned long long seq,
                                                                          int max_trips) {
  __shared__ double red_r[4][JOINT_OUT_COUNT];
  __shared__ double red_s[4][JOINT_STEP_COUNT];
  __shared__ double res_s[JOINT_ROW];
  __shared__ JointParams prm_s;
  __shared__ int kind_s, flip_s, done_s, passes_s, refused_s;
  __shared__ alignas(16) unsigned char solver_mem[sizeof(JointSolver)];
  JointSolver* solver = reinterpret_cast<JointSolver*>(solver_mem);
  const unsigned pair = blockIdx.x;
  const int tid = threadIdx.x;
  const PairDesc dsc = desc[pair];
  const BatchPairMap<ST> map{dsc};
  if (tid == 0) {
    const BatchLmIo in = io[pair];                          // mapped host memory: one read here, one write at the end
    new (solver) JointSolver();
    solver->start(in.rot, in.tran, opt);
    refused_s = in.status != 0 ? 1 : 0;                     // a non-finite start: no pass runs, the pair's depths stay as they are
    flip_s = 0;
    passes_s = 0;
  }
  for (int trip = 0; trip <= max_trips; ++trip) {      // the trip after the last pass only feeds its row (and breaks below)
    __syncthreads();                        // B0: the previous pass's row is in res_s
    if (tid == 0) {
      if (trip > 0) {
        solver->feed(res_s);
        if (solver->take_candidate()) flip_s ^= 1;
      }
      done_s = solver->done() || refused_s ? 1 : 0;
      if (!done_s) {
        const JointPassRequest& rq = solver->request();
        kind_s = rq.kind;
        joint_fill_params(rq.kind, rq.first, rq.radius, rq.rot, rq.tran, rq.rot_cand, rq.tran_cand, rq.delta_c, dsc.n, opt, &prm_s);
        if (trip < max_trips) ++passes_s;
      }
    }
    __syncthreads();                        // B1: done_s / the next pass are visible to the block
    if (done_s || trip == max_trips) break; // both block-uniform: an LDS word read after B1, the trip counter
    batch_joint_run_pass<ST>(pl, map, prm_s, kind_s, flip_s != 0, a1, a2, b1, b2, sc1, sc2, red_r, red_s, res_s);
  }
  __syncthreads();                          // flip_s is final; every store of the last pass has been issued by its thread
  {
    const bool fl = flip_s != 0;            // as batch_depth_finish_kernel, for this block's own pair
    const size_t npairs = (dsc.n + 1) / 2;
    if (fl || out)
      for (size_t pr = tid; pr < npairs; pr += kJointBlock) {
        const size_t q = map(pr);
        const double2 u = reinterpret_cast<const double2*>(fl ? b1 : a1)[q], v = reinterpret_cast<const double2*>(fl ? b2 : a2)[q];
        if (fl) { reinterpret_cast<double2*>(a1)[q] = u; reinterpret_cast<double2*>(a2)[q] = v; }
        if (out) {
          const size_t i = offsets[pair] + 2 * pr;
          reinterpret_cast<double2*>(out)[i] = make_double2(u.x, v.x);
          if (2 * pr + 1 < dsc.n) reinterpret_cast<double2*>(out)[i + 1] = make_double2(u.y, v.y);
        }
      }
  }
  if (tid == 0) {
    BatchLmIo* res = io + pair;             // field by field: a local record would be assembled in scratch memory
    for (int a = 0; a < 3; ++a) { res->rot[a] = solver->rot()[a]; res->tran[a] = solver->tran()[a]; }
    res->d1 = 0.0; res->d2 = 0.0;
    res->summary = solver->summary();
    res->status = refused_s ? SBA_ERR_NUMERIC : (solver->done() ? solver->status() : SBA_ERR_NUMERIC);   // the bound ran out: never silent
    res->pad_ = passes_s;
    if (seq_host) {                         // completion as batch_lm_kernel: record in host memory, then a ticket
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      if (__hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1) {
        __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
        __hip_atomic_store(seq_host, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      }
    }
  }
}

}  // namespace

hipError_t launch_batch_joint_pass(int store, const Planes& pl, const PairDesc* desc, const BatchJointPass* pass_host_dev, int num_pairs,
                                   const sba_lm_options& opt, double* a1, double* a2, double* b1, double* b2, double* sc1, double* sc2,
                                   double* out_host_dev, unsigned int* ticket, unsigned long long seq, hipStream_t stream) {
  if (num_pairs <= 0) return hipSuccess;
  if (store == 0)
    hipLaunchKernelGGL((batch_joint_pass_kernel<double>), dim3(num_pairs), dim3(kJointBlock), 0, stream, pl, desc, pass_host_dev, opt, a1, a2,
                       b1, b2, sc1, sc2, out_host_dev, ticket, seq);
  else
    hipLaunchKernelGGL((batch_joint_pass_kernel<float>), dim3(num_pairs), dim3(kJointBlock), 0, stream, pl, desc, pass_host_dev, opt, a1, a2,
                       b1, b2, sc1, sc2, out_host_dev, ticket, seq);
  return hipGetLastError();
}

hipError_t launch_batch_joint_solve(int store, const Planes& pl, const PairDesc* desc, int num_pairs, const sba_lm_options& opt,
                                    double* a1, double* a2, double* b1, double* b2, double* sc1, double* sc2,
                                    const unsigned long long* offsets_dev, double* out_dev, BatchLmIo* io, unsigned int* ticket,
                                    unsigned long long* seq_host_dev, unsigned long long seq, hipStream_t stream) {
  if (num_pairs <= 0) return hipSuccess;
  const int max_trips = batch_joint_pass_bound(opt);
  if (store == 0)
    hipLaunchKernelGGL((batch_joint_solve_kernel<double>), dim3(num_pairs), dim3(kJointBlock), 0, stream, pl, desc, opt, a1, a2, b1, b2,
                       sc1, sc2, offsets_dev, out_dev, io, ticket, seq_host_dev, seq, max_trips);
  else
    hipLaunchKernelGGL((batch_joint_solve_kernel<float>), dim3(num_pairs), dim3(kJointBlock), 0, stream, pl, desc, opt, a1, a2, b1, b2,
                       sc1, sc2, offsets_dev, out_dev, io, ticket, seq_host_dev, seq, max_trips);
  return hipGetLastError();
}

}  // namespace sba
