// Batched joint covariance on the device: what sba_covariance.hip's two passes and the host finish between them compute for one
// problem, for every pair of a batch in ONE launch -- one 256-thread block per pair, as the batched joint solve
// (sba_batch_joint.hip), in three phases:
//   reduce   the body of cov_reduce_kernel (sba_cov_reduce_loop.inc) over the pair's layout, stride 256, folded to one LDS row
//   finish   thread 0 runs cov_finish (sba_covariance.hpp, the text the host runs) on that row: Sigma_c and dim to LDS
//   depth    the body of cov_depth_kernel (sba_cov_depth_loop.inc) with Sigma_c read from LDS, three doubles per match to the
//            caller's row order; NaN rows for a pair whose finish failed
// The pass parameters are built by thread 0 in LDS and taken into scalar registers (they are block-uniform), Sigma_c stays in
// LDS: nothing of the 1.5 KB that cov_depth_kernel receives as kernel arguments travels that way here.
// `phases` selects the phases of a launch: all of them (the one-launch driver), or reduce alone and depth alone with the host's
// cov_finish in between (the lock-step driver, SBA_BATCH_DEVICE_COV=0) -- the same machine code either way.
// A pair's sums are formed in an order that depends on the pair's own matches only (lane = vector index mod 256, lanes by DPP,
// the four waves in wave order).  No atomics on data (the ticket word is the only atomic), no scratch.
#include "sba_batch_cov_device.hpp"
#include "sba_covariance.hpp"
#include "sba_device.hpp"
#include "sba_joint_core.hpp"
#include "sba_publish.hpp"

namespace sba {
namespace {

constexpr int kCovBlock = 256;
static_assert(COV_ROW == 32 && COV_OUT_COUNT <= 64, "BatchCovRec::row holds a row; wave 0 publishes it");

template <typename ST>
__global__ __launch_bounds__(kCovBlock, 2) void batch_cov_kernel(Planes pl, const PairDesc* __restrict__ desc, sba_lm_options opt,
                                                                double min_sin2, int phases,
                                                                const unsigned long long* __restrict__ offsets,
                                                                double* __restrict__ out, BatchCovRec* __restrict__ rec,
                                                                unsigned int* __restrict__ ticket,
                                                                unsigned long long* __restrict__ seq_host, unsigned long long seq) {
  __shared__ double red[4][COV_OUT_COUNT];
  __shared__ double row_s[COV_ROW];
  __shared__ double sigma_s[36];
  __shared__ double tran_s[3];
  __shared__ JointParams prm_s;
  __shared__ int dim_s, ok_s, refused_s;
  __shared__ alignas(16) unsigned char work_mem[sizeof(CovFinishWork)];
  const unsigned pair = blockIdx.x;
  const int tid = threadIdx.x;
  const PairDesc dsc = desc[pair];
  const BatchPairMap<ST> map{dsc};
  BatchCovRec* const r = rec + pair;                       // mapped host memory
  if (tid < COV_ROW) row_s[tid] = 0.0;
  if (tid == 0) {
    double rot[3];
    for (int a = 0; a < 3; ++a) { rot[a] = r->rot[a]; tran_s[a] = r->tran[a]; }
    cov_fill_params(rot, tran_s, dsc.n, opt, &prm_s);
    refused_s = r->refused != 0 ? 1 : 0;
    dim_s = 0; ok_s = 0;
    if (!(phases & kCovFinish)) {                          // the lock-step driver's depth launch: the host's finish
      for (int k = 0; k < 36; ++k) sigma_s[k] = r->sigma[k];
      const unsigned long long ds = r->dim_status;
      dim_s = static_cast<int>(ds & 0xffffffffull);
      ok_s = (ds >> 32) == 0 ? 1 : 0;
    }
  }
  __syncthreads();
  JointParams P;
  cov_take_params(prm_s, P);
  P.cur.n = dsc.n;
  const double* const d1 = pl.d1;
  const double* const d2 = pl.d2;
  const size_t n = dsc.n, npairs = (n + 1) / 2, stride = kCovBlock;
  if (phases & kCovReduce) {
    double acc[COV_OUT_COUNT];
#pragma unroll
    for (int k = 0; k < COV_OUT_COUNT; ++k) acc[k] = 0.0;
    size_t pr = static_cast<size_t>(tid);
#include "sba_cov_reduce_loop.inc"
    joint_block_fold<COV_OUT_COUNT, -1>(acc, red, row_s);  // row_s[k] is written by thread k
  }
  if (phases & kCovFinish) {
    __syncthreads();                        // the row is in row_s
    if (tid == 0) {
      const int m = opt.tran_param == SBA_TRAN_SPHERE ? 5 : 6;
      int dim = m;
      const bool ok = !refused_s && cov_finish(row_s + COV_OUT_S, opt.tran_param, tran_s, static_cast<long long>(row_s[COV_OUT_NUSED]),
                                               sigma_s, &dim, reinterpret_cast<CovFinishWork*>(work_mem));
      if (!ok)                              // NaN, not zero: a zero covariance reads as certainty
        for (int k = 0; k < 36; ++k) sigma_s[k] = __builtin_nan("");
      dim_s = ok ? dim : m;
      ok_s = ok ? 1 : 0;
    }
    __syncthreads();                        // Sigma_c, dim_s and ok_s are visible to the block
  }
  if ((phases & kCovDepth) && out) {
    const size_t row0 = offsets[pair];
    if (ok_s) {                             // block-uniform: an LDS word read after a barrier
      const double* sigma_c = sigma_s;
      const CovStoreRows store{out, row0, n};
      size_t pr = static_cast<size_t>(tid);
#include "sba_cov_depth_loop.inc"
    } else {
      const double nan = __builtin_nan("");
      for (size_t i = static_cast<size_t>(tid); i < n; i += kCovBlock) {
        double* p = out + 3 * (row0 + i);
        p[0] = nan; p[1] = nan; p[2] = nan;
      }
    }
  }
  if (tid >= 64) return;                    // wave 0 publishes: every word it stores below it wrote itself or reads after a barrier
  if ((phases & kCovReduce) && tid < COV_OUT_COUNT) host_store(r->row + tid, row_s[tid]);
  if (phases & kCovFinish) {
    if (tid < 36) host_store(r->sigma + tid, sigma_s[tid]);
    if (tid == 0) host_store(&r->dim_status, static_cast<unsigned long long>(static_cast<unsigned>(dim_s)) | (ok_s ? 0ull : 1ull << 32));
  }
  host_release();
  if (tid == 0 && __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1) {
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    __hip_atomic_store(seq_host, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

}  // namespace

hipError_t launch_batch_cov(int store, const Planes& pl, const PairDesc* desc, int num_pairs, const sba_lm_options& opt,
                            double min_sin2, int phases, const unsigned long long* offsets_dev, double* out, BatchCovRec* rec,
                            unsigned int* ticket, unsigned long long* seq_host_dev, unsigned long long seq, hipStream_t stream) {
  if (num_pairs <= 0) return hipSuccess;
  if (store == 0)
    hipLaunchKernelGGL((batch_cov_kernel<double>), dim3(num_pairs), dim3(kCovBlock), 0, stream, pl, desc, opt, min_sin2, phases,
                       offsets_dev, out, rec, ticket, seq_host_dev, seq);
  else
    hipLaunchKernelGGL((batch_cov_kernel<float>), dim3(num_pairs), dim3(kCovBlock), 0, stream, pl, desc, opt, min_sin2, phases,
                       offsets_dev, out, rec, ticket, seq_host_dev, seq);
  return hipGetLastError();
}

}  // namespace sba
