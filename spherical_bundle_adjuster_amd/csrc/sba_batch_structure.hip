// Batched triangulated structure on the device: what structure_kernel (sba_structure.hip) computes for one problem -- per match
// the midpoint X of the two ray ends, its 3 x 3 covariance and the score trace / X.X -- for every pair of a batch in one launch
// that follows batch_cov_kernel's reduce + finish launch on the same stream.  Grid (num_pairs, blocks per pair), 256-thread
// blocks: block (g, y) runs sba_structure_loop.inc over pair g's layout from vector y * 256 + tid with stride 256 * gridDim.y.
// The prologue is batch_cov_kernel's: thread 0 builds the pair's pass parameters in LDS from the pair's record (rot, tran) with
// cov_fill_params, Sigma_c and the finish's verdict come from the record that launch left.  The loop reads the parameters from
// LDS, as structure_kernel does.  Rows go to the caller's row order (pair g's match i at row offsets[g] + i), exactly n rows
// per pair; a pair whose finish failed gets `fill` in every row of every output asked for, without arithmetic.
// No reduction, no atomics: every value depends on its own match, the pose and Sigma_c alone, so the bits are the same for
// every number of blocks per pair, for either pair layout and for every row parity.
// Bytes per match (f64 planes): reads 64; writes 24 (xyz), 48 (cov: xx, yy, zz, xy, xz, yz), 8 (score) -- only the outputs
// the instantiation was compiled for.
#include "sba_batch_cov_device.hpp"
#include "sba_covariance.hpp"
#include "sba_device.hpp"
#include "sba_joint_core.hpp"
#include "sba_pair_map.hpp"
#include "sba_structure.hpp"

namespace sba {
namespace {

constexpr int kStructBlock = 256;

// A lane's two rows into cov[row0 + 2 pr][6] (48-byte rows: always 16-byte aligned) and score[row0 + 2 pr] (one 16-byte store
// when the pair's first row is even and both matches exist).  xyz rows: CovStoreRows.
struct StructureStoreRows {
  double *xyz, *cov, *score;
  size_t row0, n;
  template <bool WANT_XYZ, bool WANT_COV, bool WANT_SCORE>
  __device__ __forceinline__ void put(size_t pr, bool both, const double (&X)[2][3], const double (&cv)[2][6],
                                      const double (&q)[2]) const {
    if (WANT_XYZ) CovStoreRows{xyz, row0, n}(pr, X);
    if (WANT_COV) {
      double* p = cov + 6 * (row0 + 2 * pr);
#pragma unroll
      for (int k = 0; k < 3; ++k) *reinterpret_cast<double2*>(p + 2 * k) = make_double2(cv[0][2 * k], cv[0][2 * k + 1]);
      if (both) {
#pragma unroll
        for (int k = 0; k < 3; ++k) *reinterpret_cast<double2*>(p + 6 + 2 * k) = make_double2(cv[1][2 * k], cv[1][2 * k + 1]);
      }
    }
    if (WANT_SCORE) {
      double* p = score + row0 + 2 * pr;
      if (both && (row0 & 1) == 0) {
        *reinterpret_cast<double2*>(p) = make_double2(q[0], q[1]);
      } else {
        p[0] = q[0];
        if (both) p[1] = q[1];
      }
    }
  }
};

template <typename ST, bool WANT_XYZ, bool WANT_COV, bool WANT_SCORE>
__global__ __launch_bounds__(kStructBlock) void batch_structure_kernel(Planes pl, const PairDesc* __restrict__ desc, sba_lm_options opt,
                                                                       double min_sin2, double fill,
                                                                       const unsigned long long* __restrict__ offsets,
                                                                       const BatchCovRec* __restrict__ rec, double* __restrict__ xyz,
                                                                       double* __restrict__ cov, double* __restrict__ score) {
  __shared__ JointParams prm_s;
  __shared__ double sigma_s[36];
  __shared__ int ok_s;
  const unsigned pair = blockIdx.x;
  const int tid = threadIdx.x;
  const PairDesc dsc = desc[pair];
  const BatchPairMap<ST> map{dsc};
  const BatchCovRec* const r = rec + pair;                 // mapped host memory: what the reduce + finish launch published
  if (tid == 0) {
    double rot[3], tran[3];
    for (int a = 0; a < 3; ++a) { rot[a] = r->rot[a]; tran[a] = r->tran[a]; }
    cov_fill_params(rot, tran, dsc.n, opt, &prm_s);
    ok_s = (r->dim_status >> 32) == 0 ? 1 : 0;
  }
  if (tid >= 64 && tid < 64 + 36) sigma_s[tid - 64] = r->sigma[tid - 64];
  __syncthreads();
  const size_t n = dsc.n, row0 = offsets[pair];
  const size_t first = static_cast<size_t>(blockIdx.y) * kStructBlock + tid, step = static_cast<size_t>(kStructBlock) * gridDim.y;
  if (!ok_s) {                              // block-uniform: an LDS word read after a barrier
    for (size_t i = first; i < n; i += step) {
      if (WANT_XYZ) { double* p = xyz + 3 * (row0 + i); p[0] = fill; p[1] = fill; p[2] = fill; }
      if (WANT_COV) {
        double* p = cov + 6 * (row0 + i);
#pragma unroll
        for (int k = 0; k < 3; ++k) *reinterpret_cast<double2*>(p + 2 * k) = make_double2(fill, fill);
      }
      if (WANT_SCORE) score[row0 + i] = fill;
    }
    return;
  }
  const JointParams& P = prm_s;
  const double* sigma_c = sigma_s;
  const double* const d1 = pl.d1;
  const double* const d2 = pl.d2;
  const size_t npairs = (n + 1) / 2, stride = step;
  size_t pr = first;
  const StructureStoreRows rows{xyz, cov, score, row0, n};
  const auto store = [rows](size_t p, bool both, const double (&X)[2][3], const double (&cv)[2][6], const double (&q)[2]) {
    rows.template put<WANT_XYZ, WANT_COV, WANT_SCORE>(p, both, X, cv, q);
  };
#include "sba_structure_loop.inc"
}

template <typename ST>
void launch_for(int which, dim3 grid, hipStream_t stream, const Planes& pl, const PairDesc* desc, const sba_lm_options& opt,
                double min_sin2, double fill, const unsigned long long* offsets, const BatchCovRec* rec, double* xyz, double* cov,
                double* score) {
#define SBA_BATCH_STRUCTURE_CASE(W, X, C, S)                                                                             \
  case W: hipLaunchKernelGGL((batch_structure_kernel<ST, X, C, S>), grid, dim3(kStructBlock), 0, stream, pl, desc, opt, min_sin2, \
                             fill, offsets, rec, xyz, cov, score); break;
  switch (which) {
    SBA_BATCH_STRUCTURE_CASE(1, true, false, false)
    SBA_BATCH_STRUCTURE_CASE(2, false, true, false)
    SBA_BATCH_STRUCTURE_CASE(3, true, true, false)
    SBA_BATCH_STRUCTURE_CASE(4, false, false, true)
    SBA_BATCH_STRUCTURE_CASE(5, true, false, true)
    SBA_BATCH_STRUCTURE_CASE(6, false, true, true)
    SBA_BATCH_STRUCTURE_CASE(7, true, true, true)
    default: break;
  }
#undef SBA_BATCH_STRUCTURE_CASE
}

}  // namespace

hipError_t launch_batch_structure(int store, const Planes& pl, const PairDesc* desc, int num_pairs, int blocks_per_pair,
                                  const sba_lm_options& opt, double min_sin2, double fill, const unsigned long long* offsets_dev,
                                  const BatchCovRec* rec, double* xyz, double* cov, double* score, hipStream_t stream) {
  const int which = (xyz ? 1 : 0) | (cov ? 2 : 0) | (score ? 4 : 0);
  if (num_pairs <= 0 || blocks_per_pair <= 0 || which == 0) return hipSuccess;
  const dim3 grid(num_pairs, blocks_per_pair);
  if (store == 0) launch_for<double>(which, grid, stream, pl, desc, opt, min_sin2, fill, offsets_dev, rec, xyz, cov, score);
  else launch_for<float>(which, grid, stream, pl, desc, opt, min_sin2, fill, offsets_dev, rec, xyz, cov, score);
  return hipGetLastError();
}

}  // namespace sba
