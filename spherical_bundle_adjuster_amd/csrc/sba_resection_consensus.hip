// The robust resection guess on the device (entry points: sba_resection_consensus.cpp; sampler, trial moments and pick:
// sba_resection_consensus.hpp; per-match code: sba_resection_core.hpp):
//   resect_gather_kernel          the sampled rows (X = d1 x1 as resect_match rounds it, y) out of the planes; one thread per row
//   resect_score_kernel           for EVERY candidate pose the number of matches with |r|^2 <= tau^2, one streaming pass
//   resect_inlier_moments_kernel  resect_moments_kernel over the inliers of one pose only: the 60 DLT sums and their count
// The score pass is the compute-bound one of the family: a lane keeps the matches of its 16-byte vectors in registers and
// loops over the candidates, whose 12 doubles Rn | t are wave-uniform and come through scalar loads of the table (the
// next candidate's are requested before the current one is evaluated) -- they are scalar operands of the multiply-adds
// and cost no vector register.  Per candidate the wave's count is a ballot and a population count; lane (k & 63) keeps
// candidate k's count in its counter register (k >> 6).  Nothing floating-point is ever summed: the counts leave the block as
// integer adds, so they are the same for every grid and on every run.
#include "sba_device.hpp"
#include "sba_resection_consensus.hpp"
#include "sba_resection_core.hpp"

namespace sba {
namespace {

constexpr int kScoreGroups = SBA_RESECT_MAX_TRIALS / 64;     // counter registers per lane

template <typename ST>
__global__ __launch_bounds__(256) void resect_gather_kernel(Planes pl, const long long* __restrict__ index, int rows,
                                                            double* __restrict__ out) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= rows) return;
  const size_t i = static_cast<size_t>(index[k]);
  const double d1 = pl.d1[i];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    out[SBA_RESECT_ROW * k + c] = mul_rounded(d1, static_cast<double>(static_cast<const ST*>(pl.x1[c])[i]));
    out[SBA_RESECT_ROW * k + 3 + c] = static_cast<double>(static_cast<const ST*>(pl.x2[c])[i]);
  }
}

// Rn | t of candidate k out of the table: a uniform address, scalar loads.
__device__ __forceinline__ void score_candidate(const double* __restrict__ table, int k, ResectParams& P) {
  const double* c = table + static_cast<size_t>(SBA_RESECT_CANDIDATE) * k;
#pragma unroll
  for (int i = 0; i < 9; ++i) P.Rn[i] = c[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) P.t[i] = c[9 + i];
}

// At least two resident blocks per CU; the matches of a step (14 registers each), the double buffer (28 with f64 planes) and
// the 16 counters need 112 registers with f64 planes and 158 with f32, so four and three blocks fit and the grid uses them
// (resect_score_blocks_per_cu): the other waves of a SIMD cover the scalar loads and the dependent multiply-add chains.
// The counters: lane i collects candidate 64 j + i of the running group j in one register and adds it to counter register
// j when the group ends -- 16 selects per 64 candidates, every register index a compile-time constant.  (Sixteen unrolled
// copies of the candidate loop, one per counter, spilled 8-22 scalar registers.)
// count <= SBA_RESECT_MAX_TRIALS; counts[count] zeroed by the caller.
template <typename ST>
__global__ __launch_bounds__(256, 2) void resect_score_kernel(Planes pl, unsigned long long n_matches, const double* __restrict__ table,
                                                              int count, double tau2, unsigned long long* __restrict__ counts) {
  __shared__ unsigned int red[4][SBA_RESECT_MAX_TRIALS];
  constexpr int PPT = Lanes<ST>::PPT;
  const size_t n = n_matches, nvec = (n + PPT - 1) / PPT, stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  size_t p = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned int acc[kScoreGroups];
#pragma unroll
  for (int j = 0; j < kScoreGroups; ++j) acc[j] = 0u;
  ResectRegs<ST> cur, nxt;
  if (p < nvec) cur.load(pl, p);
  // whole waves stay in the loop while any of their lanes has a vector: the ballot wants every lane's answer
  while (__ballot(p < nvec) != 0ull) {
    const size_t pn = p + stride;
    if (pn < nvec) nxt.load(pl, pn);
    ResectMatch m[PPT];
    bool valid[PPT];
#pragma unroll
    for (int h = 0; h < PPT; ++h) {
      valid[h] = p < nvec && p * PPT + h < n;
      resect_match(cur, h, valid[h], m[h]);
    }
    ResectParams P, Pn;
    score_candidate(table, 0, P);
    for (int j = 0; 64 * j < count; ++j) {
      const int lim = min(64, count - 64 * j);
      unsigned int group = 0u;      // lane i: candidate 64 j + i at this step
      for (int i = 0; i < lim; ++i) {
        const int k = 64 * j + i;
        score_candidate(table, min(k + 1, count - 1), Pn);
        unsigned int cnt = 0u;
#pragma unroll
        for (int h = 0; h < PPT; ++h) {
          double inv_yy, dstar, c[3], r[3];      // 1 / (y . y) does not depend on the candidate: formed once per match
          resect_residual(P, m[h], inv_yy, dstar, c, r);
          const bool inlier = valid[h] && sq_norm(r[0], r[1], r[2]) <= tau2;     // a NaN is no inlier
          cnt += static_cast<unsigned int>(__popcll(__ballot(inlier)));
        }
        if (lane == i) group += cnt;
#pragma unroll
        for (int q = 0; q < 9; ++q) P.Rn[q] = Pn.Rn[q];
#pragma unroll
        for (int q = 0; q < 3; ++q) P.t[q] = Pn.t[q];
      }
      // into counter register j, the register index a compile-time constant: 16 selects per 64 candidates
#pragma unroll
      for (int g = 0; g < kScoreGroups; ++g) acc[g] += g == j ? group : 0u;
    }
    cur = nxt;
    p = pn;
  }
#pragma unroll
  for (int j = 0; j < kScoreGroups; ++j) red[wave][64 * j + lane] = acc[j];
  __syncthreads();
  for (int k = threadIdx.x; k < count; k += 256) {
    const unsigned long long total = static_cast<unsigned long long>(red[0][k]) + red[1][k] + red[2][k] + red[3][k];
    if (total) atomicAdd(counts + k, total);
  }
}

// resect_moments_kernel with `valid` and-ed with the inlier predicate at P (tau^2 in P.delta2).
template <typename ST>
__global__ __launch_bounds__(256, 1) void resect_inlier_moments_kernel(Planes pl, ResectParams P, double* __restrict__ partials) {
  __shared__ double red[4][SBA_RESECT_MOM_COUNT];
  constexpr int PPT = Lanes<ST>::PPT;
  const size_t n = P.n, nvec = (n + PPT - 1) / PPT, stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  size_t p = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  double acc[SBA_RESECT_MOM_COUNT];
#pragma unroll
  for (int k = 0; k < SBA_RESECT_MOM_COUNT; ++k) acc[k] = 0.0;
  ResectRegs<ST> cur, nxt;
  if (p < nvec) cur.load(pl, p);
  while (p < nvec) {
    const size_t pn = p + stride;
    if (pn < nvec) nxt.load(pl, pn);
#pragma unroll
    for (int h = 0; h < PPT; ++h) {
      const bool valid = p * PPT + h < n;
      ResectMatch m;
      resect_match(cur, h, valid, m);
      double inv_yy, dstar, c[3], r[3];
      resect_residual(P, m, inv_yy, dstar, c, r);
      resect_moments(m, valid && sq_norm(r[0], r[1], r[2]) <= P.delta2, acc);
    }
    cur = nxt;
    p = pn;
  }
  resect_block_fold<SBA_RESECT_MOM_COUNT>(acc, red, partials + static_cast<size_t>(blockIdx.x) * JOINT_ROW);
}

}  // namespace

hipError_t launch_resect_gather(int store, const Planes& pl, const long long* index, int rows, double* out, hipStream_t stream) {
  if (rows <= 0) return hipSuccess;
  const int grid = (rows + 255) / 256;
  if (store == 0) hipLaunchKernelGGL(resect_gather_kernel<double>, dim3(grid), dim3(256), 0, stream, pl, index, rows, out);
  else hipLaunchKernelGGL(resect_gather_kernel<float>, dim3(grid), dim3(256), 0, stream, pl, index, rows, out);
  return hipGetLastError();
}

hipError_t resect_score_blocks_per_cu(int store, int* blocks) {
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks, store == 0 ? reinterpret_cast<const void*>(resect_score_kernel<double>)
                                                                         : reinterpret_cast<const void*>(resect_score_kernel<float>), 256, 0);
}

hipError_t launch_resect_score(int store, const Planes& pl, size_t n, const double* table, int count, double tau2,
                               unsigned long long* counts, int grid, hipStream_t stream) {
  if (count < 1 || count > SBA_RESECT_MAX_TRIALS) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(counts, 0, static_cast<size_t>(count) * sizeof(unsigned long long), stream);
  if (e != hipSuccess || grid <= 0) return e;
  const unsigned long long nn = n;
  if (store == 0) hipLaunchKernelGGL(resect_score_kernel<double>, dim3(grid), dim3(256), 0, stream, pl, nn, table, count, tau2, counts);
  else hipLaunchKernelGGL(resect_score_kernel<float>, dim3(grid), dim3(256), 0, stream, pl, nn, table, count, tau2, counts);
  return hipGetLastError();
}

hipError_t launch_resect_inlier_moments(int store, const Planes& pl, const ResectParams& prm, double* partials, int grid, double* out,
                                        double* host_out, unsigned long long seq, hipStream_t stream) {
  if (grid > 0) {
    if (store == 0) hipLaunchKernelGGL(resect_inlier_moments_kernel<double>, dim3(grid), dim3(256), 0, stream, pl, prm, partials);
    else hipLaunchKernelGGL(resect_inlier_moments_kernel<float>, dim3(grid), dim3(256), 0, stream, pl, prm, partials);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return launch_joint_finalize(partials, grid, SBA_RESECT_MOM_COUNT, -1, out, host_out, seq, stream);
}

}  // namespace sba
