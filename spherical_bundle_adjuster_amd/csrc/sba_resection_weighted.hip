// The resection weighted by the landmarks' covariances, on the device (algebra: sba_resection_weighted.hpp, per-match code:
// sba_resection_weighted_core.hpp on top of sba_resection_core.hpp).  The weights are frozen at a reference pose, so one
// evaluation stays ONE streaming reduction:
//   resect_weights_kernel      Sigma rows + the seven planes at the reference pose -> the three planes of the factored weight;
//                              counts the matches of zero weight (ballot + population count, integer atomic); once per freeze
//   resect_wreduce_kernel      the seven planes + the three weight planes -> the 31 sums of the SBA_RESECT_* row
//   resect_weight_rows_kernel  the stored factor expanded to M_i rows; no reduction (inspection, tests)
// All: 256-thread blocks, grid-stride over 16-byte vectors (2 matches per lane with f64 planes, 4 with f32), non-temporal
// loads, plain 16-byte stores.  The reduce pass keeps the next step's vectors in registers; its fold, finalize and mapped row
// are those of the unweighted pass.  No floating-point atomics: bit-identical run to run for a fixed grid, and the two passes
// without a reduction do not depend on the grid at all.
// Bytes per match (f64 planes): the freeze reads 56 + 48 and writes 24; the reduce pass reads 56 + 24 = 80, never Sigma.
#include "sba_device.hpp"
#include "sba_resection_weighted_core.hpp"

namespace sba {
namespace {

template <typename ST>
__global__ __launch_bounds__(256) void resect_weights_kernel(Planes pl, ResectWeightParams W, const double* __restrict__ sigma,
                                                             double* __restrict__ q0, double* __restrict__ q1, double* __restrict__ q2,
                                                             unsigned long long* __restrict__ n_zero) {
  constexpr int PPT = Lanes<ST>::PPT;
  const size_t n = W.P.n, nvec = (n + PPT - 1) / PPT, stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  unsigned long long zeros = 0;      // wave-uniform: every active lane adds the same population count
  for (size_t p = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; p < nvec; p += stride) {
    ResectRegs<ST> cur;
    cur.load(pl, p);
    double2 sg[PPT][3];
#pragma unroll
    for (int h = 0; h < PPT; ++h)
#pragma unroll
      for (int k = 0; k < 3; ++k)
        sg[h][k] = VecRegs<ST, DEPTH_PER_MATCH>::stream_load(reinterpret_cast<const double2*>(sigma) + (p * PPT + h) * 3 + k);
    double out[3][PPT];
#pragma unroll
    for (int h = 0; h < PPT; ++h) {
      const bool valid = p * PPT + h < n;
      ResectMatch m;
      resect_match(cur, h, valid, m);
      const double row[6] = {sg[h][0].x, sg[h][0].y, sg[h][1].x, sg[h][1].y, sg[h][2].x, sg[h][2].y};
      double q[3];
      const bool ok = resect_weight_freeze(W, m, row, valid, q);
      zeros += __popcll(__ballot(valid && !ok));
      out[0][h] = q[0]; out[1][h] = q[1]; out[2][h] = q[2];
    }
#pragma unroll
    for (int h = 0; h < PPT / 2; ++h) {
      reinterpret_cast<double2*>(q0)[p * (PPT / 2) + h] = make_double2(out[0][2 * h], out[0][2 * h + 1]);
      reinterpret_cast<double2*>(q1)[p * (PPT / 2) + h] = make_double2(out[1][2 * h], out[1][2 * h + 1]);
      reinterpret_cast<double2*>(q2)[p * (PPT / 2) + h] = make_double2(out[2][2 * h], out[2][2 * h + 1]);
    }
  }
  // Lanes of a wave hold consecutive vectors, so lane 0 took part in every step any lane of its wave took part in.
  if ((threadIdx.x & 63) == 0 && zeros != 0) atomicAdd(n_zero, zeros);
}

// f64 planes: two resident blocks per CU like the unweighted pass (62 accumulator registers, a double buffer of 2 x 40 and
// a match's temporaries).  f32 planes: the double buffer is 2 x 56 registers -- ONE block per CU rather than a spill.
template <typename ST, bool LOSS>
__global__ __launch_bounds__(256, (Lanes<ST>::PPT == 2 ? 2 : 1)) void resect_wreduce_kernel(Planes pl, ResectWeightPlanes wp, ResectParams P,
                                                                                           double* __restrict__ partials) {
  __shared__ double red[4][SBA_RESECT_COUNT];
  constexpr int PPT = Lanes<ST>::PPT;
  const size_t n = P.n, nvec = (n + PPT - 1) / PPT, stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  size_t p = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  double acc[SBA_RESECT_COUNT];
#pragma unroll
  for (int k = 0; k < SBA_RESECT_COUNT; ++k) acc[k] = 0.0;
  ResectRegs<ST> cur, nxt;
  ResectWeightRegs<ST> wcur, wnxt;
  if (p < nvec) { cur.load(pl, p); wcur.load(wp, p); }
  while (p < nvec) {
    const size_t pn = p + stride;
    if (pn < nvec) { nxt.load(pl, pn); wnxt.load(wp, pn); }
#pragma unroll
    for (int h = 0; h < PPT; ++h) {
      const double q[3] = {wcur.get(0, h), wcur.get(1, h), wcur.get(2, h)};
      const bool live = p * PPT + h < n && q[0] != 0.0;
      ResectMatch m;
      resect_match(cur, h, live, m);
      resect_waccumulate<LOSS>(P, m, q, live, acc);
      __builtin_amdgcn_sched_barrier(0);     // one match at a time, as in resect_reduce_kernel
    }
    cur = nxt;
    wcur = wnxt;
    p = pn;
  }
  resect_block_fold<SBA_RESECT_COUNT>(acc, red, partials + static_cast<size_t>(blockIdx.x) * JOINT_ROW);
}

template <typename ST>
__global__ __launch_bounds__(256) void resect_weight_rows_kernel(Planes pl, ResectWeightPlanes wp, unsigned long long n_matches,
                                                                 double* __restrict__ out) {
  constexpr int PPT = Lanes<ST>::PPT;
  typedef typename Lanes<ST>::vec vec;
  const size_t n = n_matches, nvec = (n + PPT - 1) / PPT, stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (size_t p = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; p < nvec; p += stride) {
    vec yv[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) yv[k] = VecRegs<ST, DEPTH_PER_MATCH>::stream_load(reinterpret_cast<const vec*>(pl.x2[k]) + p);
    ResectWeightRegs<ST> w;
    w.load(wp, p);
#pragma unroll
    for (int h = 0; h < PPT; ++h) {
      const bool valid = p * PPT + h < n;
      double y[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const ST* e = reinterpret_cast<const ST*>(&yv[k]);
        y[k] = valid ? static_cast<double>(e[h]) : 0.0;
      }
      const double q[3] = {valid ? w.get(0, h) : 0.0, valid ? w.get(1, h) : 0.0, valid ? w.get(2, h) : 0.0};
      double M[6];
      resect_weight_expand(q, y, M);
      const bool live = valid && q[0] != 0.0;
      double2* o = reinterpret_cast<double2*>(out) + (p * PPT + h) * 3;
      o[0] = live ? make_double2(M[0], M[1]) : make_double2(0.0, 0.0);
      o[1] = live ? make_double2(M[2], M[3]) : make_double2(0.0, 0.0);
      o[2] = live ? make_double2(M[4], M[5]) : make_double2(0.0, 0.0);
    }
  }
}

template <typename ST>
const void* wreduce_kernel_of(bool loss) {
  return loss ? reinterpret_cast<const void*>(resect_wreduce_kernel<ST, true>) : reinterpret_cast<const void*>(resect_wreduce_kernel<ST, false>);
}

}  // namespace

hipError_t resect_wreduce_blocks_per_cu(int store, bool loss, int* blocks) {
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks, store == 0 ? wreduce_kernel_of<double>(loss) : wreduce_kernel_of<float>(loss), 256, 0);
}

hipError_t launch_resect_weights(int store, const Planes& pl, const ResectWeightParams& prm, const double* sigma, double* const q[3],
                                 unsigned long long* n_zero, int grid, hipStream_t stream) {
  hipError_t e = hipMemsetAsync(n_zero, 0, sizeof(unsigned long long), stream);
  if (e != hipSuccess || grid <= 0) return e;
  if (store == 0) hipLaunchKernelGGL(resect_weights_kernel<double>, dim3(grid), dim3(256), 0, stream, pl, prm, sigma, q[0], q[1], q[2], n_zero);
  else hipLaunchKernelGGL(resect_weights_kernel<float>, dim3(grid), dim3(256), 0, stream, pl, prm, sigma, q[0], q[1], q[2], n_zero);
  return hipGetLastError();
}

hipError_t launch_resect_wreduce(int store, const Planes& pl, const ResectWeightPlanes& wp, const ResectParams& prm, double* partials,
                                 int grid, double* out, double* host_out, unsigned long long seq, hipStream_t stream) {
  if (grid > 0) {
    const bool loss = prm.delta > 0.0;
    if (store == 0 && loss) hipLaunchKernelGGL((resect_wreduce_kernel<double, true>), dim3(grid), dim3(256), 0, stream, pl, wp, prm, partials);
    else if (store == 0) hipLaunchKernelGGL((resect_wreduce_kernel<double, false>), dim3(grid), dim3(256), 0, stream, pl, wp, prm, partials);
    else if (loss) hipLaunchKernelGGL((resect_wreduce_kernel<float, true>), dim3(grid), dim3(256), 0, stream, pl, wp, prm, partials);
    else hipLaunchKernelGGL((resect_wreduce_kernel<float, false>), dim3(grid), dim3(256), 0, stream, pl, wp, prm, partials);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return launch_joint_finalize(partials, grid, SBA_RESECT_COUNT, -1, out, host_out, seq, stream);
}

hipError_t launch_resect_weight_rows(int store, const Planes& pl, const ResectWeightPlanes& wp, size_t n, double* out, int grid,
                                     hipStream_t stream) {
  if (grid <= 0) return hipSuccess;
  const unsigned long long nn = n;
  if (store == 0) hipLaunchKernelGGL(resect_weight_rows_kernel<double>, dim3(grid), dim3(256), 0, stream, pl, wp, nn, out);
  else hipLaunchKernelGGL(resect_weight_rows_kernel<float>, dim3(grid), dim3(256), 0, stream, pl, wp, nn, out);
  return hipGetLastError();
}

}  // namespace sba
