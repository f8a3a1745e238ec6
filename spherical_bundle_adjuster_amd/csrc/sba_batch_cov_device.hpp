// Device helpers the batched covariance kernel (sba_batch_covariance.hip) and the batched structure kernel
// (sba_batch_structure.hip) share: a pair's pass parameters built on the device from its record, their way from LDS into scalar
// registers, and the store of a lane's two 24-byte rows into a caller-ordered array.  Device code only.
#pragma once
#include <cfloat>

#include "sba_covariance.hpp"
#include "sba_device.hpp"
#include "sba_joint_core.hpp"

namespace sba {

// A block-uniform value (read from LDS) as a scalar: the pass parameters then occupy scalar registers, as the kernel
// arguments of the single-problem kernels do, instead of ~50 vector registers of every lane.
__device__ __forceinline__ double uniform_f64(double v) {
  const unsigned long long q = static_cast<unsigned long long>(__double_as_longlong(v));
  const unsigned lo = __builtin_amdgcn_readfirstlane(static_cast<unsigned>(q));
  const unsigned hi = __builtin_amdgcn_readfirstlane(static_cast<unsigned>(q >> 32));
  return __longlong_as_double(static_cast<long long>((static_cast<unsigned long long>(hi) << 32) | lo));
}

// The JointParams of the covariance at (rot, tran): a first reduce pass of the undamped problem -- the device-side twin of
// what sba_problem_covariance_joint builds on the host.  Thread 0 only.
__device__ __forceinline__ void cov_fill_params(const double rot[3], const double tran[3], unsigned long long n,
                                                const sba_lm_options& o, JointParams* P) {
  fill_sweep_params(n, SBA_DEPTH_PER_MATCH, rot, tran, 1.0, 1.0, o.huber_delta, &P->cur, false);
  double B[9];
  factored_frame(rot, B, P->J);
  P->small_angle = !(rot[0] * rot[0] + rot[1] * rot[1] + rot[2] * rot[2] > DBL_EPSILON) ? 1 : 0;
#pragma unroll
  for (int k = 0; k < 6; ++k) P->delta_c[k] = 0.0;
  P->inv_radius = 0.0;                // radius = inf: the undamped system
  P->min_diagonal = o.min_lm_diagonal; P->max_diagonal = o.max_lm_diagonal;
  P->first = 1;
  P->jacobi_scaling = o.jacobi_scaling ? 1 : 0;
  P->pad_ = 0;
}

// What the two loops read of the parameters, LDS -> scalar registers (a first pass reads nothing of the candidate camera).
__device__ __forceinline__ void cov_take_params(const JointParams& s, JointParams& P) {
#pragma unroll
  for (int k = 0; k < 9; ++k) { P.cur.Rn[k] = uniform_f64(s.cur.Rn[k]); P.J[k] = uniform_f64(s.J[k]); }
#pragma unroll
  for (int k = 0; k < 3; ++k) P.cur.t[k] = uniform_f64(s.cur.t[k]);
  P.cur.d2 = uniform_f64(s.cur.d2); P.cur.delta = uniform_f64(s.cur.delta); P.cur.delta2 = uniform_f64(s.cur.delta2);
  P.inv_radius = 0.0; P.min_diagonal = uniform_f64(s.min_diagonal); P.max_diagonal = uniform_f64(s.max_diagonal);
  P.small_angle = __builtin_amdgcn_readfirstlane(s.small_angle);
  P.first = 1;
  P.jacobi_scaling = __builtin_amdgcn_readfirstlane(s.jacobi_scaling);
  P.pad_ = 0;
}

// A lane's two rows into out[row0 + 2 pr][3]: 48 contiguous bytes at byte offset 24 (row0 + 2 pr), 16-byte aligned only when
// the pair's first row is even -- an odd first row shifts the 16-byte stores by one double.  The last match of an odd-sized
// pair writes its own three doubles and nothing of the padding match: the next row belongs to the next pair.
struct CovStoreRows {
  double* out;
  size_t row0, n;
  __device__ __forceinline__ void operator()(size_t pr, const double (&o)[2][3]) const {
    double* p = out + 3 * (row0 + 2 * pr);
    const bool two = 2 * pr + 1 < n;
    if ((row0 & 1) == 0) {
      *reinterpret_cast<double2*>(p) = make_double2(o[0][0], o[0][1]);
      if (two) {
        *reinterpret_cast<double2*>(p + 2) = make_double2(o[0][2], o[1][0]);
        *reinterpret_cast<double2*>(p + 4) = make_double2(o[1][1], o[1][2]);
      } else {
        p[2] = o[0][2];
      }
    } else {
      p[0] = o[0][0];
      *reinterpret_cast<double2*>(p + 1) = make_double2(o[0][1], o[0][2]);
      if (two) {
        *reinterpret_cast<double2*>(p + 3) = make_double2(o[1][0], o[1][1]);
        p[5] = o[1][2];
      }
    }
  }
};

}  // namespace sba
