// Device-only helpers of the landmark map's kernels: included by sba_landmarks.hip, sba_landmarks_edit.hip and
// sba_landmarks_register.hip and by nothing else (the HIP-free sba_landmarks*.hpp headers stay HIP-free).  One copy of
//   load_nt, plane, counts      the non-temporal 16-byte load and the accessors of the nine f64 planes and the u32 count plane
//   ClassCounts<CLASSES>        wave-uniform class counts: a ballot and a population count per class and step, one integer atomic
//                               per wave and class at the end, to one row of counters or to one of kLandmarkCounterRows rows
//   PairRegs<NOISE>             one 16-byte vector (two landmarks) of everything a dense pass reads, split per landmark
//   gather, scatter             one landmark of the indexed form
// Everything is forceinline and small.  The body that landmarks_fuse_kernel and landmarks_register_apply_kernel share is not
// here: it is sba_landmarks_pass.inc, which both kernels expand in their own bodies over these helpers.  The caller rows
// [n][3] + [n][6] -> v[2][9] of landmarks_pack_kernel and landmarks_append_kernel are not here either: read through a shared
// function the append kernel issued its loads in another order and measured slower, so each kernel keeps its own.
#pragma once
#include "sba_device.hpp"

namespace sba {
namespace lm {

__device__ __forceinline__ double2 load_nt(const double2* ptr) {
  typedef float f4 __attribute__((ext_vector_type(4)));
  const f4 r = __builtin_nontemporal_load(reinterpret_cast<const f4*>(ptr));
  return *reinterpret_cast<const double2*>(&r);
}

__device__ __forceinline__ double2* plane(double* base, unsigned long long elems, int k) {
  return reinterpret_cast<double2*>(base + static_cast<size_t>(k) * elems);
}
__device__ __forceinline__ const double2* plane(const double* base, unsigned long long elems, int k) {
  return reinterpret_cast<const double2*>(base + static_cast<size_t>(k) * elems);
}
__device__ __forceinline__ unsigned int* counts(double* base, unsigned long long elems) {
  return reinterpret_cast<unsigned int*>(base + 9 * static_cast<size_t>(elems));
}
__device__ __forceinline__ const unsigned int* counts(const double* base, unsigned long long elems) {
  return reinterpret_cast<const unsigned int*>(base + 9 * static_cast<size_t>(elems));
}

// Wave-uniform class counts: every active lane adds the same population counts.  Lanes of a wave hold consecutive items, so
// lane 0 took part in every step any lane of its wave took part in, and it alone flushes.
template <int CLASSES>
struct ClassCounts {
  unsigned long long c[CLASSES];
  __device__ __forceinline__ void init() {
#pragma unroll
    for (int k = 0; k < CLASSES; ++k) c[k] = 0;
  }
  __device__ __forceinline__ void add(bool valid, int cls) {
#pragma unroll
    for (int k = 0; k < CLASSES; ++k) c[k] += __popcll(__ballot(valid && cls == k));
  }
  __device__ __forceinline__ void flush(unsigned long long* __restrict__ counters) const {
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
      for (int k = 0; k < CLASSES; ++k)
        if (c[k] != 0) atomicAdd(counters + k, c[k]);
    }
  }
  // One of kLandmarkCounterRows rows per wave, which the host sums: all waves on the same words serialise.
  __device__ __forceinline__ void flush_rows(unsigned long long* __restrict__ counters) const {
    if ((threadIdx.x & 63) == 0) {
      unsigned long long* row = counters + static_cast<size_t>((blockIdx.x * 4u + (threadIdx.x >> 6)) % kLandmarkCounterRows) * kLandmarkCounterStride;
#pragma unroll
      for (int k = 0; k < CLASSES; ++k)
        if (c[k] != 0) atomicAdd(row + k, c[k]);
    }
  }
};

// One 16-byte vector (landmarks 2 p and 2 p + 1) of everything a dense pass reads: nine planes, 48 bytes of bearing rows, the
// noise.  h = 0 / 1: the first / second landmark of the lane.
template <bool NOISE>
struct PairRegs {
  double2 v[9], yv[3], nz;
  __device__ __forceinline__ void load_planes(const double* base, unsigned long long elems, size_t p) {
#pragma unroll
    for (int k = 0; k < 9; ++k) v[k] = load_nt(plane(base, elems, k) + p);
  }
  __device__ __forceinline__ void load(const double* base, unsigned long long elems, const double* bearings, const double* noise, size_t p) {
    load_planes(base, elems, p);
#pragma unroll
    for (int k = 0; k < 3; ++k) yv[k] = load_nt(reinterpret_cast<const double2*>(bearings) + 3 * p + k);
    if (NOISE) nz = load_nt(reinterpret_cast<const double2*>(noise) + p);
  }
  __device__ __forceinline__ void landmark(int h, double X[3], double Sg[6]) const {
#pragma unroll
    for (int k = 0; k < 3; ++k) X[k] = h == 0 ? v[k].x : v[k].y;
#pragma unroll
    for (int k = 0; k < 6; ++k) Sg[k] = h == 0 ? v[3 + k].x : v[3 + k].y;
  }
  __device__ __forceinline__ void get(int h, double X[3], double Sg[6], double y[3]) const {
    landmark(h, X, Sg);
    y[0] = h == 0 ? yv[0].x : yv[1].y;
    y[1] = h == 0 ? yv[0].y : yv[2].x;
    y[2] = h == 0 ? yv[1].x : yv[2].y;
  }
  __device__ __forceinline__ double noise(int h) const { return h == 0 ? nz.x : nz.y; }
  __device__ __forceinline__ void set(int h, const double Xo[3], const double So[6]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { if (h == 0) v[k].x = Xo[k]; else v[k].y = Xo[k]; }
#pragma unroll
    for (int k = 0; k < 6; ++k) { if (h == 0) v[3 + k].x = So[k]; else v[3 + k].y = So[k]; }
  }
  __device__ __forceinline__ void store(double* base, unsigned long long elems, size_t p) const {
#pragma unroll
    for (int k = 0; k < 9; ++k) plane(base, elems, k)[p] = v[k];
  }
};

// Observation j of the indexed form: landmark i = idx[j] gathered from the planes, bearing row j.
__device__ __forceinline__ void gather(const double* base, unsigned long long elems, size_t i, const double* bearings, size_t j, double X[3],
                                       double Sg[6], double y[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) { X[k] = base[static_cast<size_t>(k) * elems + i]; y[k] = bearings[3 * j + k]; }
#pragma unroll
  for (int k = 0; k < 6; ++k) Sg[k] = base[static_cast<size_t>(3 + k) * elems + i];
}
__device__ __forceinline__ void scatter(double* base, unsigned long long elems, size_t i, const double Xo[3], const double So[6]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) base[static_cast<size_t>(k) * elems + i] = Xo[k];
#pragma unroll
  for (int k = 0; k < 6; ++k) base[static_cast<size_t>(3 + k) * elems + i] = So[k];
}

}  // namespace lm
}  // namespace sba
