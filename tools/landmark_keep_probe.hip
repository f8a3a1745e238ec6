// Measurement tool (not part of the library): where landmarks_keep_kernel (csrc/sba_landmarks_edit.hip) spends its time.  The
// kernel's loop with its parts switchable at compile time, on n landmarks in the map's plane layout, timed with events:
//   BALLOT    the five class counts: ten ballots and 64-bit adds per step, five integer atomics per wave at the end
//   MASK      the two mask bytes per lane          COUNT   the two u32 counts per lane          STORE   the two keep bytes per lane
//   CLASSIFY  landmark_prune_class (the very function); without it a landmark is kept when X.x + S.xx > 0
//   PREFETCH  the next step's loads are issued before this step's are consumed
//   SPREAD    a wave's five atomics go to one of 64 counter rows 256 bytes apart instead of all waves' to the same five words
//   BLOCKSUM  no atomics: the four waves' counts are added in LDS and each block stores its five sums to a row of its own
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -o landmark_keep_probe tools/landmark_keep_probe.hip     Run: ./landmark_keep_probe [n]
// Prints per variant the mean and minimum of 10 launches and the rate on 78 B per landmark; the variants run in two rounds, the
// second in reverse order.  The grid is the occupancy the runtime reports times the CUs, as the library sizes it.  The class
// counts printed are the first counter row's: all of them only where every wave adds to that row.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../spherical_bundle_adjuster_amd/csrc/sba_landmarks_edit.hpp"

#define CHECK(e)                                                                                        \
  do {                                                                                                  \
    hipError_t err_ = (e);                                                                              \
    if (err_ != hipSuccess) { std::printf("%s: %s\n", #e, hipGetErrorString(err_)); std::exit(1); }      \
  } while (0)

enum { BALLOT = 1, MASK = 2, COUNT = 4, STORE = 8, CLASSIFY = 16, PREFETCH = 32, SPREAD = 64, BLOCKSUM = 128 };
constexpr int kTile = 2048;
constexpr size_t kCounterBytes = 1 << 20;     // room for 64 spread rows and for a row per block

__device__ __forceinline__ double2 nt_load(const double2* ptr) {
  typedef float f4 __attribute__((ext_vector_type(4)));
  const f4 r = __builtin_nontemporal_load(reinterpret_cast<const f4*>(ptr));
  return *reinterpret_cast<const double2*>(&r);
}

struct Step {
  double2 v[9];
  uint2 c;
  unsigned short mb;
};

template <int F>
__device__ __forceinline__ void load_step(Step& s, const double* base, size_t elems, const unsigned char* mask, size_t p) {
#pragma unroll
  for (int k = 0; k < 9; ++k) s.v[k] = nt_load(reinterpret_cast<const double2*>(base + static_cast<size_t>(k) * elems) + p);
  s.c = (F & COUNT) ? reinterpret_cast<const uint2*>(base + 9 * elems)[p] : make_uint2(1u, 1u);
  s.mb = (F & MASK) ? reinterpret_cast<const unsigned short*>(mask)[p] : static_cast<unsigned short>(0x0101u);
}

template <int F>
__global__ __launch_bounds__(256) void keep_variant(const double* __restrict__ base, unsigned long long elems, unsigned long long n,
                                                    double max_score, unsigned int min_count, const unsigned char* __restrict__ mask,
                                                    unsigned char* __restrict__ keep, unsigned long long tile_pairs,
                                                    unsigned long long* __restrict__ counters) {
  const size_t nvec = elems / 2, stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  unsigned long long cc[5] = {0, 0, 0, 0, 0};
  unsigned sink = 0;
  size_t p = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  Step cur, nxt;
  if ((F & PREFETCH) && p < nvec) load_step<F>(cur, base, elems, mask, p);
  for (; p < tile_pairs; p += stride) {
    int cls[2] = {0, 0};
    const bool valid[2] = {2 * p < n, 2 * p + 1 < n};
    if (F & PREFETCH) {
      if (p + stride < nvec) load_step<F>(nxt, base, elems, mask, p + stride);
    } else if (p < nvec) {
      load_step<F>(cur, base, elems, mask, p);
    }
    if (p < nvec) {
      const double2* v = cur.v;
      const double X0[3] = {v[0].x, v[1].x, v[2].x}, X1[3] = {v[0].y, v[1].y, v[2].y};
      const double S0[6] = {v[3].x, v[4].x, v[5].x, v[6].x, v[7].x, v[8].x}, S1[6] = {v[3].y, v[4].y, v[5].y, v[6].y, v[7].y, v[8].y};
      if (F & CLASSIFY) {
        cls[0] = sba::landmark_prune_class(X0, S0, cur.c.x, static_cast<unsigned char>(cur.mb & 0xffu), max_score, min_count);
        cls[1] = sba::landmark_prune_class(X1, S1, cur.c.y, static_cast<unsigned char>(cur.mb >> 8), max_score, min_count);
      } else {
        double a = 0.0, b = 0.0;
#pragma unroll
        for (int k = 0; k < 9; ++k) { a += v[k].x; b += v[k].y; }
        cls[0] = a + cur.c.x + (cur.mb & 0xffu) > 0.0 ? sba::LANDMARK_KEPT : sba::LANDMARK_MASKED;
        cls[1] = b + cur.c.y + (cur.mb >> 8) > 0.0 ? sba::LANDMARK_KEPT : sba::LANDMARK_MASKED;
      }
    }
    const unsigned k0 = valid[0] && cls[0] == sba::LANDMARK_KEPT ? 1u : 0u, k1 = valid[1] && cls[1] == sba::LANDMARK_KEPT ? 1u : 0u;
    if (F & STORE) reinterpret_cast<unsigned short*>(keep)[p] = static_cast<unsigned short>(k0 | (k1 << 8));
    else sink += k0 + k1;
    if (F & BALLOT) {
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int k = 0; k < 5; ++k) cc[k] += __popcll(__ballot(valid[h] && cls[h] == k));
    }
    if (F & PREFETCH) cur = nxt;
  }
  if (F & BLOCKSUM) {
    __shared__ unsigned long long wave_cc[4][5];
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
      for (int k = 0; k < 5; ++k) wave_cc[threadIdx.x >> 6][k] = cc[k];
    }
    __syncthreads();
    if (threadIdx.x < 5) counters[static_cast<size_t>(blockIdx.x) * 8 + threadIdx.x] =
        wave_cc[0][threadIdx.x] + wave_cc[1][threadIdx.x] + wave_cc[2][threadIdx.x] + wave_cc[3][threadIdx.x];
  } else if ((F & BALLOT) && (threadIdx.x & 63) == 0) {
    unsigned long long* row = (F & SPREAD) ? counters + static_cast<size_t>((blockIdx.x * 4 + (threadIdx.x >> 6)) & 63u) * 32 : counters;
#pragma unroll
    for (int k = 0; k < 5; ++k)
      if (cc[k] != 0) atomicAdd(row + k, cc[k]);
  }
  if (!(F & STORE) && sink == 0xffffffffu) keep[0] = 1;      // never true: keeps the loads alive
}

__global__ void fill_kernel(double* base, size_t elems, unsigned char* mask) {
  const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
  for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < elems; i += stride) {
    const unsigned h = static_cast<unsigned>(i) * 2654435761u;
    const double u = (h >> 8) * (1.0 / 16777216.0);
    base[i] = 1.0 + u; base[elems + i] = -2.0 + u; base[2 * elems + i] = 4.0 - u;
    base[3 * elems + i] = 0.01 + 0.02 * u; base[4 * elems + i] = 0.02; base[5 * elems + i] = 0.03 - 0.01 * u;
    base[6 * elems + i] = 1e-3; base[7 * elems + i] = -2e-3; base[8 * elems + i] = 5e-4;
    reinterpret_cast<unsigned int*>(base + 9 * elems)[i] = h >> 30;
    mask[i] = (h >> 13) & 1u;
  }
}

struct Variant {
  const char* name;
  int flags;
  const void* fn;
};

template <int F>
Variant variant(const char* name) { return Variant{name, F, reinterpret_cast<const void*>(keep_variant<F>)}; }

int main(int argc, char** argv) {
  const size_t n = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 10000000, elems = (n + 1) / 2 * 2;
  const size_t ntiles = (n + kTile - 1) / kTile, tile_bytes = ntiles * kTile;
  double* base = nullptr;
  unsigned char *mask = nullptr, *keep = nullptr;
  unsigned long long* counters = nullptr;
  CHECK(hipMalloc(reinterpret_cast<void**>(&base), 9 * elems * sizeof(double) + elems * sizeof(unsigned int) + 16));
  CHECK(hipMalloc(reinterpret_cast<void**>(&mask), tile_bytes));
  CHECK(hipMalloc(reinterpret_cast<void**>(&keep), tile_bytes));
  CHECK(hipMalloc(reinterpret_cast<void**>(&counters), kCounterBytes));
  CHECK(hipMemset(mask, 0, tile_bytes));
  hipLaunchKernelGGL(fill_kernel, dim3(4096), dim3(256), 0, 0, base, elems, mask);
  CHECK(hipDeviceSynchronize());
  hipDeviceProp_t prop;
  CHECK(hipGetDeviceProperties(&prop, 0));
  constexpr int ALL = BALLOT | MASK | COUNT | STORE | CLASSIFY;
  const std::vector<Variant> variants = {
      variant<ALL>("as the library's"), variant<ALL & ~BALLOT>("no ballots"), variant<ALL & ~MASK>("no mask bytes"),
      variant<ALL & ~COUNT>("no counts"), variant<ALL & ~STORE>("no keep store"), variant<ALL & ~CLASSIFY>("no classification"),
      variant<0>("the nine plane loads alone"), variant<STORE>("plane loads + keep store"), variant<ALL | PREFETCH>("all, next step's loads in flight"),
      variant<(ALL & ~BALLOT) | PREFETCH>("no ballots, next step's loads in flight"), variant<ALL | SPREAD>("all, atomics spread over 64 rows"),
      variant<ALL | BLOCKSUM>("all, block sums stored, no atomics")};
  std::vector<std::vector<float>> ms(variants.size());
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  const double max_score = 0.004;      // about half of the scores lie above it
  for (int round = 0; round < 2; ++round)
    for (size_t q = 0; q < variants.size(); ++q) {
      const size_t k = round == 0 ? q : variants.size() - 1 - q;
      int occ = 1;
      CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, variants[k].fn, 256, 0));
      const size_t pairs = tile_bytes / 2;
      const unsigned grid = static_cast<unsigned>(std::min<size_t>((pairs + 255) / 256, static_cast<size_t>(prop.multiProcessorCount) * std::max(1, occ)));
      unsigned long long elems_ = elems, n_ = n, pairs_ = pairs;
      unsigned int min_count = 1;
      double ms_ = max_score;
      void* args[] = {&base, &elems_, &n_, &ms_, &min_count, &mask, &keep, &pairs_, &counters};
      for (int it = 0; it < 6; ++it) {
        CHECK(hipMemsetAsync(counters, 0, kCounterBytes, 0));
        CHECK(hipEventRecord(e0, 0));
        CHECK(hipLaunchKernel(variants[k].fn, dim3(grid), dim3(256), args, 0, 0));
        CHECK(hipEventRecord(e1, 0));
        CHECK(hipEventSynchronize(e1));
        float t = 0.f;
        CHECK(hipEventElapsedTime(&t, e0, e1));
        if (it > 0) ms[k].push_back(t);
      }
      if (round == 0) {
        unsigned long long c[5];
        CHECK(hipMemcpy(c, counters, sizeof(c), hipMemcpyDeviceToHost));
        std::printf("%-42s occupancy %2d, grid %5u, classes %llu %llu %llu %llu %llu\n", variants[k].name, occ, grid, c[0], c[1], c[2], c[3], c[4]);
      }
    }
  std::printf("n = %zu; 78 B per landmark; 8 TB/s = 1.00\n%-42s %9s %9s %10s\n", n, "variant", "mean us", "min us", "of 8 TB/s");
  for (size_t k = 0; k < variants.size(); ++k) {
    double sum = 0.0, lo = 1e30;
    for (float t : ms[k]) { sum += t; lo = std::min<double>(lo, t); }
    const double mean = sum / ms[k].size();
    std::printf("%-42s %9.1f %9.1f %10.2f\n", variants[k].name, 1e3 * mean, 1e3 * lo, 78.0 * n / (mean * 1e-3) / 8e12);
  }
  return 0;
}
