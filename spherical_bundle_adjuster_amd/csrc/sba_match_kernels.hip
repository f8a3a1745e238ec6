// Exact L2 2-nearest-neighbour matching of f32 descriptors with the reference's ratio test (feature_matcher.cpp:42-59;
// entry points in sba_match.cpp).
//
// match_pack_kernel copies the caller's strided rows into [row][dp] f32 (dp = 64 / 128 / 256, zero beyond dim): queries
// scaled by -2 (exact), train rows with their squared norm (NaN for a non-finite row: such a row never ranks).  Every pair
// starts on a whole block of queries and a whole 32-row tile of train rows, the padding rows of a tile carry a NaN norm.
//
// match_tiles_kernel: one block = one query block of one pair against one split of its train tiles.  Each wave holds QT
// tiles of 32 queries as the B operand of v_mfma_f32_32x32x2_f32 in registers; the block stages 32 train rows at a time in
// LDS (double buffered, the next tile prefetched into registers) as the A operand.  With the train tile as A and the query
// tile as B, lane l's 16 accumulators are the scores of ONE query (column l & 31) against 16 train rows
// (8 (reg >> 2) + 4 (l >> 5) + (reg & 3)), so the top-2 update runs in registers and only the two half-waves merge at the
// end.  Lane half h feeds the k range [h dp / 2, (h + 1) dp / 2), four k per 16-byte LDS read; A and B use the same k
// order, so the product is still a fixed fmaf chain of one query and one train row.  The accumulators start at the train
// row's squared norm: score = fl(|t|^2 + sum_k (-2 q_k) t_k), which ranks like |q - t|^2.  Within a lane the train rows
// arrive in increasing index order, so a strict `<` keeps the lowest index of equal scores; every later merge compares
// (score, index) lexicographically, which makes the top-2 of a query independent of the split and of the other queries.
//
// match_finish_kernel merges a query's per-split lists, rescores the two winners from the caller's rows as
// sum_k (q_k - t_k)^2 (an f32 fmaf chain in k order), orders them by (rescored, index), reports sqrt -- DMatch::distance --
// and applies the reference's float test d0 < ratio * d1.  match_scatter_kernel then writes the accepted queries in
// ascending order with the tile count / scan of sba_select.hip (ballot + mbcnt ranks, no atomics on positions).
//
// Not tuned: match_pack_kernel and match_finish_kernel run one thread per descriptor row, so their global reads are
// strided by a whole row (uncoalesced).  At one pair of 50 k rows they cost about an eighth of the product kernel, at 256
// pairs of 8 k about 0.9 x (a wave per group of rows is the next step).
#include <algorithm>

#include "sba_device.hpp"
#include "sba_match.hpp"

namespace sba {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// (s, i) ranks before (bs, bi): lexicographic on (score, index); index -1 is an empty slot.
__device__ __forceinline__ bool ranks_before(float s, int i, float bs, int bi) {
  return i >= 0 && (bi < 0 || s < bs || (s == bs && i < bi));
}
__device__ __forceinline__ void insert_top2(float s, int i, float& b0, int& i0, float& b1, int& i1) {
  // selects, not branches: a branchy form lets the compiler merge the stores into one through a selected address, which
  // puts the four values in scratch
  const bool c0 = ranks_before(s, i, b0, i0), c1 = ranks_before(s, i, b1, i1);
  const float nb1 = c0 ? b0 : (c1 ? s : b1);
  const int ni1 = c0 ? i0 : (c1 ? i : i1);
  b0 = c0 ? s : b0;
  i0 = c0 ? i : i0;
  b1 = nb1;
  i1 = ni1;
}

__global__ __launch_bounds__(256) void match_pack_kernel(const uint8_t* __restrict__ src, size_t stride, int dim, int dp,
                                                         const MatchPair* __restrict__ pairs, int num_pairs,
                                                         const unsigned long long* __restrict__ off_rel, size_t total, int side,
                                                         float* __restrict__ pack, float* __restrict__ norm) {
  const size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= total) return;
  const int g = batch_pair_of(i, off_rel, num_pairs);
  const size_t local = i - off_rel[g];
  const MatchPair P = pairs[g];
  const float* r = reinterpret_cast<const float*>(src + (static_cast<size_t>(side == 0 ? P.q_row0 : P.t_row0) + local) * stride);
  float* out = pack + (static_cast<size_t>(side == 0 ? P.q_pack : P.t_pack) + local) * dp;
  float acc = 0.f;
  bool finite = true;
  for (int k = 0; k < dim; ++k) {
    const float v = r[k];
    finite = finite && isfinite(v);
    acc = fmaf(v, v, acc);
    out[k] = side == 0 ? -2.f * v : v;
  }
  if (side == 1) norm[P.t_pack + local] = finite ? acc : __int_as_float(0x7fc00000);
}

template <int DP, int QT>
__global__ __launch_bounds__(kMatchBlock) void match_tiles_kernel(const float* __restrict__ qpack, const float* __restrict__ tpack,
                                                                  const float* __restrict__ tnorm,
                                                                  const MatchPair* __restrict__ pairs,
                                                                  const MatchItem* __restrict__ items, int splits,
                                                                  float4* __restrict__ part) {
  constexpr int HALF = DP / 2;                                 // k per lane half
  constexpr int LDS_ROW = DP + 4;                              // floats per staged row: 16 B of skew against bank conflicts
  constexpr int CHUNKS = kMatchTile * DP / 4 / kMatchBlock;    // 16-byte pieces of a train tile per thread
  static_assert(CHUNKS >= 1, "a train tile covers the block");
  __shared__ __attribute__((aligned(16))) float s_tile[2][kMatchTile * LDS_ROW];
  __shared__ __attribute__((aligned(16))) float s_norm[2][kMatchTile];
  const MatchItem it = items[blockIdx.x];
  const MatchPair P = pairs[it.pair];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, h = lane >> 5;

  f32x4 qb[QT][HALF / 4];
  size_t prow[QT];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    prow[qt] = P.q_pack + static_cast<size_t>(it.qblock) * (4 * 32 * QT) + (wave * QT + qt) * 32 + j;
    const f32x4* src = reinterpret_cast<const f32x4*>(qpack + prow[qt] * DP + h * HALF);
#pragma unroll
    for (int m = 0; m < HALF / 4; ++m) qb[qt][m] = src[m];
  }
  const unsigned t_begin = static_cast<unsigned>(static_cast<unsigned long long>(it.split) * P.t_tiles / splits);
  const unsigned t_end = static_cast<unsigned>(static_cast<unsigned long long>(it.split + 1) * P.t_tiles / splits);

  float b0[QT], b1[QT];
  int i0[QT], i1[QT];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) { b0[qt] = b1[qt] = __int_as_float(0x7f800000); i0[qt] = i1[qt] = -1; }

  f32x4 pre[CHUNKS];
  float pre_norm = 0.f;
  auto fetch = [&](unsigned t) {
    const f32x4* src = reinterpret_cast<const f32x4*>(tpack + (P.t_pack + static_cast<size_t>(t) * kMatchTile) * DP);
#pragma unroll
    for (int u = 0; u < CHUNKS; ++u) pre[u] = src[tid + u * kMatchBlock];
    if (tid < kMatchTile) pre_norm = tnorm[P.t_pack + static_cast<size_t>(t) * kMatchTile + tid];
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int u = 0; u < CHUNKS; ++u) {
      const int c = tid + u * kMatchBlock, row = c / (DP / 4), col = c % (DP / 4);
      *reinterpret_cast<f32x4*>(&s_tile[buf][row * LDS_ROW + col * 4]) = pre[u];
    }
    if (tid < kMatchTile) s_norm[buf][tid] = pre_norm;
  };
  if (t_begin < t_end) {
    fetch(t_begin);
    stash(0);
  }
  __syncthreads();
  for (unsigned t = t_begin; t < t_end; ++t) {
    const int buf = static_cast<int>((t - t_begin) & 1);
    const bool more = t + 1 < t_end;
    if (more) fetch(t + 1);
    f32x16 acc[QT];
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const f32x4 n4 = *reinterpret_cast<const f32x4*>(&s_norm[buf][8 * g4 + 4 * h]);
#pragma unroll
      for (int qt = 0; qt < QT; ++qt)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[qt][4 * g4 + r] = n4[r];
    }
    const float* arow = &s_tile[buf][j * LDS_ROW + h * HALF];
#pragma unroll
    for (int m = 0; m < HALF / 4; ++m) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(arow + 4 * m);
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) acc[qt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], qb[qt][m][e], acc[qt], 0, 0, 0);
    }
    const int base = static_cast<int>(t) * kMatchTile + 4 * h;
#pragma unroll
    for (int qt = 0; qt < QT; ++qt)
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const float s = acc[qt][reg];        // NaN (padding row, non-finite row) never passes a `<`
        const int idx = base + 8 * (reg >> 2) + (reg & 3);
        const bool c0 = s < b0[qt], c1 = s < b1[qt];
        b1[qt] = c0 ? b0[qt] : (c1 ? s : b1[qt]);
        i1[qt] = c0 ? i0[qt] : (c1 ? idx : i1[qt]);
        b0[qt] = c0 ? s : b0[qt];
        i0[qt] = c0 ? idx : i0[qt];
      }
    if (more) stash(buf ^ 1);     // buf ^ 1 was last read before the previous barrier
    __syncthreads();
  }
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const float o0 = __shfl_xor(b0[qt], 32), o1 = __shfl_xor(b1[qt], 32);
    const int oi0 = __shfl_xor(i0[qt], 32), oi1 = __shfl_xor(i1[qt], 32);
    insert_top2(o0, oi0, b0[qt], i0[qt], b1[qt], i1[qt]);
    insert_top2(o1, oi1, b0[qt], i0[qt], b1[qt], i1[qt]);
    if (h == 0)
      part[prow[qt] * splits + it.split] = make_float4(b0[qt], __int_as_float(i0[qt]), b1[qt], __int_as_float(i1[qt]));
  }
}

__device__ __forceinline__ float rescore(const float* __restrict__ q, const float* __restrict__ t, int dim) {
  float acc = 0.f;
  for (int k = 0; k < dim; ++k) {
    const float d = q[k] - t[k];
    acc = fmaf(d, d, acc);
  }
  return acc;
}

__global__ __launch_bounds__(256) void match_finish_kernel(const uint8_t* __restrict__ query, const uint8_t* __restrict__ train,
                                                           size_t stride, int dim, float ratio, const MatchPair* __restrict__ pairs,
                                                           int num_pairs, const unsigned long long* __restrict__ qoff_rel,
                                                           size_t total, int splits, const float4* __restrict__ part,
                                                           int* __restrict__ nn_index, float* __restrict__ nn_dist,
                                                           unsigned char* __restrict__ keep, unsigned int* __restrict__ pair_count) {
  const size_t r = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x;
  if (r >= total) return;
  const int g = batch_pair_of(r, qoff_rel, num_pairs);
  const size_t local = r - qoff_rel[g];
  const MatchPair P = pairs[g];
  const float inf = __int_as_float(0x7f800000);
  float b0 = inf, b1 = inf;
  int i0 = -1, i1 = -1;
  const float4* pp = part + (P.q_pack + local) * splits;
  for (int s = 0; s < splits; ++s) {
    const float4 v = pp[s];
    insert_top2(v.x, __float_as_int(v.y), b0, i0, b1, i1);
    insert_top2(v.z, __float_as_int(v.w), b0, i0, b1, i1);
  }
  const float* q = reinterpret_cast<const float*>(query + (P.q_row0 + local) * stride);
  bool q_finite = true;
  for (int k = 0; k < dim; ++k) q_finite = q_finite && isfinite(q[k]);
  if (!q_finite) i0 = i1 = -1;
  float r0 = inf, r1 = inf;
  if (i0 >= 0) r0 = rescore(q, reinterpret_cast<const float*>(train + (P.t_row0 + static_cast<size_t>(i0)) * stride), dim);
  if (i1 >= 0) r1 = rescore(q, reinterpret_cast<const float*>(train + (P.t_row0 + static_cast<size_t>(i1)) * stride), dim);
  if (i1 >= 0 && (r1 < r0 || (r1 == r0 && i1 < i0))) {
    const float tr = r0; r0 = r1; r1 = tr;
    const int ti = i0; i0 = i1; i1 = ti;
  }
  const float d0 = i0 >= 0 ? sqrtf(r0) : inf, d1 = i1 >= 0 ? sqrtf(r1) : inf;
  const bool accept = i0 >= 0 && i1 >= 0 && d0 < ratio * d1;      // feature_matcher.cpp:52, in float
  reinterpret_cast<int2*>(nn_index)[r] = make_int2(i0, i1);
  reinterpret_cast<float2*>(nn_dist)[r] = make_float2(d0, d1);
  if (accept) {
    keep[r] = 1;
    atomicAdd(&pair_count[g], 1u);
  }
}

// Block b = scan tile b (kCompactTile rows, 8 rounds of 256): as compact_scatter_kernel of sba_select.hip.
__global__ __launch_bounds__(256) void match_scatter_kernel(const unsigned char* __restrict__ keep, size_t total,
                                                            const unsigned long long* __restrict__ tile_offset,
                                                            const MatchPair* __restrict__ pairs, int num_pairs,
                                                            const unsigned long long* __restrict__ qoff_rel,
                                                            const int* __restrict__ nn_index, const float* __restrict__ nn_dist,
                                                            int* __restrict__ match_q, int* __restrict__ match_t,
                                                            float* __restrict__ match_d, unsigned long long* __restrict__ rows_q,
                                                            unsigned long long* __restrict__ rows_t) {
  __shared__ unsigned int wave_cnt[2][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t tile0 = static_cast<size_t>(blockIdx.x) * kCompactTile;
  unsigned long long pos0 = tile_offset[blockIdx.x];
  for (int r = 0; r < kCompactTile / 256; ++r) {
    const size_t i = tile0 + static_cast<size_t>(r) * 256 + threadIdx.x;
    const bool k = i < total && keep[i] != 0;
    const unsigned long long m = __ballot(k);
    const unsigned rank = __builtin_amdgcn_mbcnt_hi(static_cast<unsigned>(m >> 32),
                                                    __builtin_amdgcn_mbcnt_lo(static_cast<unsigned>(m), 0u));
    if (lane == 0) wave_cnt[r & 1][wave] = static_cast<unsigned>(__popcll(m));
    __syncthreads();
    unsigned before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const unsigned c = wave_cnt[r & 1][w];
      before += w < wave ? c : 0u;
      all += c;
    }
    if (k) {
      const size_t o = pos0 + before + rank;
      const int g = batch_pair_of(i, qoff_rel, num_pairs);
      const size_t local = i - qoff_rel[g];
      const int ti = nn_index[2 * i];
      match_q[o] = static_cast<int>(local);
      match_t[o] = ti;
      match_d[o] = nn_dist[2 * i];
      if (rows_q) {
        rows_q[o] = pairs[g].q_row0 + local;
        rows_t[o] = pairs[g].t_row0 + static_cast<unsigned long long>(ti);
      }
    }
    pos0 += all;
  }
}

unsigned grid_of(size_t n) { return static_cast<unsigned>((n + 255) / 256); }

}  // namespace

hipError_t launch_match_pack(const uint8_t* src, size_t stride_bytes, int dim, int dp, const MatchPair* pairs, int num_pairs,
                             const unsigned long long* off_rel, size_t total_rows, int side, float* pack, float* norm,
                             hipStream_t stream) {
  if (total_rows == 0) return hipSuccess;
  hipLaunchKernelGGL(match_pack_kernel, dim3(grid_of(total_rows)), dim3(256), 0, stream, src, stride_bytes, dim, dp, pairs,
                     num_pairs, off_rel, total_rows, side, pack, norm);
  return hipGetLastError();
}

hipError_t launch_match_tiles(int dp, const float* qpack, const float* tpack, const float* tnorm, const MatchPair* pairs,
                              const MatchItem* items, size_t n_items, int splits, float4* part, hipStream_t stream) {
  if (n_items == 0) return hipSuccess;
  const dim3 grid(static_cast<unsigned>(n_items)), block(kMatchBlock);
  switch (dp) {
    case 64:
      hipLaunchKernelGGL((match_tiles_kernel<64, 2>), grid, block, 0, stream, qpack, tpack, tnorm, pairs, items, splits, part);
      break;
    case 128:
      hipLaunchKernelGGL((match_tiles_kernel<128, 2>), grid, block, 0, stream, qpack, tpack, tnorm, pairs, items, splits, part);
      break;
    case 256:
      hipLaunchKernelGGL((match_tiles_kernel<256, 1>), grid, block, 0, stream, qpack, tpack, tnorm, pairs, items, splits, part);
      break;
    default:
      return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_match_finish(const uint8_t* query, const uint8_t* train, size_t stride_bytes, int dim, float ratio,
                               const MatchPair* pairs, int num_pairs, const unsigned long long* qoff_rel, size_t total_rows,
                               int splits, const float4* part, int* nn_index, float* nn_dist, unsigned char* keep,
                               unsigned int* pair_count, hipStream_t stream) {
  if (total_rows == 0) return hipSuccess;
  hipLaunchKernelGGL(match_finish_kernel, dim3(grid_of(total_rows)), dim3(256), 0, stream, query, train, stride_bytes, dim, ratio,
                     pairs, num_pairs, qoff_rel, total_rows, splits, part, nn_index, nn_dist, keep, pair_count);
  return hipGetLastError();
}

hipError_t launch_match_scatter(const unsigned char* keep, size_t total_rows, size_t ntiles,
                                const unsigned long long* tile_offset, const MatchPair* pairs, int num_pairs,
                                const unsigned long long* qoff_rel, const int* nn_index, const float* nn_dist, int* match_q,
                                int* match_t, float* match_d, unsigned long long* rows_q, unsigned long long* rows_t,
                                hipStream_t stream) {
  if (ntiles == 0) return hipSuccess;
  hipLaunchKernelGGL(match_scatter_kernel, dim3(static_cast<unsigned>(ntiles)), dim3(256), 0, stream, keep, total_rows,
                     tile_offset, pairs, num_pairs, qoff_rel, nn_index, nn_dist, match_q, match_t, match_d, rows_q, rows_t);
  return hipGetLastError();
}

}  // namespace sba
