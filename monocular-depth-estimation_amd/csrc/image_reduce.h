// The fixed-order reductions and the exact radix select behind the per-image losses and metrics
// (silog, gradmatch, ssi, align, metrics_kernel.h).  Two runs must give the same
// bits, so every summation order here is part of a result: change none of them.  Device only;
// blocks of 256 threads (four waves) unless a helper says otherwise.
#pragma once
#include "common.h"

namespace mdemi {

// ---- sums --------------------------------------------------------------------------------------
// four waves' sums, pairwise: (0 + 1) + (2 + 3), widened to fp64 before the first add
template <typename T>
__device__ __forceinline__ double pair_sum4(const T (&r)[4]) {
  return ((double)r[0] + (double)r[1]) + ((double)r[2] + (double)r[3]);
}

// out[i] = the block's sum of acc[i]: the wave tree in T, lane 0 to LDS, then pair_sum4
template <typename T, int N>
__device__ __forceinline__ void block_store_pairwise(const T (&acc)[N], double* __restrict__ out) {
  __shared__ T red[N][4];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const T v = wave_sum(acc[i]);
    if (lane == 0) red[i][wid] = v;
  }
  __syncthreads();
  if (threadIdx.x < N) out[threadIdx.x] = pair_sum4(red[threadIdx.x]);
}

// red[q][0] = the sum over the 256 threads of acc[q]: a halving tree through LDS (thread t adds
// t + 128, then t + 64, ...).  Ends with a barrier; the caller puts one before red is reused.
template <int N>
__device__ __forceinline__ void block_tree_sum(const double (&acc)[N], double (&red)[N][256]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int q = 0; q < N; ++q) red[q][t] = acc[q];
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) {
#pragma unroll
      for (int q = 0; q < N; ++q) red[q][t] += red[q][t + w];
    }
    __syncthreads();
  }
}

// m[i] = the sum over an image's chunks of part[chunk][i], the same in every lane of the calling
// wave: lane l adds chunks l, l + 64, ... in that order, then the wave tree.  (One thread adding
// the 150 chunks of a 480x640 image in chunk order made the SSI forward's two small kernels cost
// more than its two sweeps; this order is as fixed as that one.)
template <int N>
__device__ __forceinline__ void chunk_sums_strided(const double* __restrict__ part, int nchunk, double (&m)[N]) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int i = 0; i < N; ++i) m[i] = 0.0;
  for (int c = lane; c < nchunk; c += 64) {
#pragma unroll
    for (int i = 0; i < N; ++i) m[i] += part[(int64_t)c * N + i];
  }
#pragma unroll
  for (int i = 0; i < N; ++i) m[i] = wave_sum(m[i]);
}

// ---- least squares ---------------------------------------------------------------------------
// the operand of the fit: the depth itself, or its fp64 reciprocal
template <bool DISP>
__device__ __forceinline__ double lsq_operand(float v) {
  return DISP ? 1.0 / (double)v : (double)v;
}

// argmin sum (s x + t - y)^2 by the normal equations; the caller decides what det allows
struct LsqFit {
  double det, s, t;
};
__device__ __forceinline__ LsqFit lsq_fit(double n, double sx, double sy, double sxx, double sxy) {
  const double det = n * sxx - sx * sx;
  return {det, (n * sxy - sx * sy) / det, (sxx * sy - sx * sxy) / det};
}

// ---- radix select ------------------------------------------------------------------------------
// An exact rank selection over 32-bit keys in three passes of 11 / 11 / 10 bits.  Each pass counts,
// among the keys that start with the prefix found so far, the next bits (an LDS histogram per
// workgroup, flushed with integer global atomics: the order does not matter) and rs_rank_step
// picks the bin that holds the rank.
constexpr int RS_BINS = 2048;  // 11 bits; the last pass uses 1024 of them

__host__ __device__ inline int rs_shift(int pass) { return pass == 0 ? 21 : (pass == 1 ? 10 : 0); }
__host__ __device__ inline int rs_bins(int pass) { return pass == 2 ? 1024 : 2048; }
// key bits already fixed by the passes before `pass`
__host__ __device__ inline uint32_t rs_mask(int pass) {
  return pass == 0 ? 0u : (pass == 1 ? 0xFFE00000u : 0xFFFFFC00u);
}

// monotone in the float order, total on the bits: -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN
__device__ __forceinline__ uint32_t rs_key(float v) {
  const uint32_t u = __float_as_uint(v);
  return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float rs_unkey(uint32_t k) {
  return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu));
}

// the workgroup's LDS histogram(s): n words cleared, with the barrier that follows
__device__ __forceinline__ void rs_hist_zero(uint32_t* h, int n) {
  for (int i = threadIdx.x; i < n; i += 256) h[i] = 0u;
  __syncthreads();
}
// out[i] += h[i], i < nb; the caller's barrier comes first
__device__ __forceinline__ void rs_hist_flush(const uint32_t* h, uint32_t* __restrict__ out, int nb) {
  for (int i = threadIdx.x; i < nb; i += 256) {
    const uint32_t c = h[i];
    if (c) atomicAdd(&out[i], c);
  }
}

struct RsStep {
  bool found;             // in one lane at most; in none when the table is empty
  uint32_t prefix, rank;  // in that lane: the prefix with the bin appended, the rank within the bin
  uint32_t total;         // the table's sum, in every lane
};
// One wave on a table of RS_BINS counts (zero past rs_bins(pass)): lane l holds
// bins 32 l .. 32 l + 31 in registers, a wave scan finds the lane and then the bin that holds
// rank_of(total).
template <typename RankOf>
__device__ __forceinline__ RsStep rs_rank_step(const uint32_t* table, int pass, uint32_t pre, RankOf rank_of) {
  constexpr int PER = RS_BINS / 64;
  const int lane = threadIdx.x & 63;
  uint32_t c[PER], sum = 0;
#pragma unroll
  for (int i = 0; i < PER; ++i) {  // scalar in the source: the table may be only 4-byte aligned
    c[i] = table[lane * PER + i];
    sum += c[i];
  }
  uint32_t incl = sum;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t v = __shfl_up(incl, o, 64);
    if (lane >= o) incl += v;
  }
  const uint32_t excl = incl - sum, total = __shfl(incl, 63, 64);
  const uint32_t rank = rank_of(total);
  RsStep s{false, pre, rank, total};
  if (rank >= excl && rank < incl) {
    uint32_t r = rank - excl;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      if (!s.found && r < c[i]) {
        s.found = true;
        s.prefix = pre | ((uint32_t)(lane * PER + i) << rs_shift(pass));
        s.rank = r;
      }
      if (!s.found) r -= c[i];
    }
  }
  return s;
}

}  // namespace mdemi
