// Scale- and shift-invariant loss (MiDaS / DPT / Depth Anything's data term), cfg loss.ssi_weight /
// ssi_space / ssi_trim / ssi_norm -- this framework's own definition (the comment in
// include/mdemi_ext.h; pinned by tests/ssi_ref.py):
//   per image, on V = gt > min_depth: x, y = p, g (depth) or 1/p, 1/g (disp, fp64 reciprocals);
//   (s, t) = argmin sum (s x + t - y)^2 from fp64 sums (the solve of align_lsq_solve);
//   r = s x + t - y (fp64), rho = |(float) r|; tau = the u-th smallest rho, u = n - floor(trim n);
//   K = {rho <= tau}; Q = sum_K r^2, A = sum_K r x, Bt = sum_K r, U = |K|.
// Forward: sweep 1 (n, Sx, Sy, Sxx, Sxy, Syy) -> solve -> [trim > 0: an exact radix select of rank
// u - 1 over rho's float bits, 11/11/10 bits; its first pass writes rho once to a plane in the
// workspace, the other two read only that plane] -> sweep 2 (Q, A, Bt, U) -> finalize.  Backward:
// one streaming sweep that recomputes r and rho from coef with the forward's arithmetic
// (ssi_residual / ssi_rho / ssi_kept), so its K is the forward's bit for bit.
// Every sweep has grid (chunks, B); fp64 partials go through a fixed wave and block tree and the
// chunks of an image are summed in a fixed order (ssi_chunk_sums); the histograms are integers: two
// runs give the same bits.
// The dozen lines shared in spirit with align.hip (pass shifts, the fp64 wave sum, the wave scan)
// are repeated here; align.hip is left as it is.
#include "common.h"
#include "mdemi_ext.h"

namespace mdemi {

constexpr int SSI_THREADS = 256;
constexpr int SSI_P1 = 6;     // n, Sx, Sy, Sxx, Sxy, Syy
constexpr int SSI_P2 = 4;     // Q, A, Bt, U
constexpr int SSI_SOL = 12;   // the six sums, det, s, t, u, skip, v
constexpr int SSI_BINS = 2048;  // 11 bits; the last pass uses 1024 of them
constexpr int SSI_STATE = 4;    // uint32 per image: prefix, rank, 2 unused
constexpr int SSI_COEF = 8;     // s, t, tau, a, e0, e1, e2, status
constexpr uint32_t SSI_OFF = 0xFFFFFFFFu;  // plane value off V: no |float|'s bits, matches no prefix

__host__ __device__ inline int ssi_shift(int pass) { return pass == 0 ? 21 : (pass == 1 ? 10 : 0); }
__host__ __device__ inline int ssi_bins(int pass) { return pass == 2 ? 1024 : 2048; }
__host__ __device__ inline uint32_t ssi_mask(int pass) {
  return pass == 0 ? 0u : (pass == 1 ? 0xFFE00000u : 0xFFFFFC00u);
}

template <bool DISP>
__device__ __forceinline__ double ssi_x(float v) {
  return DISP ? 1.0 / (double)v : (double)v;
}
// the one definition of r, rho and K's membership that forward and backward share
__device__ __forceinline__ double ssi_residual(double s, double t, double x, double y) { return fma(s, x, t) - y; }
__device__ __forceinline__ float ssi_rho(double r) { return fabsf((float)r); }
// rho <= tau; a NaN rho or tau keeps the pixel, so a non-finite image stays NaN throughout
__device__ __forceinline__ bool ssi_kept(float rho, float tau) { return !(rho > tau); }

__device__ __forceinline__ double ssi_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// out[i] = the block's sum of acc[i]: wave tree, then the four waves in a fixed order
template <int N>
__device__ __forceinline__ void ssi_block_store(const double (&acc)[N], double* __restrict__ out) {
  __shared__ double red[N][SSI_THREADS / 64];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const double v = ssi_wave_sum(acc[i]);
    if (lane == 0) red[i][wid] = v;
  }
  __syncthreads();
  if (threadIdx.x < N) {
    const int i = threadIdx.x;
    out[i] = (red[i][0] + red[i][1]) + (red[i][2] + red[i][3]);
  }
}

// chunk ch of an image: [p0, p1), both multiples of 4 when HW is
__device__ __forceinline__ void ssi_chunk(int64_t HW, int nchunk, int64_t& p0, int64_t& p1) {
  const int64_t per = ((HW + nchunk - 1) / nchunk + 3) & ~(int64_t)3;
  p0 = min(HW, (int64_t)blockIdx.x * per);
  p1 = min(HW, p0 + per);
}

// f(i, p, g) on every pixel i of [p0, p1) of the image; VEC: 4-pixel loads (HW % 4 == 0, 16-byte bases)
template <bool VEC, typename F>
__device__ __forceinline__ void ssi_sweep(const float* __restrict__ P, const float* __restrict__ G, int64_t p0,
                                          int64_t p1, F f) {
  if (VEC) {
    for (int64_t i = p0 + 4 * (int64_t)threadIdx.x; i < p1; i += 4 * SSI_THREADS) {
      const float4 p = *reinterpret_cast<const float4*>(P + i);
      const float4 g = *reinterpret_cast<const float4*>(G + i);
      f(i, p.x, g.x); f(i + 1, p.y, g.y); f(i + 2, p.z, g.z); f(i + 3, p.w, g.w);
    }
  } else {
    for (int64_t i = p0 + threadIdx.x; i < p1; i += SSI_THREADS) f(i, P[i], G[i]);
  }
}

// part1[b][chunk][6]
template <bool DISP, bool VEC>
__global__ __launch_bounds__(SSI_THREADS) void ssi_moments(const float* __restrict__ pred, const float* __restrict__ gt,
                                                           double* __restrict__ part1, int64_t HW, float min_depth,
                                                           int nchunk) {
  const int b = blockIdx.y;
  int64_t p0, p1;
  ssi_chunk(HW, nchunk, p0, p1);
  double acc[SSI_P1];
#pragma unroll
  for (int i = 0; i < SSI_P1; ++i) acc[i] = 0.0;
  ssi_sweep<VEC>(pred + (int64_t)b * HW, gt + (int64_t)b * HW, p0, p1, [&](int64_t, float p, float g) {
    if (g > min_depth) {
      const double x = ssi_x<DISP>(p), y = ssi_x<DISP>(g);
      acc[0] += 1.0; acc[1] += x; acc[2] += y;
      acc[3] += x * x; acc[4] += x * y; acc[5] += y * y;
    }
  });
  ssi_block_store<SSI_P1>(acc, part1 + ((int64_t)b * nchunk + blockIdx.x) * SSI_P1);
}

// m[i] = the sum over an image's chunks of part[chunk][i], the same in every lane: lane l adds chunks
// l, l + 64, ... in that order, then the wave tree.  (One thread adding the 150 chunks of a 480x640
// image in chunk order, as align_lsq_solve does, made the forward's two small kernels cost more
// than its two sweeps; this order is as fixed as that one.)
template <int N>
__device__ __forceinline__ void ssi_chunk_sums(const double* __restrict__ part, int nchunk, double (&m)[N]) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int i = 0; i < N; ++i) m[i] = 0.0;
  for (int c = lane; c < nchunk; c += 64) {
#pragma unroll
    for (int i = 0; i < N; ++i) m[i] += part[(int64_t)c * N + i];
  }
#pragma unroll
  for (int i = 0; i < N; ++i) m[i] = ssi_wave_sum(m[i]);
}

// One wave per image: the sums, the solve, u and the skip rule.
__global__ __launch_bounds__(64) void ssi_solve(const double* __restrict__ part1, double* __restrict__ sol,
                                                int nchunk, float trim, int norm) {
  const int b = blockIdx.x;
  double m[SSI_P1];
  ssi_chunk_sums<SSI_P1>(part1 + (int64_t)b * nchunk * SSI_P1, nchunk, m);
  if (threadIdx.x != 0) return;
  const double n = m[0], sx = m[1], sy = m[2], sxx = m[3], sxy = m[4], syy = m[5];
  const double det = n * sxx - sx * sx;
  double v = 1.0;
  if (norm == MDEMI_SSI_NORM_GT_VAR && n > 0) v = syy / n - (sy / n) * (sy / n);
  // a non-finite det or v is not skipped: the loss shows the NaN
  const bool skip = !(n > 0) || (isfinite(det) && det <= 0.0) || (isfinite(v) && v <= 0.0);
  double* o = sol + (int64_t)b * SSI_SOL;
  for (int i = 0; i < SSI_P1; ++i) o[i] = m[i];
  o[6] = det;
  o[7] = skip ? 0.0 : (n * sxy - sx * sy) / det;
  o[8] = skip ? 0.0 : (sxx * sy - sx * sxy) / det;
  o[9] = n - floor((double)trim * n);
  o[10] = skip ? 1.0 : 0.0;
  o[11] = v;
}

// Select pass 0: writes rho's bits to the plane (SSI_OFF off V) and counts their top 11 bits.
// hist[b][bin] is all zero on entry.
template <bool DISP, bool VEC>
__global__ __launch_bounds__(SSI_THREADS) void ssi_hist_first(const float* __restrict__ pred,
                                                              const float* __restrict__ gt,
                                                              const double* __restrict__ sol,
                                                              uint32_t* __restrict__ plane, uint32_t* __restrict__ hist,
                                                              int64_t HW, float min_depth, int nchunk) {
  __shared__ uint32_t h[SSI_BINS];
  const int b = blockIdx.y;
  int64_t p0, p1;
  ssi_chunk(HW, nchunk, p0, p1);
  const double s = sol[(int64_t)b * SSI_SOL + 7], t = sol[(int64_t)b * SSI_SOL + 8];
  for (int i = threadIdx.x; i < SSI_BINS; i += SSI_THREADS) h[i] = 0u;
  __syncthreads();
  const float* P = pred + (int64_t)b * HW;
  const float* G = gt + (int64_t)b * HW;
  uint32_t* R = plane + (int64_t)b * HW;
  auto code = [&](float p, float g) -> uint32_t {
    if (!(g > min_depth)) return SSI_OFF;
    const uint32_t k = __float_as_uint(ssi_rho(ssi_residual(s, t, ssi_x<DISP>(p), ssi_x<DISP>(g))));
    atomicAdd(&h[k >> 21], 1u);
    return k;
  };
  if (VEC) {
    for (int64_t i = p0 + 4 * (int64_t)threadIdx.x; i < p1; i += 4 * SSI_THREADS) {
      const float4 p = *reinterpret_cast<const float4*>(P + i);
      const float4 g = *reinterpret_cast<const float4*>(G + i);
      *reinterpret_cast<uint4*>(R + i) = make_uint4(code(p.x, g.x), code(p.y, g.y), code(p.z, g.z), code(p.w, g.w));
    }
  } else {
    for (int64_t i = p0 + threadIdx.x; i < p1; i += SSI_THREADS) R[i] = code(P[i], G[i]);
  }
  __syncthreads();
  uint32_t* out = hist + (int64_t)b * SSI_BINS;
  for (int i = threadIdx.x; i < SSI_BINS; i += SSI_THREADS) {
    const uint32_t c = h[i];
    if (c) atomicAdd(&out[i], c);
  }
}

// Select passes 1 and 2: of the plane's values that start with the image's prefix, count the next bits.
template <bool VEC>
__global__ __launch_bounds__(SSI_THREADS) void ssi_hist_next(const uint32_t* __restrict__ plane,
                                                             const uint32_t* __restrict__ state,
                                                             uint32_t* __restrict__ hist, int64_t HW, int nchunk,
                                                             int pass) {
  __shared__ uint32_t h[SSI_BINS];
  const int b = blockIdx.y;
  int64_t p0, p1;
  ssi_chunk(HW, nchunk, p0, p1);
  const int shift = ssi_shift(pass), nb = ssi_bins(pass);
  const uint32_t mask = ssi_mask(pass), pre = state[b * SSI_STATE];
  for (int i = threadIdx.x; i < SSI_BINS; i += SSI_THREADS) h[i] = 0u;
  __syncthreads();
  const uint32_t* R = plane + (int64_t)b * HW;
  auto count = [&](uint32_t k) {
    if ((k & mask) == pre) atomicAdd(&h[(k >> shift) & (uint32_t)(nb - 1)], 1u);
  };
  if (VEC) {
    for (int64_t i = p0 + 4 * (int64_t)threadIdx.x; i < p1; i += 4 * SSI_THREADS) {
      const uint4 k = *reinterpret_cast<const uint4*>(R + i);
      count(k.x); count(k.y); count(k.z); count(k.w);
    }
  } else {
    for (int64_t i = p0 + threadIdx.x; i < p1; i += SSI_THREADS) count(R[i]);
  }
  __syncthreads();
  uint32_t* out = hist + (int64_t)b * SSI_BINS;
  for (int i = threadIdx.x; i < nb; i += SSI_THREADS) {
    const uint32_t c = h[i];
    if (c) atomicAdd(&out[i], c);
  }
}

// One wave per image: find the bin that holds the rank, append it to the prefix, make the rank
// relative to that bin and clear the image's histogram for the next pass.  After pass 2 the
// prefix is tau's bits.  An image without a valid pixel finds no bin and keeps prefix 0.
__global__ __launch_bounds__(64) void ssi_select(uint32_t* __restrict__ state, uint32_t* __restrict__ hist,
                                                 const double* __restrict__ sol, int pass) {
  const int b = blockIdx.x, lane = threadIdx.x;
  uint32_t* st = state + b * SSI_STATE;
  uint32_t* hb = hist + (int64_t)b * SSI_BINS;
  constexpr int PER = SSI_BINS / 64;  // contiguous bins per lane, held in registers; pass 2's upper half is 0
  uint32_t c[PER];
  uint4* hv = reinterpret_cast<uint4*>(hb) + lane * (PER / 4);
  uint32_t sum = 0;
#pragma unroll
  for (int i = 0; i < PER / 4; ++i) {
    const uint4 v = hv[i];
    c[4 * i] = v.x; c[4 * i + 1] = v.y; c[4 * i + 2] = v.z; c[4 * i + 3] = v.w;
    sum += (v.x + v.y) + (v.z + v.w);
  }
  uint32_t incl = sum;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t v = __shfl_up(incl, o, 64);
    if (lane >= o) incl += v;
  }
  const uint32_t excl = incl - sum;
  const uint32_t pre = pass == 0 ? 0u : st[0];
  uint32_t rank;
  if (pass == 0) {
    const double u = sol[(int64_t)b * SSI_SOL + 9];
    rank = u >= 1.0 ? (uint32_t)u - 1u : 0u;
  } else {
    rank = st[1];
  }
  bool found = false;
  uint32_t new_pre = pre, new_rank = rank;
  if (rank >= excl && rank < incl) {  // at most one lane
    uint32_t r = rank - excl;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      if (!found && r < c[i]) {
        found = true;
        new_pre = pre | ((uint32_t)(lane * PER + i) << ssi_shift(pass));
        new_rank = r;
      }
      if (!found) r -= c[i];
    }
  }
  __syncthreads();  // every read of state and of the histogram is done
  if (found) { st[0] = new_pre; st[1] = new_rank; }
#pragma unroll
  for (int i = 0; i < PER / 4; ++i) hv[i] = make_uint4(0u, 0u, 0u, 0u);
}

// part2[b][chunk][4] = Q, A, Bt, U over K; without trimming K = V and only Q is formed
template <bool DISP, bool TRIM, bool VEC>
__global__ __launch_bounds__(SSI_THREADS) void ssi_resid(const float* __restrict__ pred, const float* __restrict__ gt,
                                                         const double* __restrict__ sol,
                                                         const uint32_t* __restrict__ state,
                                                         double* __restrict__ part2, int64_t HW, float min_depth,
                                                         int nchunk) {
  const int b = blockIdx.y;
  int64_t p0, p1;
  ssi_chunk(HW, nchunk, p0, p1);
  const double s = sol[(int64_t)b * SSI_SOL + 7], t = sol[(int64_t)b * SSI_SOL + 8];
  const float tau = TRIM ? __uint_as_float(state[b * SSI_STATE]) : 0.f;
  double acc[SSI_P2];
#pragma unroll
  for (int i = 0; i < SSI_P2; ++i) acc[i] = 0.0;
  ssi_sweep<VEC>(pred + (int64_t)b * HW, gt + (int64_t)b * HW, p0, p1, [&](int64_t, float p, float g) {
    if (g > min_depth) {
      const double x = ssi_x<DISP>(p);
      const double r = ssi_residual(s, t, x, ssi_x<DISP>(g));
      if (TRIM) {
        if (ssi_kept(ssi_rho(r), tau)) { acc[0] += r * r; acc[1] += r * x; acc[2] += r; acc[3] += 1.0; }
      } else {
        acc[0] += r * r;
      }
    }
  });
  ssi_block_store<SSI_P2>(acc, part2 + ((int64_t)b * nchunk + blockIdx.x) * SSI_P2);
}

// One block.  Wave w owns images w, w + 4, ...: it sums their chunk partials (ssi_chunk_sums) and adds
// their share of the batch sums; the four waves' shares combine in a fixed order.  Then thread t
// writes the coef rows of images t, t + 256, ...: s, t, tau, a = w s, e0, e1, e2 (the bracket's last two terms as
// e0 + e1 x + e2 y, exactly 0 without trimming) and the status (1: skipped, gradient exactly 0).
constexpr int SSIF_THREADS = 256;
__global__ __launch_bounds__(SSIF_THREADS) void ssi_finalize(const double* __restrict__ part2,
                                                             const double* __restrict__ sol,
                                                             const uint32_t* __restrict__ state, int nchunk, int B,
                                                             int trimmed, int per_image, float* __restrict__ loss,
                                                             double* __restrict__ coef) {
  constexpr int NW = SSIF_THREADS / 64;
  static_assert(NW == 4, "the waves' shares are combined as (0 + 1) + (2 + 3)");
  __shared__ double red[3][NW];
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  double num = 0.0, den = 0.0, used = 0.0;  // the same in every lane of the wave
  for (int b = wid; b < B; b += NW) {
    double q[SSI_P2];
    ssi_chunk_sums<SSI_P2>(part2 + (int64_t)b * nchunk * SSI_P2, nchunk, q);
    const double* o = sol + (int64_t)b * SSI_SOL;
    const double n = o[0], det = o[6], v = o[11];
    const bool skip = o[10] != 0.0;
    double Q = q[0], A = q[1], Bt = q[2], U = q[3];
    if (!trimmed) { A = 0.0; Bt = 0.0; U = n; }
    if (!isfinite(det)) Q = __longlong_as_double(0x7FF8000000000000ll);  // whatever K came out as
    if (lane == 0) {  // A, Bt, U wait in the coef row for the second loop
      double* c = coef + (int64_t)b * SSI_COEF;
      c[4] = A; c[5] = Bt; c[6] = U;
    }
    if (!skip) {
      used += 1.0;
      if (per_image) {
        num += Q / (2.0 * U * v);
      } else {
        num += Q / v;
        den += U;
      }
    }
  }
  if (lane == 0) { red[0][wid] = num; red[1][wid] = den; red[2][wid] = used; }
  __syncthreads();  // the coef rows (lane 0's global stores) are visible to the block from here too
  num = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
  den = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
  used = (red[2][0] + red[2][1]) + (red[2][2] + red[2][3]);
  if (t == 0) loss[0] = used > 0.0 ? (float)(per_image ? num / used : num / (2.0 * den)) : 0.f;
  for (int b = t; b < B; b += SSIF_THREADS) {
    const double* o = sol + (int64_t)b * SSI_SOL;
    const double n = o[0], sx = o[1], sy = o[2], det = o[6], s = o[7], tt = o[8], v = o[11];
    const bool skip = o[10] != 0.0;
    double* c = coef + (int64_t)b * SSI_COEF;
    const double A = c[4], Bt = c[5], U = c[6];
    const double w = skip ? 0.0 : (per_image ? 1.0 / (U * v * used) : 1.0 / (v * den));
    double e0 = 0.0, e1 = 0.0, e2 = 0.0;
    if (trimmed && !skip) {
      const double cd = (A - Bt * sx / n) / det;
      e0 = w * (cd * (2.0 * s * sx - sy) - Bt * s / n);
      e1 = -2.0 * w * cd * s * n;
      e2 = w * cd * n;
    }
    c[0] = s; c[1] = tt;
    c[2] = trimmed ? (double)__uint_as_float(state[b * SSI_STATE]) : (double)INFINITY;
    c[3] = w * s;
    c[4] = e0; c[5] = e1; c[6] = e2;
    c[7] = skip ? 1.0 : 0.0;
  }
}

struct SsiCoef {
  double s, t, a, e0, e1, e2, dl;
  float tau;
  bool skip;
};

template <bool DISP>
__device__ __forceinline__ float ssi_grad(const SsiCoef& c, float p, float g, float min_depth) {
  if (c.skip || !(g > min_depth)) return 0.f;
  const double x = ssi_x<DISP>(p), y = ssi_x<DISP>(g);
  const double r = ssi_residual(c.s, c.t, x, y);
  double d = fma(c.e1, x, fma(c.e2, y, c.e0));
  if (ssi_kept(ssi_rho(r), c.tau)) d = fma(r, c.a, d);
  d *= c.dl;
  if (DISP) d *= -(x * x);  // dx/dp = -1/p^2
  return (float)d;
}

template <bool DISP, bool VEC>
__global__ __launch_bounds__(SSI_THREADS) void ssi_bwd_kernel(const float* __restrict__ pred,
                                                              const float* __restrict__ gt,
                                                              const double* __restrict__ coef,
                                                              const float* __restrict__ dloss,
                                                              float* __restrict__ dpred, int64_t HW, float min_depth) {
  const int b = blockIdx.y;
  const double* cf = coef + (int64_t)b * SSI_COEF;
  SsiCoef c;
  c.s = cf[0]; c.t = cf[1]; c.tau = (float)cf[2]; c.a = cf[3];
  c.e0 = cf[4]; c.e1 = cf[5]; c.e2 = cf[6]; c.skip = cf[7] != 0.0;
  c.dl = (double)dloss[0];
  const float* P = pred + (int64_t)b * HW;
  const float* G = gt + (int64_t)b * HW;
  float* D = dpred + (int64_t)b * HW;
  if (VEC) {
    for (int64_t i = 4 * ((int64_t)blockIdx.x * SSI_THREADS + threadIdx.x); i < HW;
         i += 4 * (int64_t)gridDim.x * SSI_THREADS) {
      const float4 p = *reinterpret_cast<const float4*>(P + i);
      const float4 g = *reinterpret_cast<const float4*>(G + i);
      float4 o;
      o.x = ssi_grad<DISP>(c, p.x, g.x, min_depth); o.y = ssi_grad<DISP>(c, p.y, g.y, min_depth);
      o.z = ssi_grad<DISP>(c, p.z, g.z, min_depth); o.w = ssi_grad<DISP>(c, p.w, g.w, min_depth);
      *reinterpret_cast<float4*>(D + i) = o;
    }
  } else {
    for (int64_t i = (int64_t)blockIdx.x * SSI_THREADS + threadIdx.x; i < HW; i += (int64_t)gridDim.x * SSI_THREADS)
      D[i] = ssi_grad<DISP>(c, P[i], G[i], min_depth);
  }
}

static int ssi_chunks(int64_t HW) {
  const int64_t c = cdiv(HW, 2048);
  return (int)(c < 1 ? 1 : (c > 512 ? 512 : c));
}
static bool ssi_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the workspace's sections, each 256-byte aligned
struct SsiLayout {
  size_t sol, part1, part2, state, hist, plane, total;
  SsiLayout(int32_t B, int64_t HW, bool trimmed) {
    const size_t nch = (size_t)ssi_chunks(HW);
    size_t o = 0;
    sol = o; o += align_up((size_t)B * SSI_SOL * sizeof(double), 256);
    part1 = o; o += align_up((size_t)B * nch * SSI_P1 * sizeof(double), 256);
    part2 = o; o += align_up((size_t)B * nch * SSI_P2 * sizeof(double), 256);
    state = hist = plane = o;
    if (trimmed) {
      state = o; o += align_up((size_t)B * SSI_STATE * sizeof(uint32_t), 256);
      hist = o; o += (size_t)B * SSI_BINS * sizeof(uint32_t);
      plane = o; o += align_up((size_t)B * HW * sizeof(uint32_t), 256);
    }
    total = o;
  }
};

// one launch of KERNEL<DISP, VEC> by the two run-time switches
#define SSI_LAUNCH2(KERNEL, disp, vec, ...)                                                          \
  do {                                                                                               \
    if (disp) {                                                                                      \
      if (vec) hipLaunchKernelGGL((KERNEL<true, true>), __VA_ARGS__);                                \
      else hipLaunchKernelGGL((KERNEL<true, false>), __VA_ARGS__);                                   \
    } else {                                                                                         \
      if (vec) hipLaunchKernelGGL((KERNEL<false, true>), __VA_ARGS__);                               \
      else hipLaunchKernelGGL((KERNEL<false, false>), __VA_ARGS__);                                  \
    }                                                                                                \
  } while (0)

template <bool DISP, bool VEC>
static void ssi_launch_resid(bool trimmed, dim3 grid, hipStream_t st, const float* pred, const float* gt,
                             const double* sol, const uint32_t* state, double* part2, int64_t HW, float min_depth,
                             int nchunk) {
  if (trimmed)
    hipLaunchKernelGGL((ssi_resid<DISP, true, VEC>), grid, dim3(SSI_THREADS), 0, st, pred, gt, sol, state, part2, HW,
                       min_depth, nchunk);
  else
    hipLaunchKernelGGL((ssi_resid<DISP, false, VEC>), grid, dim3(SSI_THREADS), 0, st, pred, gt, sol, state, part2, HW,
                       min_depth, nchunk);
}

static int ssi_check_geom(const char* what, int32_t B, int32_t H, int32_t W, int32_t space) {
  MDEMI_REQUIRE(B >= 1 && B <= 65535, "%s: B must be 1..65535, got %d", what, B);
  MDEMI_REQUIRE(H > 0 && W > 0, "%s: H and W must be positive, got H=%d W=%d", what, H, W);
  MDEMI_REQUIRE(space == MDEMI_SSI_DEPTH || space == MDEMI_SSI_DISP, "%s: space must be 0 (depth) or 1 (disp), got %d",
                what, space);
  return MDEMI_OK;
}

}  // namespace mdemi

using namespace mdemi;

extern "C" size_t mdemi_ssi_workspace_size(int32_t B, int32_t H, int32_t W, int32_t trimmed) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  return SsiLayout(B, (int64_t)H * W, trimmed != 0).total;
}

extern "C" int mdemi_ssi_fwd(const float* pred, const float* gt, float* loss, double* coef, int32_t B, int32_t H,
                             int32_t W, float min_depth, int32_t space, float trim, int32_t norm, int32_t per_image,
                             void* workspace, void* stream) {
  MDEMI_REQUIRE(pred && gt && loss && coef, "ssi_fwd: null pred, gt, loss or coef");
  if (int rc = ssi_check_geom("ssi_fwd", B, H, W, space)) return rc;
  MDEMI_REQUIRE(norm == MDEMI_SSI_NORM_NONE || norm == MDEMI_SSI_NORM_GT_VAR,
                "ssi_fwd: norm must be 0 (none) or 1 (gt_var), got %d", norm);
  MDEMI_REQUIRE(trim >= 0.f && trim <= 0.5f, "ssi_fwd: trim must be a finite number in [0, 0.5], got %g", (double)trim);
  if (!workspace) { set_error("ssi_fwd: workspace required"); return MDEMI_EWORKSPACE; }
  MDEMI_REQUIRE(ssi_aligned16(workspace), "ssi_fwd: workspace must be 16-byte aligned");
  MDEMI_REQUIRE(((uintptr_t)coef & 7) == 0, "ssi_fwd: coef must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int64_t HW = (int64_t)H * W;
  const bool trimmed = trim > 0.f, disp = space == MDEMI_SSI_DISP;
  const bool vec = HW % 4 == 0 && ssi_aligned16(pred) && ssi_aligned16(gt);
  const int nchunk = ssi_chunks(HW);
  const SsiLayout lay(B, HW, trimmed);
  char* ws = (char*)workspace;
  double* sol = (double*)(ws + lay.sol);
  double* part1 = (double*)(ws + lay.part1);
  double* part2 = (double*)(ws + lay.part2);
  uint32_t* state = (uint32_t*)(ws + lay.state);
  uint32_t* hist = (uint32_t*)(ws + lay.hist);
  uint32_t* plane = (uint32_t*)(ws + lay.plane);
  const dim3 grid(nchunk, B), block(SSI_THREADS);
  SSI_LAUNCH2(ssi_moments, disp, vec, grid, block, 0, st, pred, gt, part1, HW, min_depth, nchunk);
  hipLaunchKernelGGL(ssi_solve, dim3(B), dim3(64), 0, st, (const double*)part1, sol, nchunk, trim, norm);
  if (trimmed) {
    if (hipMemsetAsync(state, 0, lay.plane - lay.state, st) != hipSuccess) return check_launch("ssi_fwd (clear)");
    SSI_LAUNCH2(ssi_hist_first, disp, vec, grid, block, 0, st, pred, gt, (const double*)sol, plane, hist, HW, min_depth,
                nchunk);
    hipLaunchKernelGGL(ssi_select, dim3(B), dim3(64), 0, st, state, hist, (const double*)sol, 0);
    for (int pass = 1; pass < 3; ++pass) {
      if (vec)
        hipLaunchKernelGGL(ssi_hist_next<true>, grid, block, 0, st, (const uint32_t*)plane, (const uint32_t*)state,
                           hist, HW, nchunk, pass);
      else
        hipLaunchKernelGGL(ssi_hist_next<false>, grid, block, 0, st, (const uint32_t*)plane, (const uint32_t*)state,
                           hist, HW, nchunk, pass);
      hipLaunchKernelGGL(ssi_select, dim3(B), dim3(64), 0, st, state, hist, (const double*)sol, pass);
    }
  }
  if (disp) {
    if (vec) ssi_launch_resid<true, true>(trimmed, grid, st, pred, gt, sol, state, part2, HW, min_depth, nchunk);
    else ssi_launch_resid<true, false>(trimmed, grid, st, pred, gt, sol, state, part2, HW, min_depth, nchunk);
  } else {
    if (vec) ssi_launch_resid<false, true>(trimmed, grid, st, pred, gt, sol, state, part2, HW, min_depth, nchunk);
    else ssi_launch_resid<false, false>(trimmed, grid, st, pred, gt, sol, state, part2, HW, min_depth, nchunk);
  }
  hipLaunchKernelGGL(ssi_finalize, dim3(1), dim3(SSIF_THREADS), 0, st, (const double*)part2, (const double*)sol,
                     (const uint32_t*)state, nchunk, B, (int)trimmed, per_image, loss, coef);
  return check_launch("ssi_fwd");
}

extern "C" int mdemi_ssi_bwd(const float* pred, const float* gt, const double* coef, const float* dloss, float* dpred,
                             int32_t B, int32_t H, int32_t W, float min_depth, int32_t space, void* stream) {
  MDEMI_REQUIRE(pred && gt && coef && dloss && dpred, "ssi_bwd: null pred, gt, coef, dloss or dpred");
  if (int rc = ssi_check_geom("ssi_bwd", B, H, W, space)) return rc;
  const int64_t HW = (int64_t)H * W;
  const bool disp = space == MDEMI_SSI_DISP;
  const bool vec = HW % 4 == 0 && ssi_aligned16(pred) && ssi_aligned16(gt) && ssi_aligned16(dpred);
  const int64_t nb = cdiv(HW, SSI_THREADS * 8);
  const dim3 grid((unsigned)(nb < 1 ? 1 : (nb > 512 ? 512 : nb)), (unsigned)B), block(SSI_THREADS);
  SSI_LAUNCH2(ssi_bwd_kernel, disp, vec, grid, block, 0, (hipStream_t)stream, pred, gt, coef, dloss, dpred, HW,
              min_depth);
  return check_launch("ssi_bwd");
}
