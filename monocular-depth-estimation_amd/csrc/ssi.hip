// Scale- and shift-invariant loss (MiDaS / DPT / Depth Anything's data term), cfg loss.ssi_weight /
// ssi_space / ssi_trim / ssi_norm -- this framework's own definition (the comment in
// include/mdemi_ext.h; pinned by tests/ssi_ref.py):
//   per image, on V = gt > min_depth: x, y = p, g (depth) or 1/p, 1/g (disp, fp64 reciprocals);
//   (s, t) = argmin sum (s x + t - y)^2 from fp64 sums (lsq_fit, the solve of align_lsq_solve);
//   r = s x + t - y (fp64), rho = |(float) r|; tau = the u-th smallest rho, u = n - floor(trim n);
//   K = {rho <= tau}; Q = sum_K r^2, A = sum_K r x, Bt = sum_K r, U = |K|.
// Forward: sweep 1 (n, Sx, Sy, Sxx, Sxy, Syy) -> solve -> [trim > 0: an exact radix select of rank
// u - 1 over rho's float bits, 11/11/10 bits; its first pass writes rho once to a plane in the
// workspace, the other two read only that plane] -> sweep 2 (Q, A, Bt, U) -> finalize.  Backward:
// one streaming sweep that recomputes r and rho from coef with the forward's arithmetic
// (ssi_residual / ssi_rho / ssi_kept), so its K is the forward's bit for bit.
// Every sweep has grid (chunks, B); fp64 partials go through a fixed wave and block tree and the
// chunks of an image are summed in a fixed order (chunk_sums_strided); the histograms are integers:
// two runs give the same bits.  The sums, the fit and the select's steps are image_reduce.h's.
#include <type_traits>

#include "common.h"
#include "image_reduce.h"
#include "mdemi_ext.h"

namespace mdemi {

constexpr int SSI_THREADS = 256;
constexpr int SSI_P1 = 6;     // n, Sx, Sy, Sxx, Sxy, Syy
constexpr int SSI_P2 = 4;     // Q, A, Bt, U
constexpr int SSI_SOL = 12;   // the six sums, det, s, t, u, skip, v
constexpr int SSI_STATE = 4;    // uint32 per image: prefix, rank, 2 unused
constexpr int SSI_COEF = 8;     // s, t, tau, a, e0, e1, e2, status
constexpr uint32_t SSI_OFF = 0xFFFFFFFFu;  // plane value off V: no |float|'s bits, matches no prefix

// the one definition of r, rho and K's membership that forward and backward share
__device__ __forceinline__ double ssi_residual(double s, double t, double x, double y) { return fma(s, x, t) - y; }
__device__ __forceinline__ float ssi_rho(double r) { return fabsf((float)r); }
// rho <= tau; a NaN rho or tau keeps the pixel, so a non-finite image stays NaN throughout
__device__ __forceinline__ bool ssi_kept(float rho, float tau) { return !(rho > tau); }

// the pixels first, first + step, ... below end
struct SsiRange {
  int64_t first, end, step;
};
// chunk blockIdx.x of an image, [p0, p1) with both multiples of 4 when HW is, shared among the block's threads
template <bool VEC>
__device__ __forceinline__ SsiRange ssi_chunk(int64_t HW, int nchunk) {
  const int64_t per = ((HW + nchunk - 1) / nchunk + 3) & ~(int64_t)3;
  const int64_t p0 = min(HW, (int64_t)blockIdx.x * per), p1 = min(HW, p0 + per);
  constexpr int V = VEC ? 4 : 1;
  return {p0 + V * (int64_t)threadIdx.x, p1, V * SSI_THREADS};
}

// O[i] = f(in[i]...) on the pixels i of r, in order; with O a void* (pass SSI_NO_OUTPUT) f returns
// nothing and nothing is stored.  VEC: each input is loaded 4 pixels at a time, f runs on the four in
// turn and the four results go out as one vector (16-byte bases; r's three numbers multiples of 4).
// One body serves the sweeps with and without an output on purpose: written as two functions, the same
// loops gave ssi_resid<., 0, 1> six more VGPRs than before the helper existed.
constexpr void* SSI_NO_OUTPUT = nullptr;
template <bool VEC, typename TO, typename F, typename... TI>
__device__ __forceinline__ void ssi_sweep(const SsiRange r, TO* __restrict__ O, F f, const TI* __restrict__... in) {
  for (int64_t i = r.first; i < r.end; i += r.step) {
    if constexpr (VEC) {
      [&](const HIP_vector_type<TI, 4>... v) {
        if constexpr (std::is_void<TO>::value) {
          f(v.x...); f(v.y...); f(v.z...); f(v.w...);
        } else {
          *reinterpret_cast<HIP_vector_type<TO, 4>*>(O + i) = {f(v.x...), f(v.y...), f(v.z...), f(v.w...)};
        }
      }(*reinterpret_cast<const HIP_vector_type<TI, 4>*>(in + i)...);
    } else if constexpr (std::is_void<TO>::value) {
      f(in[i]...);
    } else {
      O[i] = f(in[i]...);
    }
  }
}

// part1[b][chunk][6]
template <bool DISP, bool VEC>
__global__ __launch_bounds__(SSI_THREADS) void ssi_moments(const float* __restrict__ pred, const float* __restrict__ gt,
                                                           double* __restrict__ part1, int64_t HW, float min_depth,
                                                           int nchunk) {
  const int b = blockIdx.y;
  const SsiRange r = ssi_chunk<VEC>(HW, nchunk);
  double acc[SSI_P1];
#pragma unroll
  for (int i = 0; i < SSI_P1; ++i) acc[i] = 0.0;
  ssi_sweep<VEC>(r, SSI_NO_OUTPUT, [&](float p, float g) {
    if (g > min_depth) {
      const double x = lsq_operand<DISP>(p), y = lsq_operand<DISP>(g);
      acc[0] += 1.0; acc[1] += x; acc[2] += y;
      acc[3] += x * x; acc[4] += x * y; acc[5] += y * y;
    }
  }, pred + (int64_t)b * HW, gt + (int64_t)b * HW);
  block_store_pairwise(acc, part1 + ((int64_t)b * nchunk + blockIdx.x) * SSI_P1);
}

// One wave per image: the sums, the solve, u and the skip rule.
__global__ __launch_bounds__(64) void ssi_solve(const double* __restrict__ part1, double* __restrict__ sol,
                                                int nchunk, float trim, int norm) {
  const int b = blockIdx.x;
  double m[SSI_P1];
  chunk_sums_strided(part1 + (int64_t)b * nchunk * SSI_P1, nchunk, m);
  if (threadIdx.x != 0) return;
  const double n = m[0], sy = m[2], syy = m[5];
  const LsqFit f = lsq_fit(n, m[1], sy, m[3], m[4]);
  double v = 1.0;
  if (norm == MDEMI_SSI_NORM_GT_VAR && n > 0) v = syy / n - (sy / n) * (sy / n);
  // a non-finite det or v is not skipped: the loss shows the NaN
  const bool skip = !(n > 0) || (isfinite(f.det) && f.det <= 0.0) || (isfinite(v) && v <= 0.0);
  double* o = sol + (int64_t)b * SSI_SOL;
  for (int i = 0; i < SSI_P1; ++i) o[i] = m[i];
  o[6] = f.det;
  o[7] = skip ? 0.0 : f.s;
  o[8] = skip ? 0.0 : f.t;
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
  __shared__ uint32_t h[RS_BINS];
  const int b = blockIdx.y;
  const SsiRange r = ssi_chunk<VEC>(HW, nchunk);
  const double s = sol[(int64_t)b * SSI_SOL + 7], t = sol[(int64_t)b * SSI_SOL + 8];
  rs_hist_zero(h, RS_BINS);
  ssi_sweep<VEC>(r, plane + (int64_t)b * HW, [&](float p, float g) -> uint32_t {
    if (!(g > min_depth)) return SSI_OFF;
    const uint32_t k = __float_as_uint(ssi_rho(ssi_residual(s, t, lsq_operand<DISP>(p), lsq_operand<DISP>(g))));
    atomicAdd(&h[k >> 21], 1u);
    return k;
  }, pred + (int64_t)b * HW, gt + (int64_t)b * HW);
  __syncthreads();
  rs_hist_flush(h, hist + (int64_t)b * RS_BINS, RS_BINS);
}

// Select passes 1 and 2: of the plane's values that start with the image's prefix, count the next bits.
template <bool VEC>
__global__ __launch_bounds__(SSI_THREADS) void ssi_hist_next(const uint32_t* __restrict__ plane,
                                                             const uint32_t* __restrict__ state,
                                                             uint32_t* __restrict__ hist, int64_t HW, int nchunk,
                                                             int pass) {
  __shared__ uint32_t h[RS_BINS];
  const int b = blockIdx.y;
  const SsiRange r = ssi_chunk<VEC>(HW, nchunk);
  const int shift = rs_shift(pass), nb = rs_bins(pass);
  const uint32_t mask = rs_mask(pass), pre = state[b * SSI_STATE];
  rs_hist_zero(h, RS_BINS);
  ssi_sweep<VEC>(r, SSI_NO_OUTPUT, [&](uint32_t k) {
    if ((k & mask) == pre) atomicAdd(&h[(k >> shift) & (uint32_t)(nb - 1)], 1u);
  }, plane + (int64_t)b * HW);
  __syncthreads();
  rs_hist_flush(h, hist + (int64_t)b * RS_BINS, nb);
}

// One wave per image: find the bin that holds the rank, append it to the prefix, make the rank
// relative to that bin (rs_rank_step) and clear the image's histogram for the next pass.  After
// pass 2 the prefix is tau's bits.  An image without a valid pixel finds no bin and keeps prefix 0.
__global__ __launch_bounds__(64) void ssi_select(uint32_t* __restrict__ state, uint32_t* __restrict__ hist,
                                                 const double* __restrict__ sol, int pass) {
  const int b = blockIdx.x;
  uint32_t* st = state + b * SSI_STATE;
  uint32_t* hb = hist + (int64_t)b * RS_BINS;
  const RsStep r = rs_rank_step(hb, pass, pass == 0 ? 0u : st[0], [&](uint32_t) {
    if (pass != 0) return st[1];
    const double u = sol[(int64_t)b * SSI_SOL + 9];
    return u >= 1.0 ? (uint32_t)u - 1u : 0u;
  });
  __syncthreads();  // every read of state and of the histogram is done
  if (r.found) { st[0] = r.prefix; st[1] = r.rank; }
  // the lane clears the 32 bins it read; ssi_fwd requires a 16-byte-aligned workspace
  uint4* mine = reinterpret_cast<uint4*>(hb) + threadIdx.x * (RS_BINS / 256);
#pragma unroll
  for (int i = 0; i < RS_BINS / 256; ++i) mine[i] = make_uint4(0u, 0u, 0u, 0u);
}

// part2[b][chunk][4] = Q, A, Bt, U over K; without trimming K = V and only Q is formed
template <bool DISP, bool TRIM, bool VEC>
__global__ __launch_bounds__(SSI_THREADS) void ssi_resid(const float* __restrict__ pred, const float* __restrict__ gt,
                                                         const double* __restrict__ sol,
                                                         const uint32_t* __restrict__ state,
                                                         double* __restrict__ part2, int64_t HW, float min_depth,
                                                         int nchunk) {
  const int b = blockIdx.y;
  const SsiRange r = ssi_chunk<VEC>(HW, nchunk);
  const double s = sol[(int64_t)b * SSI_SOL + 7], t = sol[(int64_t)b * SSI_SOL + 8];
  const float tau = TRIM ? __uint_as_float(state[b * SSI_STATE]) : 0.f;
  double acc[SSI_P2];
#pragma unroll
  for (int i = 0; i < SSI_P2; ++i) acc[i] = 0.0;
  ssi_sweep<VEC>(r, SSI_NO_OUTPUT, [&](float p, float g) {
    if (g > min_depth) {
      const double x = lsq_operand<DISP>(p);
      const double r = ssi_residual(s, t, x, lsq_operand<DISP>(g));
      if (TRIM) {
        if (ssi_kept(ssi_rho(r), tau)) { acc[0] += r * r; acc[1] += r * x; acc[2] += r; acc[3] += 1.0; }
      } else {
        acc[0] += r * r;
      }
    }
  }, pred + (int64_t)b * HW, gt + (int64_t)b * HW);
  block_store_pairwise(acc, part2 + ((int64_t)b * nchunk + blockIdx.x) * SSI_P2);
}

// One block.  Wave w owns images w, w + 4, ...: it sums their chunk partials (chunk_sums_strided) and
// adds their share of the batch sums; the four waves' shares combine in a fixed order.  Then thread t
// writes the coef rows of images t, t + 256, ...: s, t, tau, a = w s, e0, e1, e2 (the bracket's last two terms as
// e0 + e1 x + e2 y, exactly 0 without trimming) and the status (1: skipped, gradient exactly 0).
constexpr int SSIF_THREADS = 256;
__global__ __launch_bounds__(SSIF_THREADS) void ssi_finalize(const double* __restrict__ part2,
                                                             const double* __restrict__ sol,
                                                             const uint32_t* __restrict__ state, int nchunk, int B,
                                                             int trimmed, int per_image, float* __restrict__ loss,
                                                             double* __restrict__ coef) {
  constexpr int NW = SSIF_THREADS / 64;
  static_assert(NW == 4, "the waves' shares are combined by pair_sum4");
  __shared__ double red[3][NW];
  const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
  double num = 0.0, den = 0.0, used = 0.0;  // the same in every lane of the wave
  for (int b = wid; b < B; b += NW) {
    double q[SSI_P2];
    chunk_sums_strided(part2 + (int64_t)b * nchunk * SSI_P2, nchunk, q);
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
  num = pair_sum4(red[0]);
  den = pair_sum4(red[1]);
  used = pair_sum4(red[2]);
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
  const double x = lsq_operand<DISP>(p), y = lsq_operand<DISP>(g);
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
  constexpr int V = VEC ? 4 : 1;
  const SsiRange r{V * ((int64_t)blockIdx.x * SSI_THREADS + threadIdx.x), HW, V * (int64_t)gridDim.x * SSI_THREADS};
  ssi_sweep<VEC>(r, dpred + (int64_t)b * HW, [&](float p, float g) { return ssi_grad<DISP>(c, p, g, min_depth); },
                 pred + (int64_t)b * HW, gt + (int64_t)b * HW);
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
      hist = o; o += (size_t)B * RS_BINS * sizeof(uint32_t);
      plane = o; o += align_up((size_t)B * HW * sizeof(uint32_t), 256);
    }
    total = o;
  }
};

// f(std::bool_constant...) of the run-time switches: one kernel instantiation per combination
template <typename F>
static void ssi_dispatch(F f) {
  f();
}
template <typename F, typename... Bs>
static void ssi_dispatch(F f, bool b, Bs... rest) {
  if (b) ssi_dispatch([&](auto... c) { f(std::true_type{}, c...); }, rest...);
  else ssi_dispatch([&](auto... c) { f(std::false_type{}, c...); }, rest...);
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
  ssi_dispatch([&](auto D, auto V) {
    hipLaunchKernelGGL((ssi_moments<D.value, V.value>), grid, block, 0, st, pred, gt, part1, HW, min_depth, nchunk);
  }, disp, vec);
  hipLaunchKernelGGL(ssi_solve, dim3(B), dim3(64), 0, st, (const double*)part1, sol, nchunk, trim, norm);
  if (trimmed) {
    if (hipMemsetAsync(state, 0, lay.plane - lay.state, st) != hipSuccess) return check_launch("ssi_fwd (clear)");
    ssi_dispatch([&](auto D, auto V) {
      hipLaunchKernelGGL((ssi_hist_first<D.value, V.value>), grid, block, 0, st, pred, gt, (const double*)sol, plane,
                         hist, HW, min_depth, nchunk);
    }, disp, vec);
    hipLaunchKernelGGL(ssi_select, dim3(B), dim3(64), 0, st, state, hist, (const double*)sol, 0);
    for (int pass = 1; pass < 3; ++pass) {
      ssi_dispatch([&](auto V) {
        hipLaunchKernelGGL(ssi_hist_next<V.value>, grid, block, 0, st, (const uint32_t*)plane, (const uint32_t*)state,
                           hist, HW, nchunk, pass);
      }, vec);
      hipLaunchKernelGGL(ssi_select, dim3(B), dim3(64), 0, st, state, hist, (const double*)sol, pass);
    }
  }
  ssi_dispatch([&](auto D, auto T, auto V) {
    hipLaunchKernelGGL((ssi_resid<D.value, T.value, V.value>), grid, block, 0, st, pred, gt, (const double*)sol,
                       (const uint32_t*)state, part2, HW, min_depth, nchunk);
  }, disp, trimmed, vec);
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
  ssi_dispatch([&](auto D, auto V) {
    hipLaunchKernelGGL((ssi_bwd_kernel<D.value, V.value>), grid, block, 0, (hipStream_t)stream, pred, gt, coef, dloss,
                       dpred, HW, min_depth);
  }, disp, vec);
  return check_launch("ssi_bwd");
}
