// Per-image scale/shift alignment of a depth prediction to its ground truth (cfg eval.align,
// DESIGN.md §1c) and the metrics of the aligned prediction.
//   median: s = median(g) / median(p) by an exact radix select over the valid pixels -- three
//     passes over 11/11/10 bits of a key that orders the float bits totally (so a NaN sorts,
//     it does not derail the select).  An even n needs ranks (n-1)/2 and n/2 of each array,
//     which may part ways in any pass: the four selections (pred low/high, gt low/high) each
//     keep a prefix and a rank.  While an array's two prefixes agree one histogram serves both.
//     Counts are integers (LDS, then global atomics): the result does not depend on the order.
//   lstsq / lstsq_disp: n, Sx, Sy, Sxx, Sxy in per-thread fp64 accumulators, a fixed wave and
//     block tree, per-chunk partials summed in chunk order by one thread per image.
// Every sweep has grid (chunks, B) with the chunking of the metrics kernel.
#include "common.h"
#include "image_reduce.h"
#include "mdemi_ext.h"
#include "metrics_kernel.h"

namespace mdemi {

constexpr int AL_SEL = 4;      // pred low, pred high, gt low, gt high
constexpr int AL_STATE = 12;   // uint32 per image: prefix[4], rank[4], n, 3 unused
constexpr int LSQ_N = 5;       // n, Sx, Sy, Sxx, Sxy

// hist[b][sel][bin] += number of valid pixels of chunk (blockIdx.x) whose key starts with
// selection sel's prefix and continues with bin.  hist is all zero on entry.
__global__ __launch_bounds__(256) void align_hist(const float* __restrict__ pred, const float* __restrict__ gt,
                                                  const uint32_t* __restrict__ state, uint32_t* __restrict__ hist,
                                                  int H, int W, int y0, int y1, int x0, int x1, float dmin, float dmax,
                                                  int nchunk, int pass) {
  __shared__ uint32_t h[AL_SEL][RS_BINS];
  const int b = blockIdx.y;
  const int64_t HW = (int64_t)H * W;
  int64_t p0, p1;
  met_chunk(HW, nchunk, p0, p1);
  const int shift = rs_shift(pass), nb = rs_bins(pass);
  const uint32_t mask = rs_mask(pass);
  uint32_t pre[AL_SEL];
#pragma unroll
  for (int s = 0; s < AL_SEL; ++s) pre[s] = pass == 0 ? 0u : state[b * AL_STATE + s];
  const bool two_p = pre[1] != pre[0], two_g = pre[3] != pre[2];  // uniform over the block
  rs_hist_zero(&h[0][0], AL_SEL * RS_BINS);
  for (int64_t p = p0 + threadIdx.x; p < p1; p += 256) {
    const float g = gt[(int64_t)b * HW + p];
    if (!met_valid(p, W, g, y0, y1, x0, x1, dmin, dmax)) continue;
    const uint32_t kp = rs_key(pred[(int64_t)b * HW + p]), kg = rs_key(g);
    const uint32_t bp = (kp >> shift) & (uint32_t)(nb - 1), bg = (kg >> shift) & (uint32_t)(nb - 1);
    if ((kp & mask) == pre[0]) atomicAdd(&h[0][bp], 1u);
    if (two_p && (kp & mask) == pre[1]) atomicAdd(&h[1][bp], 1u);
    if ((kg & mask) == pre[2]) atomicAdd(&h[2][bg], 1u);
    if (two_g && (kg & mask) == pre[3]) atomicAdd(&h[3][bg], 1u);
  }
  __syncthreads();
  uint32_t* out = hist + (int64_t)b * AL_SEL * RS_BINS;
#pragma unroll
  for (int s = 0; s < AL_SEL; ++s) {
    if ((s == 1 && !two_p) || (s == 3 && !two_g)) continue;
    rs_hist_flush(h[s], out + s * RS_BINS, nb);
  }
}

// One block per image, one wave per selection: find the bin that holds the selection's rank,
// append it to the prefix, make the rank relative to that bin (rs_rank_step), and clear the
// image's histograms for the next pass.  Pass 0 also derives n and the four ranks; pass 2 writes coef.
__global__ __launch_bounds__(256) void align_select(uint32_t* __restrict__ state, uint32_t* __restrict__ hist,
                                                    double* __restrict__ coef, int pass) {
  __shared__ uint32_t key_s[AL_SEL];
  const int b = blockIdx.x, sel = threadIdx.x >> 6;
  uint32_t* st = state + b * AL_STATE;
  uint32_t* hb = hist + (int64_t)b * AL_SEL * RS_BINS;
  const int arr = sel >> 1;
  const uint32_t pre_lo = pass == 0 ? 0u : st[arr * 2], pre_hi = pass == 0 ? 0u : st[arr * 2 + 1];
  // align_hist filled the high selection's table only where the two prefixes differ
  const uint32_t* table = hb + (pre_lo == pre_hi ? arr * 2 : sel) * RS_BINS;
  const RsStep r = rs_rank_step(table, pass, (sel & 1) ? pre_hi : pre_lo, [&](uint32_t total) {
    if (pass != 0) return st[AL_SEL + sel];
    return total ? ((sel & 1) ? total / 2 : (total - 1) / 2) : 0u;
  });
  if (threadIdx.x < AL_SEL) key_s[threadIdx.x] = 0u;
  __syncthreads();  // every read of state and of the histograms is done
  if (r.found) {
    st[sel] = r.prefix;
    st[AL_SEL + sel] = r.rank;
    key_s[sel] = r.prefix;
  }
  if (pass == 0 && threadIdx.x == 0) st[2 * AL_SEL] = r.total;  // n: every valid pixel is in pass 0's pred table
  for (int i = threadIdx.x; i < AL_SEL * RS_BINS; i += 256) hb[i] = 0u;
  if (pass != 2) return;
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t n = st[2 * AL_SEL];
    const double mp = 0.5 * ((double)rs_unkey(key_s[0]) + (double)rs_unkey(key_s[1]));
    const double mg = 0.5 * ((double)rs_unkey(key_s[2]) + (double)rs_unkey(key_s[3]));
    const bool ok = n > 0 && mp > 0.0;
    coef[b * 4 + 0] = ok ? mg / mp : 1.0;
    coef[b * 4 + 1] = 0.0;
    coef[b * 4 + 2] = (double)n;
    coef[b * 4 + 3] = ok ? 0.0 : 1.0;
  }
}

// part[b][chunk][5] = n, Sx, Sy, Sxx, Sxy of the chunk's valid pixels; x, y = p, g or 1/p, 1/g
template <bool DISP>
__global__ __launch_bounds__(256) void align_lsq_partial(const float* __restrict__ pred, const float* __restrict__ gt,
                                                         double* __restrict__ part, int H, int W, int y0, int y1,
                                                         int x0, int x1, float dmin, float dmax, int nchunk) {
  const int b = blockIdx.y;
  const int64_t HW = (int64_t)H * W;
  int64_t p0, p1;
  met_chunk(HW, nchunk, p0, p1);
  double acc[LSQ_N];
#pragma unroll
  for (int i = 0; i < LSQ_N; ++i) acc[i] = 0.0;
  for (int64_t p = p0 + threadIdx.x; p < p1; p += 256) {
    const float g = gt[(int64_t)b * HW + p];
    if (!met_valid(p, W, g, y0, y1, x0, x1, dmin, dmax)) continue;
    const double xv = lsq_operand<DISP>(pred[(int64_t)b * HW + p]), yv = lsq_operand<DISP>(g);
    acc[0] += 1.0;
    acc[1] += xv;
    acc[2] += yv;
    acc[3] += xv * xv;
    acc[4] += xv * yv;
  }
  block_store_pairwise(acc, part + ((int64_t)b * nchunk + blockIdx.x) * LSQ_N);
}

// One thread per image adds its chunks in chunk order.  (The lane-strided chunk_sums_strided is
// faster but changes the last bits of the evaluation numbers: a change of its own, not made here.)
__global__ void align_lsq_solve(const double* __restrict__ part, double* __restrict__ coef, int B, int nchunk) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  double s[LSQ_N];
  for (int i = 0; i < LSQ_N; ++i) s[i] = 0.0;
  for (int c = 0; c < nchunk; ++c)
    for (int i = 0; i < LSQ_N; ++i) s[i] += part[((int64_t)b * nchunk + c) * LSQ_N + i];
  const double n = s[0];
  const LsqFit f = lsq_fit(n, s[1], s[2], s[3], s[4]);
  const bool ok = n > 0 && isfinite(f.det) && f.det > 0.0;
  coef[b * 4 + 0] = ok ? f.s : 1.0;
  coef[b * 4 + 1] = ok ? f.t : 0.0;
  coef[b * 4 + 2] = n;
  coef[b * 4 + 3] = ok ? 0.0 : 1.0;
}

static bool align_mode_ok(int mode) { return mode >= MDEMI_ALIGN_MEDIAN && mode <= MDEMI_ALIGN_LSTSQ_DISP; }
static size_t align_state_bytes(int32_t B) { return align_up((size_t)B * AL_STATE * sizeof(uint32_t), 256); }

}  // namespace mdemi

using namespace mdemi;

extern "C" size_t mdemi_depth_align_workspace_size(int32_t B, int32_t H, int32_t W, int32_t mode) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  if (mode == MDEMI_ALIGN_MEDIAN) return align_state_bytes(B) + (size_t)B * AL_SEL * RS_BINS * sizeof(uint32_t);
  return align_up((size_t)B * metrics_chunks((int64_t)H * W) * LSQ_N * sizeof(double), 256);
}

extern "C" int mdemi_depth_align(const float* pred, const float* gt, int32_t B, int32_t H, int32_t W, int32_t y0,
                                 int32_t y1, int32_t x0, int32_t x1, float min_depth, float max_depth, int32_t mode,
                                 double* coef, void* workspace, void* stream) {
  MDEMI_REQUIRE(pred && gt && coef && B > 0 && B <= 65535 && H > 0 && W > 0, "depth_align: bad args");
  MDEMI_REQUIRE(align_mode_ok(mode), "depth_align: mode must be 1 (median), 2 (lstsq) or 3 (lstsq_disp), got %d", mode);
  if (!workspace) { set_error("depth_align: workspace required"); return MDEMI_EWORKSPACE; }
  MDEMI_REQUIRE(((uintptr_t)workspace & 7) == 0, "depth_align: workspace must be 8-byte aligned");
  const int nchunk = metrics_chunks((int64_t)H * W);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(nchunk, B);
  if (mode == MDEMI_ALIGN_MEDIAN) {
    uint32_t* state = (uint32_t*)workspace;
    uint32_t* hist = (uint32_t*)((char*)workspace + align_state_bytes(B));
    if (hipMemsetAsync(workspace, 0, mdemi_depth_align_workspace_size(B, H, W, mode), st) != hipSuccess)
      return check_launch("depth_align (clear)");
    for (int pass = 0; pass < 3; ++pass) {
      hipLaunchKernelGGL(align_hist, grid, dim3(256), 0, st, pred, gt, (const uint32_t*)state, hist, H, W, y0, y1, x0,
                         x1, min_depth, max_depth, nchunk, pass);
      hipLaunchKernelGGL(align_select, dim3(B), dim3(256), 0, st, state, hist, coef, pass);
    }
  } else {
    double* part = (double*)workspace;
    if (mode == MDEMI_ALIGN_LSTSQ_DISP)
      hipLaunchKernelGGL(align_lsq_partial<true>, grid, dim3(256), 0, st, pred, gt, part, H, W, y0, y1, x0, x1,
                         min_depth, max_depth, nchunk);
    else
      hipLaunchKernelGGL(align_lsq_partial<false>, grid, dim3(256), 0, st, pred, gt, part, H, W, y0, y1, x0, x1,
                         min_depth, max_depth, nchunk);
    hipLaunchKernelGGL(align_lsq_solve, dim3((unsigned)cdiv(B, 64)), dim3(64), 0, st, (const double*)part, coef, B,
                       nchunk);
  }
  return check_launch("depth_align");
}

extern "C" int mdemi_depth_metrics_aligned(const float* pred, const float* gt, int32_t B, int32_t H, int32_t W,
                                           int32_t y0, int32_t y1, int32_t x0, int32_t x1, float min_depth,
                                           float max_depth, int32_t clamp_pred, int32_t mode, const double* coef,
                                           float* aligned, double* out, void* workspace, void* stream) {
  MDEMI_REQUIRE(pred && gt && coef && out && B > 0 && B <= 65535 && H > 0 && W > 0, "depth_metrics_aligned: bad args");
  MDEMI_REQUIRE(align_mode_ok(mode),
                "depth_metrics_aligned: mode must be 1 (median), 2 (lstsq) or 3 (lstsq_disp), got %d", mode);
  if (!workspace) { set_error("depth_metrics_aligned: workspace required"); return MDEMI_EWORKSPACE; }
  const int nchunk = metrics_chunks((int64_t)H * W);
  hipStream_t st = (hipStream_t)stream;
  const MetAlign al{coef, aligned, mode};
  hipLaunchKernelGGL((metrics_partial<1, MetAlign>), dim3(nchunk, B), dim3(256), 0, st, pred, gt,
                     (double*)workspace, H, W, y0, y1, x0, x1, min_depth, max_depth, clamp_pred, nchunk, al);
  hipLaunchKernelGGL((metrics_final<1, MetAlign>), dim3((unsigned)cdiv(B, 64)), dim3(64), 0, st,
                     (const double*)workspace, out, B, nchunk, al);
  return check_launch("depth_metrics_aligned");
}
