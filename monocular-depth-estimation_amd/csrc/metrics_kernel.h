// Depth metrics: grid (chunks, B); 11 sums per image.  One pair of kernels for mdemi_depth_metrics
// (heads.hip, ALIGN = 0) and mdemi_depth_metrics_aligned (align.hip, ALIGN = 1): the aligned
// form turns pred into q from the image's (s, t) on the fly and then runs the same per-pixel
// arithmetic, chunking and combine order, so on a given q both give the same bits.
#pragma once
#include "common.h"
#include "image_reduce.h"
#include "mdemi_ext.h"

namespace mdemi {

constexpr int MET_N = 11;  // count, a1, a2, a3, abs_rel, sq_rel, sq, sq_log, err, err^2, log10

// What the ALIGN = 1 kernels read besides the metrics arguments.  It travels as a trailing
// argument pack that is empty at ALIGN = 0, so that instantiation keeps the argument list, and
// compiles to the instructions, it had before the switch existed.
struct MetAlign {
  const double* coef;  // [B][4]: s, t, n, status
  float* aligned;      // nullable [B][H][W]: q before the clamp, on every pixel
  int mode;            // MDEMI_ALIGN_*
};
__device__ __forceinline__ const MetAlign& met_align(const MetAlign& al) { return al; }

// q of DESIGN §1c: formed in fp64, rounded once to fp32; a failed image keeps its prediction
__device__ __forceinline__ float aligned_value(float p, double s, double t, bool failed, int mode, double inv_dmax) {
  if (failed) return p;
  if (mode == MDEMI_ALIGN_LSTSQ_DISP) return (float)(1.0 / fmax(s / (double)p + t, inv_dmax));
  return (float)(s * (double)p + t);
}

// chunk blockIdx.x of an image's HW pixels: [p0, p1)
__device__ __forceinline__ void met_chunk(int64_t HW, int nchunk, int64_t& p0, int64_t& p1) {
  const int64_t per = (HW + nchunk - 1) / nchunk;
  p0 = (int64_t)blockIdx.x * per;
  p1 = min(HW, p0 + per);
}
// pixel p of a W-wide image counts: inside the crop rectangle, ground truth g in (dmin, dmax)
__device__ __forceinline__ bool met_valid(int64_t p, int W, float g, int y0, int y1, int x0, int x1, float dmin,
                                          float dmax) {
  const int y = (int)(p / W), x = (int)(p % W);
  return !(y < y0 || y >= y1 || x < x0 || x >= x1 || !(g > dmin) || !(g < dmax));
}
// the same test for a caller that has (y, x) already (boundary.hip).  Stated again, not shared:
// routing met_valid through it reordered the compares of metrics_partial, whose instructions
// stay the parent's.
__device__ __forceinline__ bool met_valid_at(int y, int x, float g, int y0, int y1, int x0, int x1, float dmin,
                                             float dmax) {
  return !(y < y0 || y >= y1 || x < x0 || x >= x1 || !(g > dmin) || !(g < dmax));
}

template <int ALIGN, typename... AL>
__global__ __launch_bounds__(256) void metrics_partial(const float* __restrict__ pred, const float* __restrict__ gt,
                                                       double* __restrict__ part, int H, int W, int y0, int y1, int x0,
                                                       int x1, float dmin, float dmax, int clamp_pred, int nchunk,
                                                       AL... al_pack) {
  static_assert(sizeof...(AL) == (ALIGN ? 1 : 0), "ALIGN = 1 takes one MetAlign, ALIGN = 0 nothing");
  const int b = blockIdx.y;
  const int64_t HW = (int64_t)H * W;
  int64_t p0, p1;
  met_chunk(HW, nchunk, p0, p1);
  double s = 1.0, t = 0.0, inv_dmax = 0.0;
  bool failed = true;
  if constexpr (ALIGN != 0) {
    const MetAlign& al = met_align(al_pack...);
    s = al.coef[b * 4 + 0];
    t = al.coef[b * 4 + 1];
    failed = al.coef[b * 4 + 3] != 0.0;
    inv_dmax = 1.0 / (double)dmax;
  }
  float acc[MET_N];
#pragma unroll
  for (int i = 0; i < MET_N; ++i) acc[i] = 0.f;
  for (int64_t p = p0 + threadIdx.x; p < p1; p += 256) {
    const float g = gt[(int64_t)b * HW + p];
    const bool skip = !met_valid(p, W, g, y0, y1, x0, x1, dmin, dmax);
    float q;
    if constexpr (ALIGN != 0) {
      const MetAlign& al = met_align(al_pack...);
      if (skip && !al.aligned) continue;
      q = aligned_value(pred[(int64_t)b * HW + p], s, t, failed, al.mode, inv_dmax);
      if (al.aligned) al.aligned[(int64_t)b * HW + p] = q;  // off the valid set too
      if (skip) continue;
    } else {
      if (skip) continue;
      q = pred[(int64_t)b * HW + p];
    }
    if (clamp_pred) q = fminf(fmaxf(q, dmin), dmax);
    const float th = fmaxf(g / q, q / g);
    const float diff = g - q;
    const float lg = logf(g), lq = logf(q);
    const float err = lq - lg;
    acc[0] += 1.f;
    acc[1] += th < 1.25f ? 1.f : 0.f;
    acc[2] += th < 1.25f * 1.25f ? 1.f : 0.f;
    acc[3] += th < 1.25f * 1.25f * 1.25f ? 1.f : 0.f;
    acc[4] += fabsf(diff) / g;
    acc[5] += diff * diff / g;
    acc[6] += diff * diff;
    acc[7] += (lg - lq) * (lg - lq);
    acc[8] += err;
    acc[9] += err * err;
    acc[10] += fabsf(log10f(g) - log10f(q));
  }
  // float accumulators and wave tree; only the four waves' sums are added in fp64
  block_store_pairwise(acc, part + ((int64_t)b * nchunk + blockIdx.x) * MET_N);
}

// out rows are 10 wide, or 12 with the image's (s, t) appended when ALIGN
template <int ALIGN, typename... AL>
__global__ void metrics_final(const double* __restrict__ part, double* __restrict__ out, int B, int nchunk,
                              AL... al_pack) {
  static_assert(sizeof...(AL) == (ALIGN ? 1 : 0), "ALIGN = 1 takes one MetAlign, ALIGN = 0 nothing");
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  double s[MET_N];
  for (int i = 0; i < MET_N; ++i) s[i] = 0.0;
  // chunk order, one thread: chunk_sums_strided is faster but changes the numbers' last bits, a change of its own
  for (int c = 0; c < nchunk; ++c)
    for (int i = 0; i < MET_N; ++i) s[i] += part[((int64_t)b * nchunk + c) * MET_N + i];
  const double n = s[0];
  double* o = out + (int64_t)b * (ALIGN ? 12 : 10);
  const double inv = n > 0 ? 1.0 / n : 0.0;
  o[0] = s[1] * inv;
  o[1] = s[2] * inv;
  o[2] = s[3] * inv;
  o[3] = s[4] * inv;
  o[4] = s[5] * inv;
  o[5] = sqrt(s[6] * inv);
  o[6] = sqrt(s[7] * inv);
  const double me = s[8] * inv;
  o[7] = sqrt(fmax(s[9] * inv - me * me, 0.0)) * 100.0;
  o[8] = s[10] * inv;
  o[9] = n;
  if constexpr (ALIGN != 0) {
    const MetAlign& al = met_align(al_pack...);
    o[10] = al.coef[b * 4 + 0];
    o[11] = al.coef[b * 4 + 1];
  }
}

inline int metrics_chunks(int64_t HW) {
  int64_t c = cdiv(HW, 4096);
  return (int)(c < 1 ? 1 : (c > 256 ? 256 : c));
}

}  // namespace mdemi
