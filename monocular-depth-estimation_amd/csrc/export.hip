// Prediction export: the model's fp32 depth -> (resampled) fp32 depth, a
// colour-mapped RGBA8 image and a 16-bit PNG payload, in one HBM-bound sweep
// (4 B read, <= 10 B written per output pixel).
//  - resize: align_corners=True bilinear with the taps and weights of
//    bilinear_fwd_kernel (bilinear.h), as evaluate.predict_depth(size=...) does
//    for the half-resolution AdaBins / Depthformer heads.
//  - rgba: utils/visualize_utils.py:10-29 (colorize) with matplotlib's
//    Colormap.__call__(bytes=True) restated in fp32: x = (d - vmin) / (vmax -
//    vmin) (x = d * 0 when vmin == vmax), x * 256 with 256 -> 255, truncation
//    to the LUT index; NaN -> the "bad" colour (0,0,0,0); d > vmax or d < vmin
//    -> white.  A true subtraction and a correctly rounded division: no
//    reciprocal, nothing for -ffp-contract to fuse.
//  - raw16: min(65535, rint(d * png_scale)), 0 for NaN and d <= 0 (0 is "no
//    measurement" in the KITTI / NYU depth PNGs).  A format decision: the
//    reference computes saving_factor (visualize_utils.py:34-37) and never
//    uses it.
// Four consecutive output pixels per thread (16-B rgba / depth stores, 8-B
// raw16 store) where the pointers are aligned, scalar otherwise and for the
// tail.  The 1 KB LUT is staged in LDS.
#include "bilinear.h"
#include "mdemi_ext.h"

namespace mdemi {

struct ExportArgs {
  const float* pred;
  const uint32_t* lut;  // 256 x RGBA8, byte order R,G,B,A
  float* depth_out;
  uint32_t* rgba;
  uint16_t* raw16;
  int64_t total;  // B*H*W output pixels
  int64_t in_hw;  // h*w
  int H, W;
  Axis ah, aw;
  float vmin, vmax, range, png_scale;
  int degenerate;  // vmin == vmax
  int vec_in, vec_depth, vec_rgba, vec_raw;
};

__device__ __forceinline__ uint32_t colour_of(float d, const ExportArgs& a, const uint32_t* lut) {
  if (d != d) return 0u;
  if (d > a.vmax || d < a.vmin) return 0xFFFFFFFFu;
  const float x = a.degenerate ? d * 0.f : (d - a.vmin) / a.range;
  const float s = x * 256.f;
  if (s != s) return 0u;
  int idx = s == 256.f ? 255 : (int)s;
  idx = idx < 0 ? 0 : (idx > 255 ? 255 : idx);  // matplotlib's under / over entries are the end colours
  return lut[idx];
}

__device__ __forceinline__ uint32_t raw16_of(float d, float png_scale) {
  return d > 0.f ? (uint32_t)fminf(rintf(d * png_scale), 65535.f) : 0u;
}

template <int RESIZE>
__device__ __forceinline__ float sample(const ExportArgs& a, int64_t p) {
  if (!RESIZE) return a.pred[p];
  const int ox = (int)(p % a.W);
  const int64_t t = p / a.W;
  const int oy = (int)(t % a.H);
  const int64_t n = t / a.H;
  int h1, hp, w1, wp; float hl1, wl1;
  a.ah.tap(oy, h1, hp, hl1);
  a.aw.tap(ox, w1, wp, wl1);
  const float* p00 = a.pred + n * a.in_hw + (int64_t)h1 * a.aw.in + w1;
  const float* p10 = p00 + (int64_t)hp * a.aw.in;
  return bilerp(1.f - hl1, hl1, 1.f - wl1, wl1, p00[0], p00[wp], p10[0], p10[wp]);
}

template <int RESIZE>
__global__ __launch_bounds__(256) void depth_export_kernel(ExportArgs a) {
  __shared__ uint32_t lut[256];
  if (a.rgba) {
    lut[threadIdx.x] = a.lut[threadIdx.x];  // blockDim.x == 256
    __syncthreads();
  }
  const int64_t groups = (a.total + 3) / 4;
  for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (int64_t)gridDim.x * blockDim.x) {
    const int64_t p0 = g * 4;
    const int cnt = a.total - p0 >= 4 ? 4 : (int)(a.total - p0);
    float d[4];
    if (!RESIZE && a.vec_in && cnt == 4) {
      const float4 q = *reinterpret_cast<const float4*>(a.pred + p0);
      d[0] = q.x; d[1] = q.y; d[2] = q.z; d[3] = q.w;
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) d[i] = i < cnt ? sample<RESIZE>(a, p0 + i) : 0.f;
    }
    if (a.depth_out) {
      if (a.vec_depth && cnt == 4) *reinterpret_cast<float4*>(a.depth_out + p0) = make_float4(d[0], d[1], d[2], d[3]);
      else
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (i < cnt) a.depth_out[p0 + i] = d[i];
    }
    if (a.rgba) {
      uint32_t c[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) c[i] = colour_of(d[i], a, lut);
      if (a.vec_rgba && cnt == 4) *reinterpret_cast<uint4*>(a.rgba + p0) = make_uint4(c[0], c[1], c[2], c[3]);
      else
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (i < cnt) a.rgba[p0 + i] = c[i];
    }
    if (a.raw16) {
      uint32_t r[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) r[i] = raw16_of(d[i], a.png_scale);
      if (a.vec_raw && cnt == 4)
        *reinterpret_cast<uint2*>(a.raw16 + p0) = make_uint2(r[0] | (r[1] << 16), r[2] | (r[3] << 16));
      else
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (i < cnt) a.raw16[p0 + i] = (uint16_t)r[i];
    }
  }
}

}  // namespace mdemi

using namespace mdemi;

extern "C" int mdemi_depth_export(const float* pred, int32_t B, int32_t h, int32_t w, int32_t H, int32_t W, float vmin,
                                  float vmax, const uint8_t* lut, float png_scale, float* depth_out, uint8_t* rgba,
                                  uint16_t* raw16, void* stream) {
  MDEMI_REQUIRE(pred && B > 0 && h > 0 && w > 0 && H > 0 && W > 0, "depth_export: bad args");
  MDEMI_REQUIRE(depth_out || rgba || raw16, "depth_export: no output requested");
  MDEMI_REQUIRE(!rgba || lut, "depth_export: rgba needs a lut");
  MDEMI_REQUIRE(!rgba || (((uintptr_t)rgba | (uintptr_t)lut) & 3) == 0, "depth_export: rgba / lut must be 4-byte aligned");
  MDEMI_REQUIRE(((uintptr_t)raw16 & 1) == 0 && (((uintptr_t)pred | (uintptr_t)depth_out) & 3) == 0,
                "depth_export: misaligned pointer");
  ExportArgs a;
  a.pred = pred;
  a.lut = reinterpret_cast<const uint32_t*>(lut);
  a.depth_out = depth_out;
  a.rgba = reinterpret_cast<uint32_t*>(rgba);
  a.raw16 = raw16;
  a.total = (int64_t)B * H * W;
  a.in_hw = (int64_t)h * w;
  a.H = H; a.W = W;
  a.ah = make_axis(h, H, 1, 0.f);
  a.aw = make_axis(w, W, 1, 0.f);
  a.vmin = vmin; a.vmax = vmax;
  a.range = (float)((double)vmax - (double)vmin);
  a.png_scale = png_scale;
  a.degenerate = vmin == vmax;
  a.vec_in = ((uintptr_t)pred & 15) == 0;
  a.vec_depth = ((uintptr_t)depth_out & 15) == 0;
  a.vec_rgba = ((uintptr_t)rgba & 15) == 0;
  a.vec_raw = ((uintptr_t)raw16 & 7) == 0;
  const int64_t nb = cdiv(cdiv(a.total, 4), 256);
  const dim3 grid((unsigned)(nb < 8192 ? nb : 8192));
  hipStream_t st = (hipStream_t)stream;
  if (h == H && w == W) hipLaunchKernelGGL(depth_export_kernel<0>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(depth_export_kernel<1>, grid, dim3(256), 0, st, a);
  return check_launch("depth_export");
}
