// Bilinear interpolation arithmetic shared by the resize sweeps (resample.hip)
// and the fused resize of the prediction export (export.hip), so both take the
// same taps and weights.  Source-index arithmetic follows ATen's
// upsample_bilinear2d (area_pixel_compute_source_index).
#pragma once
#include "common.h"

namespace mdemi {

struct Axis {
  int in, out, align;
  float scale;  // ATen rheight/rwidth
  __device__ __forceinline__ void tap(int o, int& i0, int& ip, float& l1) const {
    float src;
    if (align) src = scale * (float)o;
    else {
      src = scale * ((float)o + 0.5f) - 0.5f;
      src = src < 0.f ? 0.f : src;
    }
    i0 = (int)src;
    ip = (i0 < in - 1) ? 1 : 0;
    l1 = src - (float)i0;
  }
};

static inline Axis make_axis(int in, int out, int align, float user_scale) {
  Axis a;
  a.in = in; a.out = out; a.align = align;
  if (align) a.scale = out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f;
  else a.scale = user_scale > 0.f ? 1.f / user_scale : (float)in / (float)out;
  return a;
}

// value of the four taps (a, b on row h1; c, d on row h1 + hp) under the row / column weights
__device__ __forceinline__ float bilerp(float hl0, float hl1, float wl0, float wl1, float a, float b, float c,
                                        float d) {
  return hl0 * (wl0 * a + wl1 * b) + hl1 * (wl0 * c + wl1 * d);
}

}  // namespace mdemi
