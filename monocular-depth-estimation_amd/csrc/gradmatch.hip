// Multi-scale, scale-invariant gradient-matching loss (MegaDepth / MiDaS / DPT), cfg
// loss.grad_weight / loss.grad_scales -- this framework's own definition (DESIGN.md §1c;
// the reference's loss module is absent):
//   R = log(pred) - log(gt) on M = gt > min_depth
//   scale k (step s = 2^k) works on the grid R[::s, ::s]:
//     S_bk = sum |R(y, x+s) - R(y, x)| + sum |R(y+s, x) - R(y, x)|  over grid pairs valid at both ends
//     N_bk = number of valid grid pixels (MiDaS' normaliser)
//   per batch: L = sum_k (sum_b S_bk) / (sum_b N_bk); per image: L = mean over images with
//   N_b0 > 0 of sum_k S_bk / N_bk; an empty scale contributes 0.
//   dL/dpred = (1/pred) sum_k w_bk c_k, c_k = sum over the pixel's <= 4 scale-k neighbours n of
//   sign(R - R(n)), sign(0) = 0.
// Tiles are GM_TH x GM_TW pixels at multiples of 8, so a tile's scale-k grid is the image's.
// Each workgroup turns its tile (+ halo) into R once -- one logf pair per pixel -- in LDS and
// evaluates every scale from there.  The pair (p, p+s) belongs to p: the forward needs one
// halo row/column below/right (p+s of the tile's last grid pixel is the next tile's first).
// The backward is a gather: it also needs p-s, i.e. rows/columns -1,-2,-4,-8 above/left.
#include "common.h"
#include "image_reduce.h"
#include "mdemi_ext.h"

namespace mdemi {

constexpr int GM_THREADS = 256;
constexpr int GM_TH = 32, GM_TW = 128;  // tile; both multiples of the largest step
constexpr int GM_MAXK = 4;
constexpr int GM_HALO = 1 << (GM_MAXK - 1);  // 8: the largest step
constexpr int GM_RPAD = 4;                   // right halo: 1 column needed, 4 loaded (16-byte rows)
constexpr uint32_t GM_INVALID = 0xFFFFFFFFu;  // a NaN pattern no R below takes
constexpr uint32_t GM_QNAN = 0x7FC00000u;

static_assert(GM_TH % GM_HALO == 0 && GM_TW % GM_HALO == 0 && (GM_TW & (GM_TW - 1)) == 0, "tile");

// R's bits, or GM_INVALID off the mask; a NaN R (pred <= 0 / NaN) stays a NaN the loss shows
__device__ __forceinline__ uint32_t gm_code(float p, float g, float min_depth) {
  if (!(g > min_depth)) return GM_INVALID;
  const float r = logf(p) - logf(g);
  return r != r ? GM_QNAN : __float_as_uint(r);
}

// tile[r][c] <- code of image pixel (row_of(r), x0 + c); pixels outside the image are invalid.
// VEC: W % 4 == 0 and 16-byte aligned bases, x0 % 4 == 0 -- a 4-pixel vector is all in or all out.
template <int ROWS, int COLS, bool VEC, typename RowOf>
__device__ __forceinline__ void gm_fill(uint32_t* tile, const float* __restrict__ P, const float* __restrict__ G,
                                        int H, int W, int x0, float min_depth, RowOf row_of) {
  // Two phases -- every load of the thread issued, then the logf pairs and the LDS stores -- so
  // that a workgroup has its whole tile in flight at once: at 2-3 workgroups per CU the loads'
  // latency is not hidden by other waves.  gt = NaN stands for "outside" (never > min_depth).
  const float nan = __uint_as_float(GM_QNAN);
  if (VEC) {
    constexpr int CV = COLS / 4, NV = ROWS * CV, IT = (NV + GM_THREADS - 1) / GM_THREADS;
    float4 p[IT], g[IT];
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int i = threadIdx.x + it * GM_THREADS;
      const int r = i / CV, c = (i - r * CV) * 4;
      const int y = row_of(r), x = x0 + c;
      p[it] = make_float4(1.f, 1.f, 1.f, 1.f);
      g[it] = make_float4(nan, nan, nan, nan);
      if (i < NV && y >= 0 && y < H && x >= 0 && x < W) {
        const int64_t o = (int64_t)y * W + x;
        p[it] = *reinterpret_cast<const float4*>(P + o);
        g[it] = *reinterpret_cast<const float4*>(G + o);
      }
    }
#pragma unroll
    for (int it = 0; it < IT; ++it) {
      const int i = threadIdx.x + it * GM_THREADS;
      if (i < NV) {
        const uint4 v = make_uint4(gm_code(p[it].x, g[it].x, min_depth), gm_code(p[it].y, g[it].y, min_depth),
                                   gm_code(p[it].z, g[it].z, min_depth), gm_code(p[it].w, g[it].w, min_depth));
        *reinterpret_cast<uint4*>(tile + i * 4) = v;  // i * 4 == r * COLS + c
      }
    }
  } else {
    constexpr int NS = ROWS * COLS, CH = 8;  // 8 pixels per thread and phase pair
    for (int base = 0; base < NS; base += CH * GM_THREADS) {
      float p[CH], g[CH];
#pragma unroll
      for (int it = 0; it < CH; ++it) {
        const int i = base + threadIdx.x + it * GM_THREADS;
        const int r = i / COLS, c = i - r * COLS;
        const int y = row_of(r), x = x0 + c;
        p[it] = 1.f;
        g[it] = nan;
        if (i < NS && y >= 0 && y < H && x >= 0 && x < W) {
          const int64_t o = (int64_t)y * W + x;
          p[it] = P[o];
          g[it] = G[o];
        }
      }
#pragma unroll
      for (int it = 0; it < CH; ++it) {
        const int i = base + threadIdx.x + it * GM_THREADS;
        if (i < NS) tile[i] = gm_code(p[it], g[it], min_depth);
      }
    }
  }
}

// part[(b * nblk + block)][8] = {N_0..N_3, S_0..S_3} of the block's tile
template <bool VEC>
__global__ __launch_bounds__(GM_THREADS) void gm_fwd_kernel(const float* __restrict__ pred,
                                                            const float* __restrict__ gt, float* __restrict__ part,
                                                            int H, int W, float min_depth, int K) {
  constexpr int ROWS = GM_TH + 1, COLS = GM_TW + GM_RPAD;
  __shared__ __attribute__((aligned(16))) uint32_t tile[ROWS * COLS];
  __shared__ float red[GM_THREADS / 64][2 * GM_MAXK];
  const int y0 = blockIdx.y * GM_TH, x0 = blockIdx.x * GM_TW;
  const int64_t img = (int64_t)blockIdx.z * H * W;
  gm_fill<ROWS, COLS, VEC>(tile, pred + img, gt + img, H, W, x0, min_depth, [y0](int r) { return y0 + r; });
  __syncthreads();
  float n[GM_MAXK], s[GM_MAXK];
#pragma unroll
  for (int k = 0; k < GM_MAXK; ++k) {
    n[k] = 0.f; s[k] = 0.f;
    if (k < K) {
      constexpr int LOGW = 7;  // log2(GM_TW)
      static_assert((1 << LOGW) == GM_TW, "LOGW");
      const int st = 1 << k, gw = GM_TW >> k, cells = (GM_TH >> k) * gw;
      for (int i = threadIdx.x; i < cells; i += GM_THREADS) {  // the tile's scale-k grid, compacted
        const int cy = i >> (LOGW - k), cx = i & (gw - 1);
        const uint32_t* c = tile + (cy << k) * COLS + (cx << k);
        const uint32_t a = c[0];
        if (a != GM_INVALID) {
          const float ra = __uint_as_float(a);
          const uint32_t r = c[st], d = c[st * COLS];
          n[k] += 1.f;
          if (r != GM_INVALID) s[k] += fabsf(__uint_as_float(r) - ra);
          if (d != GM_INVALID) s[k] += fabsf(__uint_as_float(d) - ra);
        }
      }
    }
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < GM_MAXK; ++k) {
    const float nk = wave_sum(n[k]), sk = wave_sum(s[k]);
    if (lane == 0) { red[wid][k] = nk; red[wid][GM_MAXK + k] = sk; }
  }
  __syncthreads();
  if (threadIdx.x < 2 * GM_MAXK) {
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < GM_THREADS / 64; ++w) t += red[w][threadIdx.x];
    const int64_t blk = ((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    part[blk * (2 * GM_MAXK) + threadIdx.x] = t;
  }
}

// One block: each group's partials are summed by all threads in a fixed strided order, then a
// fixed fp64 tree through LDS (block_tree_sum, as silog_finalize).  Writes loss[0] and wk[b][k] = dL/dS_bk:
// per batch 1 / sum_b N_bk, per image 1 / (N_bk * images used); 0 for an empty or unused scale.
constexpr int GMF_THREADS = 256;
__global__ __launch_bounds__(GMF_THREADS) void gm_finalize(const float* __restrict__ part, int nblk, int B, int K,
                                                           int per_image, double* __restrict__ nd,
                                                           float* __restrict__ loss, float* __restrict__ wk) {
  __shared__ double red[2 * GM_MAXK][GMF_THREADS];
  __shared__ int used_s;
  const int t = threadIdx.x;
  const int G = per_image ? B : 1;
  double total = 0.0;
  int used = 0;
  for (int g = 0; g < G; ++g) {
    const int64_t j0 = per_image ? (int64_t)g * nblk : 0, j1 = per_image ? (int64_t)(g + 1) * nblk : (int64_t)B * nblk;
    double acc[2 * GM_MAXK];
#pragma unroll
    for (int q = 0; q < 2 * GM_MAXK; ++q) acc[q] = 0.0;
    for (int64_t j = j0 + t; j < j1; j += GMF_THREADS) {
      const float4 a = *reinterpret_cast<const float4*>(part + j * 8);
      const float4 b = *reinterpret_cast<const float4*>(part + j * 8 + 4);
      acc[0] += a.x; acc[1] += a.y; acc[2] += a.z; acc[3] += a.w;
      acc[4] += b.x; acc[5] += b.y; acc[6] += b.z; acc[7] += b.w;
    }
    block_tree_sum(acc, red);
    if (t == 0) {
      double lg = 0.0;
      for (int k = 0; k < GM_MAXK; ++k) {
        const double n = red[k][0];
        nd[g * GM_MAXK + k] = n;
        if (k < K && n > 0) lg += red[GM_MAXK + k][0] / n;
      }
      if (!per_image || red[0][0] > 0) { total += lg; ++used; }
    }
    __syncthreads();
  }
  if (t == 0) {
    used_s = used;
    loss[0] = per_image ? (used ? (float)(total / used) : 0.f) : (float)total;
  }
  __syncthreads();  // nd (thread 0's global stores) and used_s are visible to the block from here
  used = used_s;
  for (int i = t; i < B * GM_MAXK; i += GMF_THREADS) {
    const int b = i / GM_MAXK, k = i - b * GM_MAXK;
    double w = 0.0;
    if (k < K) {
      if (per_image) {
        const double n = nd[i], n0 = nd[b * GM_MAXK];
        if (n > 0 && n0 > 0) w = 1.0 / (n * used);
      } else {
        const double n = nd[k];
        if (n > 0) w = 1.0 / n;
      }
    }
    wk[i] = (float)w;
  }
}

__device__ __forceinline__ int gm_sign(float ra, uint32_t nb) {
  if (nb == GM_INVALID) return 0;
  const float d = ra - __uint_as_float(nb);
  return (d > 0.f) - (d < 0.f);
}

// LDS image of the backward: rows 0..3 hold image rows y0-8, y0-4, y0-2, y0-1 (the only rows above
// the tile a gather reaches: y - s < y0 happens at the tile's first row alone), rows 4.. the tile and
// one row below; columns start at x0 - 8.
constexpr int GMB_TOP = GM_MAXK, GMB_ROWS = GMB_TOP + GM_TH + 1, GMB_COLS = GM_HALO + GM_TW + GM_RPAD;

// sum_k w[k] * c_k of tile pixel (ly, lx); 0 off the mask
__device__ __forceinline__ float gm_pixel(const uint32_t* tile, int ly, int lx, int K, const float* w) {
  const uint32_t* c = tile + (GMB_TOP + ly) * GMB_COLS + GM_HALO + lx;
  const uint32_t a = c[0];
  if (a == GM_INVALID) return 0.f;
  const float ra = __uint_as_float(a);
  const int m = ly | lx;
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < GM_MAXK; ++k) {
    const int st = 1 << k;
    if (k >= K || (m & (st - 1))) break;  // not on the scale-k grid, nor on any coarser one
    const uint32_t* up = ly >= st ? c - st * GMB_COLS : tile + (GMB_TOP - 1 - k) * GMB_COLS + GM_HALO + lx;
    const int cnt = gm_sign(ra, c[st]) + gm_sign(ra, c[-st]) + gm_sign(ra, c[st * GMB_COLS]) + gm_sign(ra, up[0]);
    acc = fmaf(w[k], (float)cnt, acc);
  }
  return acc;
}

template <bool VEC>
__global__ __launch_bounds__(GM_THREADS) void gm_bwd_kernel(const float* __restrict__ pred,
                                                            const float* __restrict__ gt,
                                                            const float* __restrict__ wk,
                                                            const float* __restrict__ dloss,
                                                            float* __restrict__ dpred, int H, int W, float min_depth,
                                                            int K) {
  __shared__ __attribute__((aligned(16))) uint32_t tile[GMB_ROWS * GMB_COLS];
  const int b = blockIdx.z, y0 = blockIdx.y * GM_TH, x0 = blockIdx.x * GM_TW;
  const int64_t img = (int64_t)b * H * W;
  const float* P = pred + img;
  gm_fill<GMB_ROWS, GMB_COLS, VEC>(tile, P, gt + img, H, W, x0 - GM_HALO, min_depth, [y0](int r) {
    return r < GMB_TOP ? y0 - (GM_HALO >> r) : y0 + r - GMB_TOP;
  });
  float w[GM_MAXK];
  const float dl = dloss[0];
#pragma unroll
  for (int k = 0; k < GM_MAXK; ++k) w[k] = k < K ? wk[b * GM_MAXK + k] * dl : 0.f;
  __syncthreads();
  float* dP = dpred + img;
  if (VEC) {
    for (int i = threadIdx.x; i < GM_TH * GM_TW / 4; i += GM_THREADS) {
      const int ly = i / (GM_TW / 4), lx = (i - ly * (GM_TW / 4)) * 4;
      const int y = y0 + ly, x = x0 + lx;
      if (y >= H || x >= W) continue;
      const int64_t o = (int64_t)y * W + x;
      const float4 p = *reinterpret_cast<const float4*>(P + o);
      const float a0 = gm_pixel(tile, ly, lx, K, w), a1 = gm_pixel(tile, ly, lx + 1, K, w);
      const float a2 = gm_pixel(tile, ly, lx + 2, K, w), a3 = gm_pixel(tile, ly, lx + 3, K, w);
      float4 out;  // 0 on invalid pixels whatever pred holds there
      out.x = a0 != 0.f ? a0 / p.x : 0.f; out.y = a1 != 0.f ? a1 / p.y : 0.f;
      out.z = a2 != 0.f ? a2 / p.z : 0.f; out.w = a3 != 0.f ? a3 / p.w : 0.f;
      *reinterpret_cast<float4*>(dP + o) = out;
    }
  } else {
    for (int i = threadIdx.x; i < GM_TH * GM_TW; i += GM_THREADS) {
      const int ly = i / GM_TW, lx = i - ly * GM_TW;
      const int y = y0 + ly, x = x0 + lx;
      if (y >= H || x >= W) continue;
      const int64_t o = (int64_t)y * W + x;
      const float a = gm_pixel(tile, ly, lx, K, w);
      dP[o] = a != 0.f ? a / P[o] : 0.f;
    }
  }
}

static int64_t gm_tiles(int32_t H, int32_t W) { return cdiv(H, GM_TH) * cdiv(W, GM_TW); }
static bool gm_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static size_t gm_nd_bytes(int32_t B) { return align_up((size_t)B * GM_MAXK * sizeof(double), 16); }

}  // namespace mdemi

using namespace mdemi;

extern "C" size_t mdemi_gradmatch_workspace_size(int32_t B, int32_t H, int32_t W) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  return gm_nd_bytes(B) + (size_t)B * gm_tiles(H, W) * 2 * GM_MAXK * sizeof(float);
}

static int gm_check_geom(const char* what, int32_t B, int32_t H, int32_t W, int32_t scales) {
  MDEMI_REQUIRE(B > 0 && H > 0 && W > 0, "%s: bad args", what);
  MDEMI_REQUIRE(scales >= 1 && scales <= GM_MAXK, "%s: scales must be 1..%d, got %d", what, GM_MAXK, scales);
  MDEMI_REQUIRE(B <= 65535 && cdiv(H, GM_TH) <= 65535 && (int64_t)B * gm_tiles(H, W) < (1ll << 31),
                "%s: B=%d H=%d W=%d exceeds the launch grid", what, B, H, W);
  return MDEMI_OK;
}

extern "C" int mdemi_gradmatch_fwd(const float* pred, const float* gt, float* loss, float* wk, int32_t B, int32_t H,
                                   int32_t W, float min_depth, int32_t scales, int32_t per_image, void* workspace,
                                   void* stream) {
  MDEMI_REQUIRE(pred && gt && loss && wk, "gradmatch_fwd: bad args");
  if (int rc = gm_check_geom("gradmatch_fwd", B, H, W, scales)) return rc;
  if (!workspace) { set_error("gradmatch_fwd: workspace required"); return MDEMI_EWORKSPACE; }
  MDEMI_REQUIRE(gm_aligned16(workspace), "gradmatch_fwd: workspace must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  double* nd = (double*)workspace;
  float* part = (float*)((char*)workspace + gm_nd_bytes(B));
  const dim3 grid((unsigned)cdiv(W, GM_TW), (unsigned)cdiv(H, GM_TH), (unsigned)B);
  if (W % 4 == 0 && gm_aligned16(pred) && gm_aligned16(gt))
    hipLaunchKernelGGL(gm_fwd_kernel<true>, grid, dim3(GM_THREADS), 0, st, pred, gt, part, H, W, min_depth, scales);
  else
    hipLaunchKernelGGL(gm_fwd_kernel<false>, grid, dim3(GM_THREADS), 0, st, pred, gt, part, H, W, min_depth, scales);
  hipLaunchKernelGGL(gm_finalize, dim3(1), dim3(GMF_THREADS), 0, st, (const float*)part, (int)gm_tiles(H, W), B, scales,
                     per_image, nd, loss, wk);
  return check_launch("gradmatch_fwd");
}

extern "C" int mdemi_gradmatch_bwd(const float* pred, const float* gt, const float* wk, const float* dloss,
                                   float* dpred, int32_t B, int32_t H, int32_t W, float min_depth, int32_t scales,
                                   void* stream) {
  MDEMI_REQUIRE(pred && gt && wk && dloss && dpred, "gradmatch_bwd: bad args");
  if (int rc = gm_check_geom("gradmatch_bwd", B, H, W, scales)) return rc;
  const dim3 grid((unsigned)cdiv(W, GM_TW), (unsigned)cdiv(H, GM_TH), (unsigned)B);
  if (W % 4 == 0 && gm_aligned16(pred) && gm_aligned16(gt) && gm_aligned16(dpred))
    hipLaunchKernelGGL(gm_bwd_kernel<true>, grid, dim3(GM_THREADS), 0, (hipStream_t)stream, pred, gt, wk, dloss, dpred,
                       H, W, min_depth, scales);
  else
    hipLaunchKernelGGL(gm_bwd_kernel<false>, grid, dim3(GM_THREADS), 0, (hipStream_t)stream, pred, gt, wk, dloss,
                       dpred, H, W, min_depth, scales);
  return check_launch("gradmatch_bwd");
}
