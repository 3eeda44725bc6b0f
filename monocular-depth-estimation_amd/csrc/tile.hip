// Tiled inference (cfg eval.tile): cut an image batch into overlapping tiles, and
// merge the tiles' depth predictions back into one map.
//   extract: img [B][C][H][W] -> out [B*T][C][th][tw], a bit-exact copy in one launch.
//   blend:   out(y, x) = (float)(sum_k w_k q_k / sum_k w_k) over the covering tiles in ascending
//     k = iy * nx + ix, all in fp64 and rounded once; w = wy * wx with the ramp
//     wy(u) = min(u + 1, th - u, max(1, oy)).  A gather: per output pixel a loop over the covering
//     tile rows x columns, so there is no canvas, no atomic and the order is fixed.
//   align:   for affine-invariant predictions.  Tile 0 is the anchor; tile k = 1 .. T-1 in turn is
//     fitted (s_k, t_k) to the blend of the aligned tiles j < k over the pixels they share with it:
//     one statistics kernel over tile k's rectangle (per-chunk fp64 partials of n, Sx, Sy, Sxx,
//     Sxy), one one-wave-per-image solve that writes coef[b][k] for the next step to read.
// The plan (origins, sizes) travels in the kernel arguments: no device table, every call capturable.
#include "common.h"
#include "image_reduce.h"
#include "mdemi_ext.h"

namespace mdemi {

constexpr int TL_N = 5;          // n, Sx, Sy, Sxx, Sxy
constexpr int TL_CHUNK = 1024;   // pixels of a tile per statistics block (4 per thread)
constexpr int TL_MAX_CHUNKS = 512;

struct TilePlan {
  int H, W, th, tw, ny, nx;
  int ry, rx;  // the ramps' caps: max(1, overlap)
  int ys[MDEMI_TILE_MAX_AXIS], xs[MDEMI_TILE_MAX_AXIS];
};

__device__ __forceinline__ double ramp(int u, int n, int cap) { return (double)min(min(u + 1, n - u), cap); }

// q of DESIGN §1c: the tile's value in the frame of tile 0.  MODE 0 none, 1 lstsq, 2 lstsq_disp
template <int MODE>
__device__ __forceinline__ double tile_q(float p, double s, double t) {
  if (MODE == 0) return (double)p;
  return s * lsq_operand<MODE == 2>(p) + t;
}

// ---- extract -----------------------------------------------------------------------------------
struct ExtractArgs {
  const float* img;
  float* out;
  TilePlan p;
  int C;
  int vec_out;       // out 16-byte aligned and tw % 4 == 0
  uint32_t vec_col;  // bit ix: tile column ix reads whole aligned float4s (img, W, xs[ix], tw)
};

// grid (blocks over th * ceil(tw / 4), T * C, B): four consecutive pixels of a tile row per thread
__global__ __launch_bounds__(256) void tile_extract_kernel(ExtractArgs a) {
  const TilePlan& p = a.p;
  const int gw = (p.tw + 3) >> 2;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= p.th * gw) return;
  const int u = idx / gw, v = (idx - u * gw) * 4;
  const int k = blockIdx.y / a.C, c = blockIdx.y - k * a.C, b = blockIdx.z;
  const int iy = k / p.nx, ix = k - iy * p.nx;
  const int T = p.ny * p.nx;
  const float* src = a.img + (((int64_t)b * a.C + c) * p.H + p.ys[iy] + u) * p.W + p.xs[ix] + v;
  float* dst = a.out + ((((int64_t)b * T + k) * a.C + c) * p.th + u) * p.tw + v;
  const int cnt = min(4, p.tw - v);
  float d[4];
  if ((a.vec_col >> ix) & 1u) {
    const float4 q = *reinterpret_cast<const float4*>(src);
    d[0] = q.x; d[1] = q.y; d[2] = q.z; d[3] = q.w;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) d[i] = i < cnt ? src[i] : 0.f;
  }
  if (a.vec_out) *reinterpret_cast<float4*>(dst) = make_float4(d[0], d[1], d[2], d[3]);
  else
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < cnt) dst[i] = d[i];
}

// ---- blend -------------------------------------------------------------------------------------
struct BlendArgs {
  const float* tiles;  // [B*T][th][tw]
  const double* coef;  // [B][T][4], unused in MODE 0
  float* out;          // [B][H][W]
  TilePlan p;
  double floor_disp;  // 1 / max_depth
  int vec_tile;       // tiles 16-byte aligned and tw % 4 == 0
  int vec_out;        // out 16-byte aligned and W % 4 == 0
};

// grid (blocks over H * ceil(W / 4), B): four consecutive pixels of an output row per thread
template <int MODE>
__global__ __launch_bounds__(256) void tile_blend_kernel(BlendArgs a) {
  const TilePlan& p = a.p;
  const int gW = (p.W + 3) >> 2;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= p.H * gW) return;
  const int b = blockIdx.y, y = idx / gW, x = (idx - y * gW) * 4;
  const int T = p.ny * p.nx;
  double num[4] = {0.0, 0.0, 0.0, 0.0}, den[4] = {0.0, 0.0, 0.0, 0.0};
  for (int iy = 0; iy < p.ny; ++iy) {
    const int u = y - p.ys[iy];
    if (u < 0) break;  // origins ascend
    if (u >= p.th) continue;
    const double wy = ramp(u, p.th, p.ry);
    for (int ix = 0; ix < p.nx; ++ix) {
      const int v = x - p.xs[ix];
      if (v + 3 < 0) break;
      if (v >= p.tw) continue;
      const int64_t bk = (int64_t)b * T + iy * p.nx + ix;
      const float* row = a.tiles + (bk * p.th + u) * p.tw;
      double s = 1.0, t = 0.0;
      if (MODE != 0) {
        s = a.coef[bk * 4 + 0];
        t = a.coef[bk * 4 + 1];
      }
      float pv[4];
      if (a.vec_tile && (v & 3) == 0 && v >= 0 && v + 3 < p.tw) {
        const float4 q = *reinterpret_cast<const float4*>(row + v);
        pv[0] = q.x; pv[1] = q.y; pv[2] = q.z; pv[3] = q.w;
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) pv[i] = (v + i >= 0 && v + i < p.tw) ? row[v + i] : 0.f;
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (v + i < 0 || v + i >= p.tw) continue;  // also x + i >= W: every tile ends inside the image
        const double w = wy * ramp(v + i, p.tw, p.rx);
        num[i] += w * tile_q<MODE>(pv[i], s, t);
        den[i] += w;
      }
    }
  }
  float r[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    double q = num[i] / den[i];
    if (MODE == 2) q = 1.0 / (q < a.floor_disp ? a.floor_disp : q);  // a NaN stays a NaN
    r[i] = (float)q;
  }
  float* dst = a.out + ((int64_t)b * p.H + y) * p.W + x;
  if (a.vec_out) *reinterpret_cast<float4*>(dst) = make_float4(r[0], r[1], r[2], r[3]);
  else
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (x + i < p.W) dst[i] = r[i];
}

// ---- align -------------------------------------------------------------------------------------
// coef[b][k] = s 1, t 0, n 0, status 0 on every tile: the anchor's row, and a defined value for all
__global__ void tile_coef_init(double* __restrict__ coef, int rows) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows) return;
  coef[i * 4 + 0] = 1.0;
  coef[i * 4 + 1] = 0.0;
  coef[i * 4 + 2] = 0.0;
  coef[i * 4 + 3] = 0.0;
}

// part[b][chunk][5] over the chunk's pixels of tile k that a tile j < k covers: x = op(p_k),
// y = the blend of the aligned tiles j < k.  grid (nchunk, B).
template <bool DISP>
__global__ __launch_bounds__(256) void tile_align_partial(const float* __restrict__ tiles,
                                                          const double* __restrict__ coef, double* __restrict__ part,
                                                          TilePlan p, int k, int nchunk) {
  constexpr int MODE = DISP ? 2 : 1;
  const int b = blockIdx.y, T = p.ny * p.nx;
  const int ky = k / p.nx, kx = k - ky * p.nx;
  const int npix = p.th * p.tw, per = (npix + nchunk - 1) / nchunk;
  const int p0 = blockIdx.x * per, p1 = min(npix, p0 + per);
  const float* mine = tiles + ((int64_t)b * T + k) * npix;
  double acc[TL_N];
#pragma unroll
  for (int i = 0; i < TL_N; ++i) acc[i] = 0.0;
  for (int q = p0 + threadIdx.x; q < p1; q += 256) {
    const int u = q / p.tw, v = q - u * p.tw;
    const int y = p.ys[ky] + u, x = p.xs[kx] + v;
    double num = 0.0, den = 0.0;
    for (int jy = 0; jy <= ky; ++jy) {
      const int uu = y - p.ys[jy];
      if (uu >= p.th) continue;  // uu >= 0: ys[jy] <= ys[ky]
      const double wy = ramp(uu, p.th, p.ry);
      const int jx_end = jy == ky ? kx : p.nx;  // j < k in raster order
      for (int jx = 0; jx < jx_end; ++jx) {
        const int vv = x - p.xs[jx];
        if (vv < 0) break;
        if (vv >= p.tw) continue;
        const int64_t bj = (int64_t)b * T + jy * p.nx + jx;
        const double w = wy * ramp(vv, p.tw, p.rx);
        num += w * tile_q<MODE>(tiles[(bj * p.th + uu) * p.tw + vv], coef[bj * 4 + 0], coef[bj * 4 + 1]);
        den += w;
      }
    }
    if (!(den > 0.0)) continue;
    const float pk = mine[q];
    if (DISP && !(pk > 0.f)) continue;
    const double xv = lsq_operand<DISP>(pk), yv = num / den;
    if (!isfinite(xv) || !isfinite(yv)) continue;
    acc[0] += 1.0;
    acc[1] += xv;
    acc[2] += yv;
    acc[3] += xv * xv;
    acc[4] += xv * yv;
  }
  block_store_pairwise(acc, part + ((int64_t)b * nchunk + blockIdx.x) * TL_N);
}

// one wave per image: the chunks' sums, the fit, the failure rule
__global__ __launch_bounds__(64) void tile_align_solve(const double* __restrict__ part, double* __restrict__ coef,
                                                       int T, int k, int nchunk) {
  const int b = blockIdx.x;
  double m[TL_N];
  chunk_sums_strided(part + (int64_t)b * nchunk * TL_N, nchunk, m);
  if (threadIdx.x != 0) return;
  const LsqFit f = lsq_fit(m[0], m[1], m[2], m[3], m[4]);
  const bool ok = m[0] >= 2.0 && isfinite(f.det) && f.det > 0.0 && f.s > 0.0;
  double* c = coef + ((int64_t)b * T + k) * 4;
  c[0] = ok ? f.s : 1.0;
  c[1] = ok ? f.t : 0.0;
  c[2] = m[0];
  c[3] = ok ? 0.0 : 1.0;
}

// ---- host --------------------------------------------------------------------------------------
static const char* plan_error(int H, int W, int th, int tw, int oy, int ox, const int32_t* ys, int ny,
                              const int32_t* xs, int nx, bool cover) {
  if (H <= 0 || W <= 0 || (int64_t)H * W > 0x7FFFFFFF) return "H, W must be positive with H * W < 2^31";
  if (th <= 0 || th > H || tw <= 0 || tw > W) return "the tile must be inside the image";
  if (oy < 0 || oy >= th || ox < 0 || ox >= tw) return "the overlap must be in [0, tile)";
  if (!ys || !xs) return "null origin list";
  if (ny < 1 || ny > MDEMI_TILE_MAX_AXIS || nx < 1 || nx > MDEMI_TILE_MAX_AXIS) return "ny, nx must be in 1..32";
  for (int axis = 0; axis < 2; ++axis) {
    const int32_t* o = axis ? xs : ys;
    const int n = axis ? nx : ny, size = axis ? W : H, t = axis ? tw : th;
    for (int i = 0; i < n; ++i) {
      if (o[i] < 0 || o[i] > size - t) return "a tile origin is outside the image";
      if (i && o[i] <= o[i - 1]) return "tile origins must ascend";
      if (cover && i && o[i] - o[i - 1] > t) return "the tiles leave a gap";
    }
    if (cover && (o[0] != 0 || o[n - 1] != size - t)) return "the tiles do not reach the image's border";
  }
  return nullptr;
}

static TilePlan make_plan(int H, int W, int th, int tw, int oy, int ox, const int32_t* ys, int ny, const int32_t* xs,
                          int nx) {
  TilePlan p{};
  p.H = H; p.W = W; p.th = th; p.tw = tw; p.ny = ny; p.nx = nx;
  p.ry = oy > 1 ? oy : 1;
  p.rx = ox > 1 ? ox : 1;
  for (int i = 0; i < ny; ++i) p.ys[i] = ys[i];
  for (int i = 0; i < nx; ++i) p.xs[i] = xs[i];
  return p;
}

static int tile_chunks(int th, int tw) {
  const int64_t c = cdiv((int64_t)th * tw, TL_CHUNK);
  return (int)(c > TL_MAX_CHUNKS ? TL_MAX_CHUNKS : c);
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace mdemi

using namespace mdemi;

extern "C" int mdemi_tile_extract(const float* img, float* out, int32_t B, int32_t C, int32_t H, int32_t W, int32_t th,
                                  int32_t tw, const int32_t* ys, int32_t ny, const int32_t* xs, int32_t nx,
                                  void* stream) {
  MDEMI_REQUIRE(img && out && B > 0 && B <= 65535 && C > 0, "tile_extract: bad args");
  MDEMI_REQUIRE((((uintptr_t)img | (uintptr_t)out) & 3) == 0, "tile_extract: misaligned pointer");
  const char* err = plan_error(H, W, th, tw, 0, 0, ys, ny, xs, nx, false);
  MDEMI_REQUIRE(!err, "tile_extract: %s", err);
  MDEMI_REQUIRE((int64_t)ny * nx * C <= 65535, "tile_extract: tiles x channels must be at most 65535");
  ExtractArgs a;
  a.img = img;
  a.out = out;
  a.p = make_plan(H, W, th, tw, 0, 0, ys, ny, xs, nx);
  a.C = C;
  a.vec_out = aligned16(out) && tw % 4 == 0;
  a.vec_col = 0;
  if (aligned16(img) && W % 4 == 0 && tw % 4 == 0)
    for (int i = 0; i < nx; ++i)
      if (xs[i] % 4 == 0) a.vec_col |= 1u << i;
  const dim3 grid((unsigned)cdiv((int64_t)th * cdiv(tw, 4), 256), (unsigned)(ny * nx * C), (unsigned)B);
  hipLaunchKernelGGL(tile_extract_kernel, grid, dim3(256), 0, (hipStream_t)stream, a);
  return check_launch("tile_extract");
}

extern "C" size_t mdemi_tile_align_workspace_size(int32_t B, int32_t th, int32_t tw) {
  if (B <= 0 || th <= 0 || tw <= 0) return 0;
  return align_up((size_t)B * tile_chunks(th, tw) * TL_N * sizeof(double), 256);
}

extern "C" int mdemi_tile_align(const float* tiles, int32_t B, int32_t H, int32_t W, int32_t th, int32_t tw, int32_t oy,
                                int32_t ox, const int32_t* ys, int32_t ny, const int32_t* xs, int32_t nx, int32_t mode,
                                double* coef, void* workspace, void* stream) {
  MDEMI_REQUIRE(tiles && coef && B > 0 && B <= 65535, "tile_align: bad args");
  MDEMI_REQUIRE(((uintptr_t)tiles & 3) == 0 && ((uintptr_t)coef & 7) == 0, "tile_align: misaligned pointer");
  MDEMI_REQUIRE(mode == MDEMI_ALIGN_LSTSQ || mode == MDEMI_ALIGN_LSTSQ_DISP,
                "tile_align: mode must be 2 (lstsq) or 3 (lstsq_disp), got %d", mode);
  const char* err = plan_error(H, W, th, tw, oy, ox, ys, ny, xs, nx, true);
  MDEMI_REQUIRE(!err, "tile_align: %s", err);
  MDEMI_REQUIRE((ny == 1 || oy > 0) && (nx == 1 || ox > 0), "tile_align: an axis with several tiles needs an overlap");
  if (!workspace) { set_error("tile_align: workspace required"); return MDEMI_EWORKSPACE; }
  MDEMI_REQUIRE(((uintptr_t)workspace & 7) == 0, "tile_align: workspace must be 8-byte aligned");
  const TilePlan p = make_plan(H, W, th, tw, oy, ox, ys, ny, xs, nx);
  const int T = ny * nx, nchunk = tile_chunks(th, tw);
  hipStream_t st = (hipStream_t)stream;
  double* part = (double*)workspace;
  hipLaunchKernelGGL(tile_coef_init, dim3((unsigned)cdiv((int64_t)B * T, 256)), dim3(256), 0, st, coef, B * T);
  for (int k = 1; k < T; ++k) {
    if (mode == MDEMI_ALIGN_LSTSQ_DISP)
      hipLaunchKernelGGL(tile_align_partial<true>, dim3(nchunk, B), dim3(256), 0, st, tiles, (const double*)coef, part,
                         p, k, nchunk);
    else
      hipLaunchKernelGGL(tile_align_partial<false>, dim3(nchunk, B), dim3(256), 0, st, tiles, (const double*)coef, part,
                         p, k, nchunk);
    hipLaunchKernelGGL(tile_align_solve, dim3(B), dim3(64), 0, st, (const double*)part, coef, T, k, nchunk);
  }
  return check_launch("tile_align");
}

extern "C" int mdemi_tile_blend(const float* tiles, const double* coef, int32_t B, int32_t H, int32_t W, int32_t th,
                                int32_t tw, int32_t oy, int32_t ox, const int32_t* ys, int32_t ny, const int32_t* xs,
                                int32_t nx, int32_t mode, float max_depth, float* out, void* stream) {
  MDEMI_REQUIRE(tiles && out && B > 0 && B <= 65535, "tile_blend: bad args");
  MDEMI_REQUIRE((((uintptr_t)tiles | (uintptr_t)out) & 3) == 0 && ((uintptr_t)coef & 7) == 0,
                "tile_blend: misaligned pointer");
  MDEMI_REQUIRE(mode == MDEMI_TILE_NONE || mode == MDEMI_ALIGN_LSTSQ || mode == MDEMI_ALIGN_LSTSQ_DISP,
                "tile_blend: mode must be 0 (none), 2 (lstsq) or 3 (lstsq_disp), got %d", mode);
  MDEMI_REQUIRE(mode == MDEMI_TILE_NONE || coef, "tile_blend: an aligned mode needs coef");
  MDEMI_REQUIRE(mode != MDEMI_ALIGN_LSTSQ_DISP || max_depth > 0.f, "tile_blend: lstsq_disp needs max_depth > 0");
  const char* err = plan_error(H, W, th, tw, oy, ox, ys, ny, xs, nx, true);
  MDEMI_REQUIRE(!err, "tile_blend: %s", err);
  BlendArgs a;
  a.tiles = tiles;
  a.coef = coef;
  a.out = out;
  a.p = make_plan(H, W, th, tw, oy, ox, ys, ny, xs, nx);
  a.floor_disp = mode == MDEMI_ALIGN_LSTSQ_DISP ? 1.0 / (double)max_depth : 0.0;
  a.vec_tile = aligned16(tiles) && tw % 4 == 0;
  a.vec_out = aligned16(out) && W % 4 == 0;
  const dim3 grid((unsigned)cdiv((int64_t)H * cdiv(W, 4), 256), (unsigned)B);
  hipStream_t st = (hipStream_t)stream;
  if (mode == MDEMI_TILE_NONE) hipLaunchKernelGGL(tile_blend_kernel<0>, grid, dim3(256), 0, st, a);
  else if (mode == MDEMI_ALIGN_LSTSQ) hipLaunchKernelGGL(tile_blend_kernel<1>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(tile_blend_kernel<2>, grid, dim3(256), 0, st, a);
  return check_launch("tile_blend");
}
