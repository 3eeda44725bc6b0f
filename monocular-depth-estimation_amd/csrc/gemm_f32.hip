// fp32 GEMM on gfx950 MFMA (v_mfma_f32_32x32x2_f32: exact f32 products,
// f32 accumulate, 64 FLOP/clk/SIMD = the chip's 157 TF fp32 matrix peak).
//
// One kernel family serves every dense contraction of the hot path:
//   nn.Linear fwd / dgrad / wgrad   (swin_transformer.py:18-20,104,106,259;
//                                     newcrf_layers.py:16-20,102,104; ...)
//   nn.Conv2d fwd / dgrad / wgrad   through an implicit-im2col operand
//                                     (newcrf_layers.py:384,389;
//                                      uper_crf_head.py:38-44,341-348; ...)
// Operand element (i,k) of A / (k,j) of B is produced by a loader selected at
// compile time (dense k-contiguous, dense m/n-contiguous, or NHWC conv gather)
// with an optional GELU transform on load (so nn.GELU's output is never
// materialised: fc2 reads GELU(fc1 pre-activation) directly).  The epilogue
// fuses alpha/beta, bias, activation (or GELU-backward multiply) and a
// residual add.  Long reductions (weight gradients over B*H*W rows) split K
// over workgroups into fp32 slabs reduced by a second deterministic kernel.
//
// Tiling: 128x128 block tile, BK = 16, 256 threads = 4 waves in 2x2, each wave
// 64x64 = 2x2 MFMA 32x32 accumulators.  MFMA k-step s of a K tile takes, in
// lane half h, k = 8*(s/4) + 4*h + (s%4).  Both operands are staged in LDS as
// [k][row] images read with ds_read_b32 (32 consecutive floats per half-wave,
// conflict-free): M/N-contiguous sources are written as float4 rows (pitch
// 132), k-contiguous sources are transposed on the way in (4x ds_write_b32,
// pitch 130).  Register-staged prefetch of the next K tile (issue early, write
// late) into the second of two LDS buffers, one barrier per tile.  Block ids
// are remapped so that the tiles an XCD runs concurrently share A row-panels
// and B column-panels in that XCD's L2 (guide T1).  Variants: F32_VARIANTS (gemm_plan.h).
#include "common.h"
#include "gemm_core.h"
#include "gemm_f32_kernel.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <mutex>
#include <tuple>

namespace mdemi {

// Deterministic split-K combine + epilogue: sums slabs in split order, four
// consecutive columns per thread when N % 4 == 0; also folds the row-sum
// partials [split][M] of a weight-gradient GEMM (bias gradient) in the same launch.
__global__ __launch_bounds__(256) void gemm_splitk_reduce(GemmParams p, const float* __restrict__ rs_part,
                                                          float* __restrict__ rs_out) {
  const int64_t MN = (int64_t)(p.M - p.m_split) * p.N;  // the split rows [m_split, M)
  const bool quad = (p.N & 3) == 0;
  const int64_t units = quad ? MN / 4 : MN;
  const int64_t total = units * p.batch;
  const int64_t slab_stride = (int64_t)p.batch * MN;
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, gstride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t e = gid; e < total; e += gstride) {
    const int b = (int)(e / units);
    const int64_t u = e - (int64_t)b * units;
    const int64_t rem = quad ? 4 * u : u;
    const int i = (int)(rem / p.N) + p.m_split, j = (int)(rem - (int64_t)(i - p.m_split) * p.N);
    const float* src = p.slab + (int64_t)b * MN + rem;
    float* dst = p.C + boff(p, b, p.c_bs, p.c_bs2) + (int64_t)i * p.ldc + j;
    __bf16* dst16 = p.c16 ? reinterpret_cast<__bf16*>(p.c16) + (dst - p.C) : nullptr;  // C's layout
    if (quad) {
      float4 acc = *reinterpret_cast<const float4*>(src);
      for (int q = 1; q < p.split; ++q) {
        const float4 t = *reinterpret_cast<const float4*>(src + q * slab_stride);
        acc.x += t.x; acc.y += t.y; acc.z += t.z; acc.w += t.w;
      }
      const float v[4] = {epilogue_value(p, b, i, j, acc.x), epilogue_value(p, b, i, j + 1, acc.y),
                          epilogue_value(p, b, i, j + 2, acc.z), epilogue_value(p, b, i, j + 3, acc.w)};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        dst[e] = v[e];
        if (dst16) dst16[e] = (__bf16)v[e];
      }
    } else {
      float acc = src[0];
      for (int q = 1; q < p.split; ++q) acc += src[q * slab_stride];
      const float v = epilogue_value(p, b, i, j, acc);
      dst[0] = v;
      if (dst16) dst16[0] = (__bf16)v;
    }
  }
  if (rs_part)
    for (int64_t i = gid; i < p.M; i += gstride) {
      float acc = rs_part[i];
      for (int q = 1; q < p.split; ++q) acc += rs_part[(int64_t)q * p.M + i];
      rs_out[i] = acc;
    }
}

static int g_variant = -1;  // -1: autotune per shape
// A/B switches (environment, read once): MDEMI_GEMM_TAIL_SPLIT=0 disables the tail split;
// MDEMI_GEMM_INLINE_REDUCE=1 (fp32) / MDEMI_GEMM_INLINE_REDUCE_B16=1 (bf16) combine split-K
// slabs in the kernel (the tile's last-arriving workgroup) instead of the separate reduce
// kernel.  The separate, chip-wide reduce is the default since round 6: one last arriver
// reading every other slab of its tile serialises on a workgroup's fetch rate (~32 GB/s:
// profiles/round6/b16_variants_*.txt), which the bf16 step's small-grid weight gradients
// hit hardest -- configs[4] 145.5 -> 152.2 img/s, NYU 60.2 -> 60.8, AdaBins 73.6 -> 73.9 on
// one box (profiles/round6/ab_inline_reduce.txt).  The tail split always combines inline.
static bool env_on(const char* name) {
  const char* v = getenv(name);
  return !(v && v[0] == '0');
}
static bool env_set(const char* name) {
  const char* v = getenv(name);
  return v && v[0] && v[0] != '0';
}
static GemmOptions g_opt{env_on("MDEMI_GEMM_TAIL_SPLIT"), 8};  // tail split; raster group_m
static bool g_inline_reduce = env_set("MDEMI_GEMM_INLINE_REDUCE");
static bool g_inline_reduce_b16 = env_set("MDEMI_GEMM_INLINE_REDUCE_B16");
static int g_variant_m16 = -1;  // 16-bit family (bf16 / split fp32)
static int g_variant_b16 = -1;  // bf16-operand family

KernelFn f32_pick_part0(int al, int bl, int aop, int bop, int v);
KernelFn f32_pick_part1(int al, int bl, int aop, int bop, int v);
KernelFn f32_pick_part2(int al, int bl, int aop, int bop, int v);
KernelFn f32_pick_part3(int al, int bl, int aop, int bop, int v);

KernelFn glds_pick_part0(int al, int bl, int v);
KernelFn glds_pick_part1(int al, int bl, int v);

static KernelFn pick_kernel(int al, int bl, int aop, int bop, int v) {
  if (F32_VARIANTS[v].dma) {  // direct-to-LDS variants: dense operands without a load-time op
    if (aop != MDEMI_OP_NONE || bop != MDEMI_OP_NONE) return nullptr;
    if (KernelFn f = glds_pick_part0(al, bl, v)) return f;
    return glds_pick_part1(al, bl, v);
  }
  if (KernelFn f = f32_pick_part0(al, bl, aop, bop, v)) return f;
  if (KernelFn f = f32_pick_part1(al, bl, aop, bop, v)) return f;
  if (KernelFn f = f32_pick_part2(al, bl, aop, bop, v)) return f;
  return f32_pick_part3(al, bl, aop, bop, v);
}

static int validate(const mdemi_gemm_desc* d) {
  MDEMI_REQUIRE(d, "gemm: null descriptor");
  MDEMI_REQUIRE(d->M > 0 && d->N > 0 && d->K > 0 && d->batch > 0, "gemm: bad sizes M=%d N=%d K=%d batch=%d",
                d->M, d->N, d->K, d->batch);
  MDEMI_REQUIRE(d->A && d->B && d->C, "gemm: null operand");
  MDEMI_REQUIRE(d->split_k >= 1, "gemm: split_k must be >= 1");
  if (d->a_layout == MDEMI_L_CONV || d->b_layout == MDEMI_L_CONV) {
    const mdemi_conv_geom& g = d->conv;
    MDEMI_REQUIRE(g.c % 4 == 0, "gemm: conv operand needs C %% 4 == 0 (C=%d)", g.c);
    MDEMI_REQUIRE(g.kh > 0 && g.kw > 0 && g.stride > 0 && g.pad > -1024 && g.oh > 0 && g.ow > 0,
                  "gemm: bad conv geometry");
    const int64_t pixels = (int64_t)g.n * g.oh * g.ow;
    const int64_t taps = (int64_t)g.kh * g.kw * g.c;
    if (d->a_layout == MDEMI_L_CONV)
      MDEMI_REQUIRE(d->M == pixels && d->K == taps, "gemm: conv A needs M=N*OH*OW and K=KH*KW*C");
    if (d->b_layout == MDEMI_L_CONV)
      MDEMI_REQUIRE(d->K == pixels && d->N == taps && d->N % 4 == 0,
                    "gemm: conv B needs K=N*OH*OW and N=KH*KW*C");
    MDEMI_REQUIRE(al16(d->a_layout == MDEMI_L_CONV ? d->A : d->B), "gemm: conv operand must be 16-B aligned");
  }
  MDEMI_REQUIRE(d->bias_mode == MDEMI_BIAS_NONE || d->bias, "gemm: bias pointer missing");
  MDEMI_REQUIRE(!d->rowsum_a || (d->a_layout == MDEMI_L_MNCONTIG && d->batch == 1),
                "gemm: rowsum_a needs an m-contiguous A and batch 1");
  if (d->rowsum_a) MDEMI_REQUIRE(d->rowsum_a != d->C, "gemm: rowsum_a must not alias C");
  if (d->row_scale)
    MDEMI_REQUIRE(d->batch == 1 && d->row_scale_group > 0 && d->row_scale_group < ((int64_t)1 << 31),
                  "gemm: row_scale needs batch 1 and 0 < row_scale_group < 2^31");
  if (d->m_live || d->k_live)
    MDEMI_REQUIRE(d->batch == 1 && d->a_layout != MDEMI_L_CONV && d->b_layout != MDEMI_L_CONV,
                  "gemm: m_live / k_live need batch 1 and no conv operand");
  if (d->m_live)
    MDEMI_REQUIRE(d->m_live_group > 0 && d->m_live_group < ((int64_t)1 << 31) && !d->rowsum_a,
                  "gemm: m_live needs 0 < m_live_group < 2^31 and no rowsum_a");
  if (d->k_live)
    MDEMI_REQUIRE(d->k_live_group > 0 && d->k_live_group < ((int64_t)1 << 31),
                  "gemm: k_live needs 0 < k_live_group < 2^31");
  if (d->batch_inner > 1)
    MDEMI_REQUIRE(d->batch % d->batch_inner == 0 && !d->aux && !d->residual && !d->preact && !d->rowsum_a,
                  "gemm: batch_inner needs batch %% batch_inner == 0 and no aux/residual/preact/rowsum_a");
  // tile-relative 32-bit buffer offsets: 128 rows (or 16 k-rows) of any leading dimension
  const int64_t lim = (int64_t)1 << 21;
  MDEMI_REQUIRE(d->lda < lim && d->ldb < lim && d->ldc < lim && d->ldaux < lim && d->ldres < lim &&
                    d->ldpre < lim, "gemm: leading dimension too large for 32-bit tile offsets");
  if (d->split_k > 1)
    MDEMI_REQUIRE(d->N < lim, "gemm: N too large for split-K slabs");
  MDEMI_REQUIRE(!(d->act == MDEMI_ACT_GELU_GRAD || d->act == MDEMI_ACT_RELU_GRAD || d->act == MDEMI_ACT_SILU_GRAD) ||
                    d->aux, "gemm: *_GRAD epilogue needs aux");
  return MDEMI_OK;
}

static int device_cus() {
  static int cus[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  if (!cus[dev]) {
    hipDeviceProp_t pr;
    cus[dev] = hipGetDeviceProperties(&pr, dev) == hipSuccess && pr.multiProcessorCount > 0 ? pr.multiProcessorCount
                                                                                           : 256;
  }
  return cus[dev];
}

static void fill_params(const mdemi_gemm_desc* d, const GemmPlan& pl, GemmParams& p) {
  p.M = d->M; p.N = d->N; p.K = d->K; p.batch = d->batch;
  p.A = d->A; p.lda = d->lda; p.a_bs = d->a_bstride;
  p.B = d->B; p.ldb = d->ldb; p.b_bs = d->b_bstride;
  p.C = d->C; p.ldc = d->ldc; p.c_bs = d->c_bstride;
  p.alpha = d->alpha; p.beta = d->beta;
  p.bias = d->bias; p.bias_mode = d->bias_mode; p.act = d->act;
  p.aux = d->aux; p.ldaux = d->ldaux; p.aux_bs = d->aux_bstride;
  p.res = d->residual; p.ldres = d->ldres; p.res_bs = d->res_bstride;
  p.cv = d->conv;
  p.pre = d->preact; p.ldpre = d->ldpre; p.pre_bs = d->pre_bstride;
  p.rowsum = d->rowsum_a;
  p.rowscale = d->row_scale;
  if (d->row_scale) p.fd_rs = make_fastdiv((uint32_t)d->row_scale_group);
  p.m_live = d->m_live; p.k_live = d->k_live;
  if (d->m_live) p.fd_mlive = make_fastdiv((uint32_t)d->m_live_group);
  if (d->k_live) p.fd_klive = make_fastdiv((uint32_t)d->k_live_group);
  p.binner = d->batch_inner > 1 ? d->batch_inner : 1;
  p.a_bs2 = p.binner > 1 ? d->a_bstride_inner : 0;
  p.b_bs2 = p.binner > 1 ? d->b_bstride_inner : 0;
  p.c_bs2 = p.binner > 1 ? d->c_bstride_inner : 0;
  p.split = pl.split; p.ktile_per_split = pl.ktile_per_split; p.m_split = pl.m_split;
  p.tiles_m1 = pl.tiles_m1; p.tiles_m = pl.tiles_m; p.tiles_n = pl.tiles_n; p.group_m = pl.group_m;
  p.slab = nullptr; p.tile_cnt = nullptr; p.rowsum_out = nullptr; p.c16 = nullptr;
  p.a_vec = a_vec(d); p.b_vec = b_vec(d);
  if (d->a_layout == MDEMI_L_CONV || d->b_layout == MDEMI_L_CONV) {
    const mdemi_conv_geom& g = d->conv;
    p.fd_c = make_fastdiv(g.c); p.fd_kw = make_fastdiv(g.kw);
    p.fd_ow = make_fastdiv(g.ow); p.fd_oh = make_fastdiv(g.oh);
  }
}

}  // namespace mdemi

using namespace mdemi;

// Per-device split-tile counters for the in-kernel slab combine: zeroed once on the
// launch stream, left zeroed by every launch (the last arriver resets its tile's slot).
// GEMMs with split tiles on two streams at once would share them: the library runs its
// GEMMs on one compute stream.  None is allocated during a graph capture (nullptr: the
// launch falls back to the reduce kernel); a grown buffer keeps the old one alive for
// graphs that recorded it.
static int* tile_counters(int64_t n, hipStream_t st) {
  static std::mutex mu;
  static std::map<int, std::pair<int*, int64_t>> bufs;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  std::lock_guard<std::mutex> lk(mu);
  auto& e = bufs[dev];
  if (e.second >= n) return e.first;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return nullptr;
  const int64_t cap = std::max<int64_t>(n, (int64_t)1 << 16);
  int* ptr = nullptr;
  if (hipMalloc(&ptr, cap * sizeof(int)) != hipSuccess) return nullptr;
  if (hipMemsetAsync(ptr, 0, cap * sizeof(int), st) != hipSuccess) return nullptr;
  e = {ptr, cap};
  return ptr;
}
// The plan under the process's options; the device is asked for its CU count only where
// the tail split can apply.
// A launch that honours a liveness mask takes the plain raster.  The grouped raster hands each
// XCD one contiguous range of row tiles (or of K pieces) -- with 8 samples on 8 XCDs, about one
// sample each -- so a dead sample would idle one XCD while the other seven took as long as
// before (measured: no gain, profiles/drop_skip/).  In the plain raster neighbouring jobs go
// to different XCDs and the dead ones spread evenly.  The raster never changes a value.
static GemmPlan plan_for(const mdemi_gemm_desc* d, int mode, int variant) {
  const bool tail = g_opt.tail_split && tail_split_shape(d);
  const bool masked = mode == GEMM_F32 && (d->m_live || d->k_live);
  return plan_gemm(d, mode, variant, tail ? device_cus() : 0, GemmOptions{tail, masked ? 0 : g_opt.group_m});
}
// workspace of a split plan: slabs, row-sum partials, then the deep combine's column-sum scratch
static size_t plan_bytes(const mdemi_gemm_desc* d, const GemmPlan& g) {
  return g.slab_bytes + g.rowsum_bytes + (g.deep ? colsum_ws_bytes(g.split, (int64_t)d->M * d->N) : 0);
}

// bf16 operands / output of mdemi_gemm_bf16x (null for the fp32-operand entry points)
struct B16Ext {
  const void* a16; const void* b16; void* c16;
};

// One GEMM made ready to launch: the plan, the kernel arguments and what follows the launch.
// launch() runs it in a grid of its own; launch_pair() puts two of them into one grid.
struct Prepared {
  GemmPlan g;
  GemmParams p;
  float* rowsum_part;
  bool deep;
  int64_t counters;  // split-tile counters an in-launch combine needs (0: combined after the launch)
};

// everything of launch() up to the counters and the kernel choice
static int prepare(const mdemi_gemm_desc* d, int variant, int mode, const B16Ext* ext, Prepared& r) {
  r.g = plan_for(d, mode, variant);
  const GemmPlan& g = r.g;
  GemmParams& p = r.p;
  fill_params(d, g, p);
  if (ext) {
    p.c16 = ext->c16;
    if (mode == GEMM_B16) {  // the kernel reads the bf16 tensors through the A/B slots
      p.A = reinterpret_cast<const float*>(ext->a16);
      p.B = reinterpret_cast<const float*>(ext->b16);
    }
  }
  r.rowsum_part = nullptr;
  if (p.split > 1) {
    const size_t need = plan_bytes(d, g);
    if (!d->workspace || (size_t)d->workspace_bytes < need) {
      set_error("gemm: split-K needs %zu workspace bytes", need);
      return MDEMI_EWORKSPACE;
    }
    p.slab = (float*)d->workspace;
    if (d->rowsum_a) {
      r.rowsum_part = (float*)((char*)d->workspace + g.slab_bytes);
      p.rowsum = r.rowsum_part;
    }
  }
  MDEMI_REQUIRE(g.nblocks < (int64_t)1 << 31, "gemm: grid too large");
  r.deep = g.deep && !p.c16;  // the column-sum combine writes fp32 only
  // both bf16 families (bf16 operands in HBM, or rounded at staging) combine alike, so the
  // bf16-storage step stays bit-identical to the fp32-operand bf16 step
  const bool inline_reduce = (mode == GEMM_B16 || mode == GEMM_BF16) ? g_inline_reduce_b16 : g_inline_reduce;
  r.counters = (p.split > 1 && !r.deep && (inline_reduce || p.m_split > 0)) ? (int64_t)p.tiles_m * p.tiles_n * d->batch : 0;
  return MDEMI_OK;
}
// hands the split tiles their counters (null: none to be had, the reduce kernel combines)
static void set_counters(const mdemi_gemm_desc* d, Prepared& r, int* cnt) {
  r.p.tile_cnt = cnt;
  if (cnt && r.rowsum_part) r.p.rowsum_out = d->rowsum_a;  // the last arrivers sum the row partials
}
static int finish(const mdemi_gemm_desc* d, const Prepared& r, hipStream_t st);

static int launch(const mdemi_gemm_desc* d, int variant, hipStream_t st, int mode, const B16Ext* ext = nullptr) {
  variant = resolve_variant(d, mode, variant);
  KernelFn fn = mode == GEMM_F32   ? pick_kernel(d->a_layout, d->b_layout, d->a_op, d->b_op, variant)
                : mode == GEMM_B16 ? pick_kernel_b16(d->a_layout, d->b_layout, variant)
                                   : pick_kernel_m16(d->a_layout, d->b_layout, d->a_op, d->b_op,
                                                     mode == GEMM_BF16 ? 1 : 3, variant);
  if (!fn) {
    set_error("gemm: unsupported layout/op combination a=%d/%d b=%d/%d", d->a_layout, d->a_op, d->b_layout,
              d->b_op);
    return MDEMI_EUNSUP;
  }
  Prepared r;
  if (int rc = prepare(d, variant, mode, ext, r)) return rc;
  if (r.counters) set_counters(d, r, tile_counters(r.counters, st));
  hipLaunchKernelGGL(fn, dim3((unsigned)r.g.nblocks), dim3(GTHREADS), 0, st, r.p);
  if (int rc = finish(d, r, st)) return rc;
  return check_launch(mode == GEMM_BF16 ? "gemm_bf16" : mode == GEMM_F32E ? "gemm_f32e" : mode == GEMM_B16 ? "gemm_bf16x" : "gemm_f32");
}

// the combine of a split GEMM whose pieces were not combined inside the launch
static int finish(const mdemi_gemm_desc* d, const Prepared& r, hipStream_t st) {
  const GemmPlan& g = r.g;
  const GemmParams& p = r.p;
  float* const rowsum_part = r.rowsum_part;
  const bool deep = r.deep;
  if (p.split > 1 && !p.tile_cnt) {
    if (deep) {
      // many slabs over a small C (skinny weight gradients over ~10^6 pixels): a
      // column sum parallel over the slab rows, not one thread per output summing
      // `split` dependent loads
      char* cws = (char*)d->workspace + g.slab_bytes + g.rowsum_bytes;
      int rc = colsum_launch(p.slab, p.split, (int64_t)d->M * d->N, (int64_t)d->M * d->N, d->C, 0, cws, st);
      if (!rc && rowsum_part) rc = colsum_launch(rowsum_part, p.split, d->M, d->M, d->rowsum_a, 0, cws, st);
      if (rc) return rc;
    } else {
      const int64_t total = (int64_t)(d->M - p.m_split) * d->N * d->batch / ((d->N & 3) == 0 ? 4 : 1);
      const int nb = (int)(cdiv(total, 256) < 4096 ? cdiv(total, 256) : 4096);
      hipLaunchKernelGGL(gemm_splitk_reduce, dim3(nb), dim3(256), 0, st, p, (const float*)rowsum_part,
                         rowsum_part ? d->rowsum_a : (float*)nullptr);
    }
  }
  return MDEMI_OK;
}

struct TuneKey {
  int al, bl, aop, bop, M, N, K, batch, split, mode;
  bool operator<(const TuneKey& o) const {
    return std::tie(al, bl, aop, bop, M, N, K, batch, split, mode) <
           std::tie(o.al, o.bl, o.aop, o.bop, o.M, o.N, o.K, o.batch, o.split, o.mode);
  }
};
static std::map<TuneKey, int> g_tuned;
static std::mutex g_tune_mu;

// Re-running the GEMM is only harmless when C is write-only and aliases no input.
static bool tunable(const mdemi_gemm_desc* d, hipStream_t st) {
  if (d->beta != 0.f) return false;
  const void* c = d->C;
  if (c == d->A || c == d->B || c == d->residual || c == d->aux || c == d->bias) return false;
  if (d->rowsum_a && (d->rowsum_a == d->A || d->rowsum_a == d->B)) return false;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return false;
  return true;
}

static int choose_variant(const mdemi_gemm_desc* d_in, hipStream_t st, int mode, const B16Ext* ext = nullptr) {
  const int forced = mode == GEMM_F32 ? g_variant : mode == GEMM_B16 ? g_variant_b16 : g_variant_m16;
  if (forced >= 0) return forced;
  // the candidates are timed on the whole product (no liveness mask), so the cached winner of
  // a shape does not depend on which samples one call happened to drop
  mdemi_gemm_desc whole = *d_in;
  whole.m_live = whole.k_live = nullptr;
  const mdemi_gemm_desc* d = &whole;
  const TuneKey key{d->a_layout, d->b_layout, d->a_op, d->b_op, d->M, d->N, d->K, d->batch, d->split_k, mode};
  {
    std::lock_guard<std::mutex> lk(g_tune_mu);
    auto it = g_tuned.find(key);
    if (it != g_tuned.end()) return it->second;
  }
  if (!tunable(d, st)) return 0;
  if (ext && ext->c16 && (ext->c16 == ext->a16 || ext->c16 == ext->b16)) return 0;
  hipEvent_t e0, e1;
  if (hipEventCreate(&e0) != hipSuccess) return 0;
  if (hipEventCreate(&e1) != hipSuccess) {
    (void)hipEventDestroy(e0);
    return 0;
  }
  int best = 0;
  float best_ms = 1e30f;
  for (int v = 0; v < variant_table(mode).n; ++v) {
    if (!tune_candidate(d, mode, v)) continue;
    if (launch(d, v, st, mode, ext) != MDEMI_OK) continue;  // warm (and validate)
    (void)hipEventRecord(e0, st);
    for (int r = 0; r < 3; ++r) launch(d, v, st, mode, ext);
    (void)hipEventRecord(e1, st);
    float ms = 0.f;
    if (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess) continue;
    if (ms < best_ms) { best_ms = ms; best = v; }
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  std::lock_guard<std::mutex> lk(g_tune_mu);
  g_tuned[key] = best;
  return best;
}

extern "C" size_t mdemi_gemm_workspace_size(const mdemi_gemm_desc* d) {
  if (!d) return 0;
  // every variant of every family splits at the same 32-element chunks
  return plan_bytes(d, plan_for(d, GEMM_F32, 0));
}

static int gemm_entry(const mdemi_gemm_desc* d, void* stream, int mode) {
  int rc = validate(d);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  return launch(d, choose_variant(d, st, mode), st, mode);
}

// bf16-operand path: both operands bf16 in HBM and a layout the DMA loaders stage (16-B
// quads of 8 bf16: k-contiguous K % 8, m/n-contiguous extent % 8, implicit-im2col C % 8,
// leading dimensions and batch strides % 8, 16-B aligned bases, no load-time op, no
// bias-gradient row sums -- those are summed from the unrounded fp32 operand)
static bool b16_ok(const mdemi_gemm_desc* d, const B16Ext& e) {
  if (!e.a16 || !e.b16 || !al16(e.a16) || !al16(e.b16)) return false;
  if (d->a_op != MDEMI_OP_NONE || d->b_op != MDEMI_OP_NONE || d->rowsum_a) return false;
  if (d->a_layout == MDEMI_L_CONV && d->b_layout == MDEMI_L_CONV) return false;
  auto operand = [&](int layout, int64_t ld, int64_t bs, int64_t bs2, int64_t extent) {
    if (layout == MDEMI_L_CONV) {
      const mdemi_conv_geom& g = d->conv;
      return g.c % 8 == 0 && (int64_t)g.n * g.h * g.w * g.c * 2 < ((int64_t)1 << 31);
    }
    if (ld % 8 || bs % 8 || bs2 % 8) return false;
    return layout == MDEMI_L_KCONTIG ? d->K % 8 == 0 : extent % 8 == 0;
  };
  const int64_t ai = d->batch_inner > 1 ? d->a_bstride_inner : 0, bi = d->batch_inner > 1 ? d->b_bstride_inner : 0;
  return operand(d->a_layout, d->lda, d->a_bstride, ai, d->M) && operand(d->b_layout, d->ldb, d->b_bstride, bi, d->N);
}

extern "C" int mdemi_gemm_bf16x(const mdemi_gemm_desc* d, const void* a16, const void* b16, void* c16, void* stream) {
  MDEMI_REQUIRE(d, "gemm: null descriptor");
  const B16Ext e{a16, b16, c16};
  hipStream_t st = (hipStream_t)stream;
  if (b16_ok(d, e)) {
    mdemi_gemm_desc v = *d;  // validate() checks the fp32 operand slots; the bf16 ones stand in
    v.A = (const float*)a16;
    v.B = (const float*)b16;
    int rc = validate(&v);
    if (rc) return rc;
    return launch(d, choose_variant(d, st, GEMM_B16, &e), st, GEMM_B16, &e);
  }
  // a layout the bf16 loaders cannot stage: the m16 family on the fp32 operands (the same
  // bf16 products, bit for bit)
  MDEMI_REQUIRE(d->A && d->B, "gemm_bf16x: no bf16 path for this layout (a=%d b=%d) and no fp32 operands given",
                d->a_layout, d->b_layout);
  int rc = validate(d);
  if (rc) return rc;
  const B16Ext f{nullptr, nullptr, c16};
  return launch(d, choose_variant(d, st, GEMM_BF16, &f), st, GEMM_BF16, &f);
}

extern "C" int mdemi_gemm_bf16x_supported(const mdemi_gemm_desc* d, const void* a16, const void* b16) {
  return d && b16_ok(d, B16Ext{a16, b16, nullptr}) ? 1 : 0;
}

extern "C" int mdemi_gemm_f32(const mdemi_gemm_desc* d, void* stream) { return gemm_entry(d, stream, GEMM_F32); }
extern "C" int mdemi_gemm_bf16(const mdemi_gemm_desc* d, void* stream) { return gemm_entry(d, stream, GEMM_BF16); }
extern "C" int mdemi_gemm_f32e(const mdemi_gemm_desc* d, void* stream) { return gemm_entry(d, stream, GEMM_F32E); }

// ---------------------------------------------------------------------------------------------
// Paired launch: two independent fp32 GEMMs in one grid (gemm_glds_kernel_pair).  Each member
// keeps the plan plan_for() gives it alone -- K split, tail split, raster, split chunks -- and
// its own combine after the launch, so every tile is the tile its own launch computes and
// only the launch it runs in changes.  Which of {two launches, pair at variant 11, pair at
// variant 8} runs is timed once per pair of shapes; all three are bit-identical.
// ---------------------------------------------------------------------------------------------
namespace mdemi {
using KernelPairFn = void (*)(GemmParams, GemmParams, int);
KernelPairFn glds_pair_pick_part0(int al0, int bl0, int al1, int bl1, int v);
KernelPairFn glds_pair_pick_part1(int al0, int bl0, int al1, int bl1, int v);
}  // namespace mdemi

enum { PAIR_SEPARATE = 0, PAIR_V11 = 1, PAIR_V8 = 2, PAIR_ARMS = 3 };
static const int PAIR_ARM_VARIANT[PAIR_ARMS] = {-1, 11, 8};
static bool g_pair_on = env_on("MDEMI_GEMM_PAIR");
static bool g_pair_log = env_set("MDEMI_GEMM_PAIR_LOG");
static int g_pair_force = -1;  // -1: the tuner decides
static int g_pair_last = -1;   // the arm the last mdemi_gemm_f32_pair call ran
static std::map<std::pair<TuneKey, TuneKey>, int> g_pair_tuned;

static size_t align256(size_t n) { return (n + 255) / 256 * 256; }

static KernelPairFn pick_pair(const mdemi_gemm_desc* d0, const mdemi_gemm_desc* d1, int v) {
  if (KernelPairFn f = glds_pair_pick_part0(d0->a_layout, d0->b_layout, d1->a_layout, d1->b_layout, v)) return f;
  return glds_pair_pick_part1(d0->a_layout, d0->b_layout, d1->a_layout, d1->b_layout, v);
}

// The two may share a grid at variant v: both run v as itself (dense vectorisable operands,
// no load-time op), batch 1, a kernel for their layouts, and nothing one writes overlaps
// anything the other reads or writes.  Anything else is two launches, not an error.
static bool pair_eligible(const mdemi_gemm_desc* d0, const mdemi_gemm_desc* d1, int v) {
  if (!pair_variant(v) || d0->batch != 1 || d1->batch != 1) return false;
  if (!glds_ok(d0) || !glds_ok(d1) || !pick_pair(d0, d1, v)) return false;
  const size_t ws0 = plan_bytes(d0, plan_for(d0, GEMM_F32, v)), ws1 = plan_bytes(d1, plan_for(d1, GEMM_F32, v));
  return pair_independent(gemm_footprint(d0, ws0), gemm_footprint(d1, ws1));
}

static int launch_pair(const mdemi_gemm_desc* d0, const mdemi_gemm_desc* d1, int v, hipStream_t st) {
  KernelPairFn fn = pick_pair(d0, d1, v);
  MDEMI_REQUIRE(fn && pair_variant(v), "gemm_pair: no paired kernel for these layouts at variant %d", v);
  Prepared r0, r1;
  if (int rc = prepare(d0, v, GEMM_F32, nullptr, r0)) return rc;
  if (int rc = prepare(d1, v, GEMM_F32, nullptr, r1)) return rc;
  MDEMI_REQUIRE(r0.g.nblocks + r1.g.nblocks < (int64_t)1 << 31, "gemm_pair: grid too large");
  if (r0.counters + r1.counters) {  // disjoint ranges of the per-device counters
    int* cnt = tile_counters(r0.counters + r1.counters, st);
    if (r0.counters) set_counters(d0, r0, cnt);
    if (r1.counters) set_counters(d1, r1, cnt ? cnt + r0.counters : nullptr);
  }
  hipLaunchKernelGGL(fn, dim3((unsigned)(r0.g.nblocks + r1.g.nblocks)), dim3(GTHREADS), 0, st, r0.p, r1.p,
                     (int)r0.g.nblocks);
  if (int rc = finish(d0, r0, st)) return rc;
  if (int rc = finish(d1, r1, st)) return rc;
  return check_launch("gemm_f32_pair");
}

static int run_pair_arm(const mdemi_gemm_desc* d0, const mdemi_gemm_desc* d1, int arm, int v0, int v1, hipStream_t st) {
  if (arm != PAIR_SEPARATE) return launch_pair(d0, d1, PAIR_ARM_VARIANT[arm], st);
  if (int rc = launch(d0, v0, st, GEMM_F32)) return rc;
  return launch(d1, v1, st, GEMM_F32);
}

static TuneKey tune_key(const mdemi_gemm_desc* d, int mode) {
  return TuneKey{d->a_layout, d->b_layout, d->a_op, d->b_op, d->M, d->N, d->K, d->batch, d->split_k, mode};
}

// The arm this pair runs.  Pairing off, a forced arm or a forced variant decide at once; else
// the cached winner of the two shapes, timed on first use outside a capture (on the unmasked
// descriptors, as choose_variant does).  An arm the pair is not eligible for is never returned.
static int choose_pair_arm(const mdemi_gemm_desc* d0, const mdemi_gemm_desc* d1, hipStream_t st) {
  if (!g_pair_on) return PAIR_SEPARATE;
  // eligibility (two plans and a footprint comparison per arm) is worked out only for the
  // arm that would run
  auto arm_if_ok = [&](int a) {
    return a != PAIR_SEPARATE && pair_eligible(d0, d1, PAIR_ARM_VARIANT[a]) ? a : (int)PAIR_SEPARATE;
  };
  if (g_pair_force >= 0) return arm_if_ok(g_pair_force);
  if (g_variant >= 0) {
    for (int a = 1; a < PAIR_ARMS; ++a)
      if (PAIR_ARM_VARIANT[a] == g_variant) return arm_if_ok(a);
    return PAIR_SEPARATE;
  }
  mdemi_gemm_desc w0 = *d0, w1 = *d1;
  w0.m_live = w0.k_live = w1.m_live = w1.k_live = nullptr;
  const std::pair<TuneKey, TuneKey> key{tune_key(&w0, GEMM_F32), tune_key(&w1, GEMM_F32)};
  {
    std::lock_guard<std::mutex> lk(g_tune_mu);
    auto it = g_pair_tuned.find(key);
    if (it != g_pair_tuned.end()) return arm_if_ok(it->second);
  }
  const bool ok[PAIR_ARMS] = {true, pair_eligible(d0, d1, 11), pair_eligible(d0, d1, 8)};
  // not cached: a pair that cannot share a grid in this call (its pointers, its alignment)
  // says nothing about the shapes, so nothing is recorded for them
  if (!ok[PAIR_V11] && !ok[PAIR_V8]) return PAIR_SEPARATE;
  if (!tunable(&w0, st) || !tunable(&w1, st)) return PAIR_SEPARATE;
  const int v0 = choose_variant(&w0, st, GEMM_F32), v1 = choose_variant(&w1, st, GEMM_F32);
  hipEvent_t e0, e1;
  if (hipEventCreate(&e0) != hipSuccess) return PAIR_SEPARATE;
  if (hipEventCreate(&e1) != hipSuccess) {
    (void)hipEventDestroy(e0);
    return PAIR_SEPARATE;
  }
  int best = PAIR_SEPARATE;
  float best_ms = 1e30f, arm_ms[PAIR_ARMS] = {-1.f, -1.f, -1.f};
  for (int a = 0; a < PAIR_ARMS; ++a) {
    if (!ok[a]) continue;
    if (run_pair_arm(&w0, &w1, a, v0, v1, st) != MDEMI_OK) continue;  // warm (and validate)
    (void)hipEventRecord(e0, st);
    for (int r = 0; r < 3; ++r) run_pair_arm(&w0, &w1, a, v0, v1, st);
    (void)hipEventRecord(e1, st);
    float ms = 0.f;
    if (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess) continue;
    arm_ms[a] = ms / 3.f;
    if (ms < best_ms) { best_ms = ms; best = a; }  // ties stay two launches
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (g_pair_log)  // MDEMI_GEMM_PAIR_LOG=1: what the tuner measured, once per pair of shapes (ms; -1: arm not run)
    fprintf(stderr, "mdemi gemm_pair tune: %dx%dx%d/%d (v%d) + %dx%dx%d/%d (v%d): two launches %.4f, pair v11 %.4f, "
            "pair v8 %.4f -> arm %d\n", w0.M, w0.N, w0.K, w0.split_k, v0, w1.M, w1.N, w1.K, w1.split_k, v1,
            arm_ms[0], arm_ms[1], arm_ms[2], best);
  std::lock_guard<std::mutex> lk(g_tune_mu);
  g_pair_tuned[key] = best;
  return best;
}

extern "C" size_t mdemi_gemm_pair_workspace_size(const mdemi_gemm_desc* d0, const mdemi_gemm_desc* d1) {
  return align256(mdemi_gemm_workspace_size(d0)) + mdemi_gemm_workspace_size(d1);
}
extern "C" size_t mdemi_gemm_pair_workspace_offset(const mdemi_gemm_desc* d0) {
  return align256(mdemi_gemm_workspace_size(d0));
}

extern "C" int mdemi_gemm_f32_pair(const mdemi_gemm_desc* d0, const mdemi_gemm_desc* d1, void* stream) {
  if (int rc = validate(d0)) return rc;
  if (int rc = validate(d1)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int arm = choose_pair_arm(d0, d1, st);
  g_pair_last = arm;
  if (arm != PAIR_SEPARATE) return launch_pair(d0, d1, PAIR_ARM_VARIANT[arm], st);
  if (int rc = launch(d0, choose_variant(d0, st, GEMM_F32), st, GEMM_F32)) return rc;
  return launch(d1, choose_variant(d1, st, GEMM_F32), st, GEMM_F32);
}

extern "C" int mdemi_gemm_pair_set_options(int32_t enabled, int32_t force_arm) {
  MDEMI_REQUIRE(force_arm >= -1 && force_arm < PAIR_ARMS, "gemm_pair_set_options: bad arm %d", force_arm);
  g_pair_on = enabled != 0;
  g_pair_force = force_arm;
  return MDEMI_OK;
}
extern "C" int mdemi_gemm_pair_enabled(void) { return g_pair_on ? 1 : 0; }
extern "C" int mdemi_gemm_pair_last_arm(void) { return g_pair_last; }

// Benchmark/tuning hooks: force a variant of a family (an index of its table in
// gemm_plan.h; -1 = per-shape autotune, the default) and the tile raster (group_m > 0:
// XCD-aware grouped raster; 0: plain).
extern "C" int mdemi_gemm_set_variant(int32_t variant, int32_t group_m) {
  MDEMI_REQUIRE(variant >= -1 && variant < variant_table(GEMM_F32).n && group_m >= 0, "gemm_set_variant: bad args");
  g_variant = variant;
  g_opt.group_m = group_m;
  return MDEMI_OK;
}

extern "C" int mdemi_gemm_set_options(int32_t tail_split, int32_t inline_reduce) {
  g_opt.tail_split = tail_split != 0;
  g_inline_reduce = inline_reduce != 0;
  return MDEMI_OK;
}

extern "C" int mdemi_gemm_set_variant_m16(int32_t variant) {
  MDEMI_REQUIRE(variant >= -1 && variant < variant_table(GEMM_BF16).n, "gemm_set_variant_m16: bad variant");
  g_variant_m16 = variant;
  return MDEMI_OK;
}

extern "C" int mdemi_gemm_set_variant_b16(int32_t variant) {
  MDEMI_REQUIRE(variant >= -1 && variant < variant_table(GEMM_B16).n, "gemm_set_variant_b16: bad variant");
  g_variant_b16 = variant;
  return MDEMI_OK;
}
