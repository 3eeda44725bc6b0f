// Host half of the GEMM families in plain C++17, no HIP: what a variant is (one table per
// family), the launch plan (K split, tail split, tile counts, grid, workspace) and the
// workgroup -> job raster the kernels share.  A host compiler builds this header as it is
// (tests/gemm_plan_probe.cpp), so CPU tests check the text the launcher and kernels run.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "mdemi.h"

#ifdef __HIPCC__
#define MDEMI_HD __host__ __device__ __forceinline__
#else
#define MDEMI_HD inline
#endif

namespace mdemi {

// precision modes of the GEMM entry points
constexpr int GEMM_F32 = 0;   // exact-product fp32 MFMA (gemm_f32.hip)
constexpr int GEMM_BF16 = 1;  // bf16 operands, fp32 accumulate (gemm_mfma16.hip, NP = 1)
constexpr int GEMM_F32E = 2;  // fp32 as three bf16 planes, six products (gemm_mfma16.hip, NP = 3)
constexpr int GEMM_B16 = 3;   // bf16 operands in HBM, direct-to-LDS (gemm_b16_kernel.h); numerics of GEMM_BF16

// A variant as the host sees it.  The kernels' pick switches (pick_variant, pick_glds,
// m16_variant, pick_b16) instantiate rows / cols / bk from these entries or static_assert
// them, so the grid the host sizes and the tile a kernel computes cannot disagree.
struct GemmVariant {
  int rows, cols, bk;  // block tile and K depth per LDS tile
  bool dma;            // fp32 operands DMA'd straight into LDS: only where glds_ok
  bool bf16_only;      // bf16 LDS images hold one bf16 plane: not for GEMM_F32E
  bool candidate;      // timed by the per-shape autotuner
};

// fp32 family (tools/gemm_bench.py on the NewCRFs-L07 480x640 bs=8 shapes,
// profiles/r01_gemm_variants_v2.log).  No variant wins every shape (e.g. weight-gradient
// GEMMs over few output tiles want BK32/2 buffers, token-major forwards want BK32/1
// buffer), so by default each distinct (layouts, ops, M, N, K, batch, split) is timed once
// over the candidates on first use and the winner cached.  All variants add the k products
// in the same order and split K at the same 32-element boundaries, so the choice never
// changes a result bit.  (A BK64 single-buffer variant measured no faster than 4 on the
// model's shapes: profiles/round3/gemm_study_bk64.txt)
constexpr GemmVariant F32_VARIANTS[] = {
    // 0: 2 LDS buffers, register prefetch, k-contiguous operands transposed into [k][row]
    //    images (ds_read_b32 fragments)
    {128, 128, 16, false, false, true},
    {128, 128, 16, false, false, true},   // 1: as 0 with [row][k] images (ds_read_b128 fragments)
    {128, 128, 16, false, false, false},  // 2: as 0 capped at 128 VGPRs (4 waves/SIMD; spills)
    {128, 128, 32, false, false, true},   // 3: 2 buffers (2 workgroups/CU by LDS)
    {128, 128, 32, false, false, true},   // 4: 1 buffer
    {128, 128, 32, false, false, true},   // 5: as 3, [row][k]
    {256, 128, 32, false, false, true},   // 6: waves of 128x64, 1 buffer
    {256, 128, 16, false, false, true},   // 7: waves of 128x64, 2 buffers
    // direct-to-LDS staging (buffer_load ... lds, gemm_glds_kernel.h)
    {128, 128, 32, true, false, true},    // 8
    {256, 128, 16, true, false, true},    // 9
    {256, 128, 32, true, false, true},    // 10: 96 KiB, one workgroup per CU
    {128, 128, 16, true, false, true},    // 11
    {128, 192, 32, true, false, true},    // 12: Swin stage 0's N = 192 / 576: no half-empty 128-column tile
};
// 16-bit family (bf16 / split fp32, gemm_mfma16_kernel.h)
constexpr GemmVariant M16_VARIANTS[] = {
    {128, 128, 32, false, false, true},  // 0: two LDS buffers
    {128, 128, 32, false, false, true},  // 1: one buffer (two workgroups per CU by LDS)
    {256, 128, 32, false, false, true},  // 2: two buffers (96 KiB)
    {128, 128, 32, false, true, true},   // 3: bf16 LDS images, two buffers (32 KiB)
    {256, 128, 32, false, true, true},   // 4: bf16 LDS images, two buffers (48 KiB)
};
// bf16-operand family (gemm_b16_kernel.h; DMA throughout, gated as a whole by b16_ok)
constexpr GemmVariant B16_VARIANTS[] = {
    {128, 128, 32, false, false, true},  // 0: 3 waves/SIMD
    {256, 128, 32, false, false, true},  // 1
    {128, 128, 32, false, false, true},  // 2: two K tiles per LDS stage (2 waves/SIMD)
};

struct VariantTable { const GemmVariant* v; int n; };
template <size_t N>
constexpr VariantTable table_of(const GemmVariant (&t)[N]) { return {t, (int)N}; }
constexpr VariantTable variant_table(int mode) {
  return mode == GEMM_F32 ? table_of(F32_VARIANTS) : mode == GEMM_B16 ? table_of(B16_VARIANTS) : table_of(M16_VARIANTS);
}
// every entry with this `dma` has `cols` columns and (bk > 0) K depth bk: what a kernel
// template fixes instead of taking it from its entry
template <size_t N>
constexpr bool tiles_fixed(const GemmVariant (&t)[N], bool dma, int cols, int bk = 0) {
  for (const GemmVariant& e : t)
    if (e.dma == dma && (e.cols != cols || (bk && e.bk != bk))) return false;
  return true;
}

constexpr int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// vector loads need every row start 16-B aligned and whole quads in range
// (KCONTIG: K % 4; MNCONTIG: the row/column extent % 4)
inline bool a_vec(const mdemi_gemm_desc* d) {
  return al16(d->A) && d->lda % 4 == 0 && d->a_bstride % 4 == 0 &&
         (d->batch_inner <= 1 || d->a_bstride_inner % 4 == 0) &&
         (d->a_layout == MDEMI_L_KCONTIG ? d->K % 4 == 0 : d->M % 4 == 0);
}
inline bool b_vec(const mdemi_gemm_desc* d) {
  return al16(d->B) && d->ldb % 4 == 0 && d->b_bstride % 4 == 0 &&
         (d->batch_inner <= 1 || d->b_bstride_inner % 4 == 0) &&
         (d->b_layout == MDEMI_L_KCONTIG ? d->K % 4 == 0 : d->N % 4 == 0);
}
// the direct-to-LDS variants need dense operands that load as whole 16-B quads and no
// load-time transform
inline bool glds_ok(const mdemi_gemm_desc* d) {
  return d->a_layout != MDEMI_L_CONV && d->b_layout != MDEMI_L_CONV && d->a_op == MDEMI_OP_NONE &&
         d->b_op == MDEMI_OP_NONE && a_vec(d) && b_vec(d);
}

// The variant that runs when v is asked for: fp32e has no bf16-image variant and a forced
// DMA variant cannot stage every operand; both fall back to variant 0.
inline int resolve_variant(const mdemi_gemm_desc* d, int mode, int v) {
  const GemmVariant& e = variant_table(mode).v[v];
  return ((mode == GEMM_F32E && e.bf16_only) || (e.dma && !glds_ok(d))) ? 0 : v;
}
// the autotuner times v: a candidate that runs as itself (ties go to the first, in table order)
inline bool tune_candidate(const mdemi_gemm_desc* d, int mode, int v) {
  return variant_table(mode).v[v].candidate && resolve_variant(d, mode, v) == v;
}

// Tail split.  A whole-K GEMM whose 128x128 tiles fill R full rounds of resident
// workgroups plus a thin last round (profiles/round3: 9600x3072x768 = 2.34 rounds of the
// 3-workgroup/CU variant runs at 115 TF/s vs 130 at exactly 2 or 3 rounds) splits the rows
// holding the leftover tiles into `split` K pieces, which fit in the last round's free
// slots, and the last-arriving piece of each tile combines them.  The plan depends on the
// shape only (rows cut at a 256-row boundary, K at the family's 32-element chunks), so every
// variant splits the same outputs the same way and the family stays bit-identical.
struct TailPlan { int m_split, split; };  // split 1: no tail split
// the GEMMs it can apply to; for every other the plan does not depend on the CU count
inline bool tail_split_shape(const mdemi_gemm_desc* d) { return d->split_k <= 1 && d->batch == 1 && !d->rowsum_a; }
inline TailPlan tail_plan(const mdemi_gemm_desc* d, int cus, bool enabled) {
  TailPlan t{0, 1};
  if (!enabled || !tail_split_shape(d)) return t;
  const int64_t tm = ceil_div(d->M, 128), tn = ceil_div(d->N, 128), T = tm * tn;
  const int64_t S = 3LL * cus;  // resident 128x128 tiles (3 workgroups per CU)
  const int64_t full = T / S, rem = T - full * S;
  if (full < 1 || rem == 0 || rem * 10 > S * 6) return t;  // no thin last round
  const int64_t m_split = (tm - ceil_div(rem, tn)) / 2 * 256;
  if (m_split <= 0) return t;
  const int64_t tail_tiles = ceil_div(d->M - m_split, 128) * tn;
  int64_t s = std::min<int64_t>(4, S / tail_tiles);
  s = std::min<int64_t>(s, ceil_div(d->K, 32) / 2);  // every piece keeps >= 2 K chunks
  if (s < 2) return t;
  t.m_split = (int)m_split;
  t.split = (int)s;
  return t;
}

struct GemmOptions { bool tail_split; int group_m; };  // group_m > 0: XCD-aware grouped raster; 0: plain
// Tail split (batch 1): row tiles [0, tiles_m1) take the whole K; the tiles_m row tiles
// below m_split = tiles_m1 * rows are split `split` ways (the last, partial round of
// tiles), as is every tile of an ordinary split-K GEMM (tiles_m1 = 0).
struct GemmPlan {
  int tiles_m1, tiles_m, tiles_n, group_m, batch, split;  // the grid as the raster reads it
  int ktile_per_split, m_split;
  int64_t nblocks;
  size_t slab_bytes, rowsum_bytes;  // split-K slabs [split][batch][M - m_split][N]; row-sum partials [split][M]
  bool deep;  // deep split with a plain store epilogue (no epilogue stage at all, row_scale
              // included): combine by column sums (misc.hip; its workspace,
              // colsum_ws_bytes(split, M * N), follows the two above)
};
inline GemmPlan plan_gemm(const mdemi_gemm_desc* d, int mode, int variant, int cus, const GemmOptions& o) {
  const GemmVariant& e = variant_table(mode).v[variant];
  GemmPlan g{};
  // split boundaries in fixed 32-element K chunks whatever the variant's BK, so the
  // variants of a family agree bit for bit
  const int CH = 32;
  const int kc = (int)ceil_div(d->K, CH);
  const TailPlan tp = tail_plan(d, cus, o.tail_split);
  const int want = tp.split > 1 ? tp.split : d->split_k;
  const int chunks_per_split = (int)ceil_div(kc, want < kc ? want : kc);
  g.ktile_per_split = chunks_per_split * (CH / e.bk);
  g.split = (int)ceil_div(kc, chunks_per_split);
  g.m_split = (tp.split > 1 && g.split > 1) ? tp.m_split : 0;
  g.tiles_m1 = g.m_split / e.rows;
  g.tiles_m = (int)ceil_div(d->M - g.m_split, e.rows);
  g.tiles_n = (int)ceil_div(d->N, e.cols);
  g.group_m = o.group_m;
  g.batch = d->batch;
  g.nblocks = (int64_t)g.tiles_m1 * g.tiles_n + (int64_t)g.tiles_m * g.tiles_n * d->batch * g.split;
  if (g.split > 1) {
    const size_t slab = (size_t)g.split * d->batch * (size_t)(d->M - g.m_split) * d->N * sizeof(float);
    g.slab_bytes = (slab + 255) / 256 * 256;
    g.rowsum_bytes = d->rowsum_a ? (size_t)g.split * d->M * sizeof(float) : 0;
    g.deep = g.split >= 32 && d->batch == 1 && d->alpha == 1.f && d->beta == 0.f && d->bias_mode == MDEMI_BIAS_NONE &&
             d->act == MDEMI_ACT_NONE && !d->residual && !d->preact && !d->row_scale && d->ldc == d->N;
  }
  return g;
}

// n / d for 0 <= n < 2^31 and 0 < d < 2^31 by multiply-shift: the magic is computed on the
// host, the division is exact.
struct FastDiv {
  uint32_t mul, shift;
};
inline FastDiv make_fastdiv(uint32_t d) {
  uint32_t c = 0;
  while ((1u << c) < d) ++c;
  const uint32_t L = 31 + c;
  return FastDiv{(uint32_t)(((uint64_t)1 << L) / d + 1), L};
}
MDEMI_HD int fdiv(int n, const FastDiv& f) { return (int)(((uint64_t)(uint32_t)n * f.mul) >> f.shift); }

// Liveness masks (mdemi_gemm_desc.m_live / k_live): index i belongs to group i / group, and a
// group whose mask entry == 0.0f is dead (a NaN entry is live).  The kernels ask these two
// questions with wave-uniform arguments, so each is a scalar decision: a block tile of rows
// that are all dead runs over no K tile, and a 32-element K chunk (the family's split
// granularity, aligned from k = 0) with no live k is not loaded.
// The group size is carried as its multiply-shift reciprocal (make_fastdiv(group)).
// every index of [i0, i1), 0 <= i0 < i1, is dead
MDEMI_HD bool range_all_dead(const float* live, const FastDiv& group, int i0, int i1) {
  for (int g = fdiv(i0, group), last = fdiv(i1 - 1, group); g <= last; ++g)
    if (live[g] != 0.f) return false;
  return true;
}
// K chunk `chunk` (k in [32 chunk, min(32 chunk + 32, K)), 32 chunk < K) holds a live k
MDEMI_HD bool chunk_live(const float* live, const FastDiv& group, int chunk, int K) {
  const int k0 = 32 * chunk;
  return !range_all_dead(live, group, k0, K - k0 < 32 ? K : k0 + 32);
}

// XCD-aware linear order: workgroup ids b, b+8, ... (one XCD) take one contiguous range
// of [0, n), so neighbouring jobs share that XCD's L2.
MDEMI_HD int xcd_lin(int bid, int n) {
  const int q = n / 8, r = n % 8;
  const int xcd = bid % 8, idx = bid / 8;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

// tile (tm, tn) for a linear workgroup id over tiles_m x tiles_n tiles: XCD-aware
// remap (blocks b, b+8, ... share an XCD), then grouped raster so concurrently running
// tiles of one XCD reuse A row-panels (group_m rows of tiles) and B column-panels.
// G: GemmPlan or GemmParams (the fields they share).
template <class G>
MDEMI_HD void tile_of(const G& p, int bid, int ntiles, int tiles_m, int& tm, int& tn, bool remap = true) {
  if (p.group_m <= 0) {  // plain raster: n fastest
    tm = bid / p.tiles_n;
    tn = bid % p.tiles_n;
    return;
  }
  const int lin = remap ? xcd_lin(bid, ntiles) : bid;
  const int per_group = p.group_m * p.tiles_n;
  const int grp = lin / per_group;
  const int first_m = grp * p.group_m;
  const int gm = tiles_m - first_m < p.group_m ? tiles_m - first_m : p.group_m;
  const int in_grp = lin % per_group;
  tm = first_m + in_grp % gm;
  tn = in_grp / gm;
}

// What workgroup `bid` computes: the whole-K tiles of the leading region come first in
// launch order, then the split region's pieces (all tiles' piece 0, then piece 1, ...).
struct GemmJob {
  int b, sidx, tm, tn, cid;  // cid: counter slot of a split tile
  bool split;
};
template <class G>
MDEMI_HD GemmJob job_of(const G& p, int bid) {
  GemmJob j;
  const int n1 = p.tiles_m1 * p.tiles_n;
  if (bid < n1) {
    j.b = 0; j.sidx = 0; j.split = false; j.cid = 0;
    tile_of(p, bid, n1, p.tiles_m1, j.tm, j.tn);
    return j;
  }
  bid -= n1;
  const int n2 = p.tiles_m * p.tiles_n;
  // The XCD remap runs over all (batch entry, K piece, tile) jobs, piece-major: every tile
  // of one K piece (and of one batch entry) lands on one XCD, so a piece's operand rows --
  // e.g. the NHWC pixels the im2col columns of a weight-gradient GEMM gather once per
  // tap -- are fetched into one L2 instead of up to eight.
  if (p.group_m > 0) bid = xcd_lin(bid, n2 * p.batch * p.split);
  const int zb = bid / n2, t2 = bid - zb * n2;
  j.b = zb / p.split;
  j.sidx = zb - j.b * p.split;
  j.split = p.split > 1;
  int tm2;
  tile_of(p, t2, n2, p.tiles_m, tm2, j.tn, false);
  j.tm = p.tiles_m1 + tm2;
  j.cid = j.b * n2 + tm2 * p.tiles_n + j.tn;
  return j;
}

// Paired launch (mdemi_gemm_f32_pair): one grid of nblocks0 + nblocks1 workgroups runs two
// independent GEMMs.  Workgroup `bid` is job `bid` of member 0 when bid < nblocks0, else job
// bid - nblocks0 of member 1; within a member, job_of maps the job as in its own launch.
struct PairJob { int member, bid; };
MDEMI_HD PairJob pair_job_of(int bid, int nblocks0) {
  return bid < nblocks0 ? PairJob{0, bid} : PairJob{1, bid - nblocks0};
}
// the variants a pair can run in one grid: direct-to-LDS, 128x128 tiles
constexpr bool pair_variant(int v) {
  return v >= 0 && v < (int)(sizeof(F32_VARIANTS) / sizeof(F32_VARIANTS[0])) && F32_VARIANTS[v].dma &&
         F32_VARIANTS[v].rows == 128 && F32_VARIANTS[v].cols == 128;
}

// What a GEMM reads and writes, as byte ranges computed from the descriptor's extents and
// leading dimensions (batch 1): rows of `width` bytes every `pitch` bytes within [lo, hi)
// (pitch 0: one row).  Two GEMMs may share a grid only when nothing one writes overlaps
// anything the other reads or writes.
struct ByteRange { uintptr_t lo, hi, pitch, width; };
// Conservative: false only when no byte can be shared -- the spans are apart, or both are
// rows of one pitch whose column intervals (addresses modulo the pitch) are apart, as
// column slices of one wider buffer are.
inline bool ranges_overlap(const ByteRange& a, const ByteRange& b) {
  if (!(a.lo < b.hi && b.lo < a.hi)) return false;
  const uintptr_t pitch = a.pitch ? a.pitch : b.pitch;
  if (!pitch || (b.pitch && b.pitch != pitch)) return true;
  // relative to a's rows, which take residues [0, a.width): b's take [delta, delta + b.width)
  const uintptr_t delta = b.lo >= a.lo ? (b.lo - a.lo) % pitch : (pitch - (a.lo - b.lo) % pitch) % pitch;
  return !(delta >= a.width && delta + b.width <= pitch);
}
struct GemmFootprint {
  ByteRange reads[9], writes[4];
  int nr, nw;
};
inline ByteRange span_of(const void* p, int64_t rows, int64_t ld, int64_t cols) {  // rows x cols floats, pitch ld
  const uintptr_t lo = (uintptr_t)p, w = (uintptr_t)cols * sizeof(float);
  return ByteRange{lo, lo + (uintptr_t)(rows - 1) * (uintptr_t)ld * sizeof(float) + w,
                   rows > 1 ? (uintptr_t)ld * sizeof(float) : 0, w};
}
// ws_bytes: the bytes of d->workspace the plan uses (0: none)
inline GemmFootprint gemm_footprint(const mdemi_gemm_desc* d, size_t ws_bytes) {
  GemmFootprint f{};
  auto rd = [&](const void* p, int64_t rows, int64_t ld, int64_t cols) {
    if (p) f.reads[f.nr++] = span_of(p, rows, ld, cols);
  };
  auto wr = [&](const void* p, int64_t rows, int64_t ld, int64_t cols) {
    if (p) f.writes[f.nw++] = span_of(p, rows, ld, cols);
  };
  if (d->a_layout == MDEMI_L_KCONTIG) rd(d->A, d->M, d->lda, d->K); else rd(d->A, d->K, d->lda, d->M);
  if (d->b_layout == MDEMI_L_KCONTIG) rd(d->B, d->N, d->ldb, d->K); else rd(d->B, d->K, d->ldb, d->N);
  rd(d->aux, d->M, d->ldaux, d->N);
  rd(d->residual, d->M, d->ldres, d->N);
  if (d->bias_mode != MDEMI_BIAS_NONE) rd(d->bias, 1, 0, d->bias_mode == MDEMI_BIAS_ROW ? d->M : d->N);
  if (d->row_scale) rd(d->row_scale, 1, 0, ceil_div(d->M, d->row_scale_group));
  if (d->m_live) rd(d->m_live, 1, 0, ceil_div(d->M, d->m_live_group));
  if (d->k_live) rd(d->k_live, 1, 0, ceil_div(d->K, d->k_live_group));
  wr(d->C, d->M, d->ldc, d->N);
  wr(d->preact, d->M, d->ldpre, d->N);
  wr(d->rowsum_a, 1, 0, d->M);
  if (ws_bytes && d->workspace) f.writes[f.nw++] = ByteRange{(uintptr_t)d->workspace, (uintptr_t)d->workspace + ws_bytes, 0, ws_bytes};
  return f;
}
inline bool pair_independent(const GemmFootprint& f0, const GemmFootprint& f1) {
  auto clash = [](const GemmFootprint& w, const GemmFootprint& o) {
    for (int i = 0; i < w.nw; ++i) {
      for (int j = 0; j < o.nr; ++j)
        if (ranges_overlap(w.writes[i], o.reads[j])) return true;
      for (int j = 0; j < o.nw; ++j)
        if (ranges_overlap(w.writes[i], o.writes[j])) return true;
    }
    return false;
  };
  return !clash(f0, f1) && !clash(f1, f0);
}

}  // namespace mdemi
