// Host probe of csrc/gemm_plan.h for the CPU tests (tests/gemm_plan_util.py builds it with the
// host compiler, -Iinclude only): prints what the launcher's own plan and raster code compute.
//   jobs tiles_m1 tiles_m tiles_n batch split group_m -> "b sidx tm tn" per workgroup id
//   plan M N K batch split_k cus [row_scale]         -> one line per mode and variant legal for it
//                                                       (row_scale 1: the descriptor carries a row_scale)
//   tail M N K cus                                   -> "m_split split" of tail_plan
//   tables                                           -> "mode n" and the autotune candidates per mode,
//                                                       for operands that can / cannot be DMA-staged
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "gemm_plan.h"

using namespace mdemi;

static mdemi_gemm_desc dense(int M, int N, int K, int batch, int split_k) {
  mdemi_gemm_desc d;
  memset(&d, 0, sizeof d);
  d.M = M; d.N = N; d.K = K; d.batch = batch; d.split_k = split_k;
  d.lda = d.ldb = K; d.ldc = N;  // k-contiguous A and B, plain store epilogue
  d.a_bstride = d.b_bstride = 0; d.c_bstride = (int64_t)M * N;
  d.alpha = 1.f;
  return d;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  int a[8] = {0};
  for (int i = 2; i < argc && i < 10; ++i) a[i - 2] = atoi(argv[i]);
  const int modes[] = {GEMM_F32, GEMM_BF16, GEMM_F32E, GEMM_B16};
  if (!strcmp(argv[1], "jobs") && argc == 8) {
    GemmPlan g{};
    g.tiles_m1 = a[0]; g.tiles_m = a[1]; g.tiles_n = a[2]; g.batch = a[3]; g.split = a[4]; g.group_m = a[5];
    const int64_t n = (int64_t)g.tiles_m1 * g.tiles_n + (int64_t)g.tiles_m * g.tiles_n * g.batch * g.split;
    for (int bid = 0; bid < n; ++bid) {
      const GemmJob j = job_of(g, bid);
      printf("%d %d %d %d\n", j.b, j.sidx, j.tm, j.tn);
    }
  } else if (!strcmp(argv[1], "plan") && (argc == 8 || argc == 9)) {
    mdemi_gemm_desc d = dense(a[0], a[1], a[2], a[3], a[4]);
    static const float scale[1] = {1.f};
    if (a[6]) { d.row_scale = scale; d.row_scale_group = d.M; }
    for (int mode : modes)
      for (int v = 0; v < variant_table(mode).n; ++v) {
        const GemmVariant& e = variant_table(mode).v[v];
        if (mode == GEMM_F32E && e.bf16_only) continue;
        const GemmPlan g = plan_gemm(&d, mode, v, a[5], GemmOptions{true, 8});
        printf("%d %d %d %d %d %d %d %d %d %d %d %lld %zu %zu %d\n", mode, v, e.rows, e.cols, e.bk, g.split,
               g.ktile_per_split, g.m_split, g.tiles_m1, g.tiles_m, g.tiles_n, (long long)g.nblocks, g.slab_bytes,
               g.rowsum_bytes, (int)g.deep);
      }
  } else if (!strcmp(argv[1], "tail") && argc == 6) {
    const mdemi_gemm_desc d = dense(a[0], a[1], a[2], 1, 1);
    const TailPlan t = tail_plan(&d, a[3], true);
    printf("%d %d\n", t.m_split, t.split);
  } else if (!strcmp(argv[1], "tables")) {
    for (int mode : modes) {
      printf("%d %d\n", mode, variant_table(mode).n);
      for (int K : {64, 63}) {  // K % 4 != 0: k-contiguous operands cannot load as 16-B quads
        const mdemi_gemm_desc d = dense(64, 64, K, 1, 1);
        for (int v = 0; v < variant_table(mode).n; ++v)
          if (tune_candidate(&d, mode, v)) printf("%d ", v);
        printf("\n");
      }
    }
  } else {
    return 2;
  }
  return 0;
}
