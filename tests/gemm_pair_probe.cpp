// Host probe of the paired-launch half of csrc/gemm_plan.h (tests/test_gemm_pair_plan.py builds
// it with the host compiler, also once with -fsanitize=address,undefined):
//   map      -> per ordered pair of member plans "i j n0 n1 ok": ok = every workgroup id of
//               [0, n0 + n1) maps to exactly one (member, job) and every job of both members
//               (batch entry, K piece, tile) is hit exactly once
//   overlap  -> "name independent" for pairs of descriptors laid out in one host buffer
#include <cstdio>
#include <cstring>
#include <set>
#include <tuple>
#include <vector>

#include "gemm_plan.h"

using namespace mdemi;

struct Member { const char* name; int M, N, K, split_k, cus, group_m; };
// unsplit, split 3, split 7, tail-split at 256 CUs (plain and grouped raster), ragged tiles
static const Member MEMBERS[] = {
    {"unsplit-grouped", 200, 136, 72, 1, 0, 8},   {"unsplit-plain", 136, 72, 200, 1, 0, 0},
    {"split3-grouped", 136, 264, 1000, 3, 0, 8},  {"split7-plain", 768, 3072, 9600, 7, 0, 0},
    {"split7-grouped", 768, 3072, 9600, 7, 0, 8}, {"tail-grouped", 9600, 3072, 768, 1, 256, 8},
    {"tail-plain", 9600, 3072, 768, 1, 256, 0},
};

static mdemi_gemm_desc desc(const Member& m) {
  mdemi_gemm_desc d;
  memset(&d, 0, sizeof d);
  d.M = m.M; d.N = m.N; d.K = m.K; d.batch = 1; d.split_k = m.split_k;
  d.lda = d.ldb = m.K; d.ldc = m.N; d.alpha = 1.f;
  return d;
}
static GemmPlan plan(const Member& m) {
  const mdemi_gemm_desc d = desc(m);
  return plan_gemm(&d, GEMM_F32, 11, m.cus, GemmOptions{m.cus > 0, m.group_m});
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const int n = (int)(sizeof(MEMBERS) / sizeof(MEMBERS[0]));
  if (!strcmp(argv[1], "map")) {
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) {
        const GemmPlan g[2] = {plan(MEMBERS[i]), plan(MEMBERS[j])};
        const int n0 = (int)g[0].nblocks, n1 = (int)g[1].nblocks;
        std::set<std::tuple<int, int, int, int, int>> seen;
        std::vector<int> hits[2] = {std::vector<int>(n0, 0), std::vector<int>(n1, 0)};
        bool ok = true;
        for (int bid = 0; bid < n0 + n1; ++bid) {
          const PairJob pj = pair_job_of(bid, n0);
          if (pj.member < 0 || pj.member > 1 || pj.bid < 0 || pj.bid >= (pj.member ? n1 : n0)) { ok = false; break; }
          hits[pj.member][pj.bid]++;
          const GemmJob job = job_of(g[pj.member], pj.bid);
          const GemmPlan& p = g[pj.member];
          ok = ok && job.tm >= 0 && job.tm < p.tiles_m1 + p.tiles_m && job.tn >= 0 && job.tn < p.tiles_n &&
               job.sidx >= 0 && job.sidx < p.split && job.split == (job.tm >= p.tiles_m1 && p.split > 1);
          ok = ok && seen.insert({pj.member, job.b, job.sidx, job.tm, job.tn}).second;
        }
        for (int m = 0; m < 2; ++m)
          for (int h : hits[m]) ok = ok && h == 1;
        // every job of both members: whole-K tiles once, split tiles once per piece
        for (int m = 0; m < 2 && ok; ++m) {
          const GemmPlan& p = g[m];
          for (int tm = 0; tm < p.tiles_m1 + p.tiles_m; ++tm)
            for (int tn = 0; tn < p.tiles_n; ++tn)
              for (int s = 0; s < (tm < p.tiles_m1 ? 1 : p.split); ++s) ok = ok && seen.count({m, 0, s, tm, tn}) == 1;
        }
        printf("%d %d %d %d %d %d %d\n", i, j, n0, n1, (int)ok, g[0].m_split, g[0].split);
      }
  } else if (!strcmp(argv[1], "overlap")) {
    static float buf[1 << 16];
    mdemi_gemm_desc d0, d1;
    auto base = [&](mdemi_gemm_desc& d, int M, int N, int K) {
      memset(&d, 0, sizeof d);
      d.M = M; d.N = N; d.K = K; d.batch = 1; d.split_k = 1; d.alpha = 1.f;
      d.a_layout = d.b_layout = MDEMI_L_KCONTIG; d.lda = d.ldb = K;
    };
    // member 1 reads member 0's C as its A
    base(d0, 64, 32, 16); base(d1, 64, 48, 32);
    d0.A = buf; d0.B = buf + 2048; d0.C = buf + 4096; d0.ldc = 32;
    d1.A = d0.C; d1.lda = 32; d1.B = buf + 8192; d1.C = buf + 16384; d1.ldc = 48;
    printf("dependent %d\n", (int)pair_independent(gemm_footprint(&d0, 0), gemm_footprint(&d1, 0)));
    // column slices [0, 32) and [32, 80) of one [64][80] buffer
    d1.A = buf + 12288; d1.lda = 32;
    d0.C = buf + 20480; d0.ldc = 80; d1.C = buf + 20480 + 32; d1.ldc = 80;
    printf("column_slices %d\n", (int)pair_independent(gemm_footprint(&d0, 0), gemm_footprint(&d1, 0)));
    // slices that share columns [24, 32)
    d1.C = buf + 20480 + 24;
    printf("column_slices_shared %d\n", (int)pair_independent(gemm_footprint(&d0, 0), gemm_footprint(&d1, 0)));
    // apart, but member 1's workspace lies over member 0's rowsum_a
    d1.C = buf + 20480 + 32;
    d0.a_layout = MDEMI_L_MNCONTIG; d0.lda = 64; d0.rowsum_a = buf + 40000;
    d1.workspace = buf + 39990; d1.workspace_bytes = 1024;
    printf("workspace_over_rowsum %d\n", (int)pair_independent(gemm_footprint(&d0, 0), gemm_footprint(&d1, 1024)));
    printf("both_write_one_c %d\n", (int)pair_independent(gemm_footprint(&d0, 0), gemm_footprint(&d0, 0)));
  } else {
    return 2;
  }
  return 0;
}
