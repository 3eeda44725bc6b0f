// Host probe of the liveness predicates of csrc/gemm_plan.h (range_all_dead, chunk_live): the
// text the fp32 GEMM kernels compile, built with the host compiler by tests/test_drop_skip_plan.py.
//   rows group M tile mask   -> one 0/1 per block tile of `tile` rows: every row of the tile is dead
//   chunks group K mask      -> one 0/1 per 32-element K chunk: the chunk holds a live k
// mask: one character per group, '1' live (1.0f), 's' live (a DropPath scale, 1 / 0.7f),
// 'n' live (NaN), '0' dead (0.0f), '-' dead (-0.0f).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gemm_plan.h"

using namespace mdemi;

int main(int argc, char** argv) {
  if (argc < 5) return 2;
  const bool rows = !strcmp(argv[1], "rows");
  if (!rows && strcmp(argv[1], "chunks")) return 2;
  if (argc != (rows ? 6 : 5)) return 2;
  const int group = atoi(argv[2]), extent = atoi(argv[3]);
  const int tile = rows ? atoi(argv[4]) : 32;
  const char* mask = argv[rows ? 5 : 4];
  if (group <= 0 || extent <= 0 || tile <= 0 || (int64_t)strlen(mask) != ceil_div(extent, group)) return 2;
  std::vector<float> live;
  for (const char* c = mask; *c; ++c) {
    switch (*c) {
      case '1': live.push_back(1.f); break;
      case 's': live.push_back(1.f / 0.7f); break;
      case 'n': live.push_back(NAN); break;
      case '0': live.push_back(0.f); break;
      case '-': live.push_back(-0.f); break;
      default: return 2;
    }
  }
  const FastDiv fd = make_fastdiv((uint32_t)group);  // how the launcher hands the group size to the kernels
  for (int t = 0; t * tile < extent; ++t) {
    const int i0 = t * tile, i1 = std::min(i0 + tile, extent);
    const bool r = rows ? range_all_dead(live.data(), fd, i0, i1) : chunk_live(live.data(), fd, t, extent);
    printf("%d", (int)r);
  }
  printf("\n");
  return 0;
}
