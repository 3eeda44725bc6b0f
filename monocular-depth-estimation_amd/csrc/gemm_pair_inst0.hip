// Instantiations of the paired direct-to-LDS fp32 GEMM (gemm_glds_kernel_pair,
// gemm_glds_kernel.h): member 0 (KCONTIG, MNCONTIG) -- an input gradient dY . W -- beside
// member 1 (MNCONTIG, MNCONTIG) -- a weight gradient dY^T . X.  The other order is in
// gemm_pair_inst1.hip; a pair of any other layouts runs as two launches.
#include "gemm_glds_kernel.h"

namespace mdemi {

KernelPairFn glds_pair_pick_part0(int al0, int bl0, int al1, int bl1, int v) {
  if (al0 == MDEMI_L_KCONTIG && bl0 == MDEMI_L_MNCONTIG && al1 == MDEMI_L_MNCONTIG && bl1 == MDEMI_L_MNCONTIG)
    return pick_glds_pair<MDEMI_L_KCONTIG, MDEMI_L_MNCONTIG, MDEMI_L_MNCONTIG, MDEMI_L_MNCONTIG>(v);
  return nullptr;
}

}  // namespace mdemi
