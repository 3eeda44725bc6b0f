// fp32 MFMA GEMM with direct-to-LDS operand staging (gfx950 `buffer_load_dwordx4 ... lds`):
// the dma variants of the fp32 family (F32_VARIANTS in gemm_plan.h; pick_glds below) for
// dense operands (k-contiguous or m/n-contiguous, 16-B vectorisable, no load-time op).
//
// Why: the register-staged kernel spends its issue slots and VGPRs on the global loads, the
// LDS stores and the barrier around them; with every load landing in LDS by DMA a wave issues
// one buffer load per KiB of tile and nothing else (profiles/round3/gemm_study_ceilings.txt:
// without global loads the same tiles ran 118-132 TF/s against 97-114 shipped).
//
// Staging.  One wave instruction moves 64 lanes x 16 B into 1 KiB of LDS at a wave-uniform
// base (M0) + 16 * lane, so the images are lane-linear and any swizzle is applied to the
// per-lane GLOBAL address (cdna_hip_programming.md §5, "Async global->LDS copy"):
//   k-contiguous source  -> [row][k] image, BK floats per row, 16-B chunks permuted by
//     chunk ^ swz(row) (BK 32: (row >> 1) & 7; BK 16: (row >> 2) & 3) so the fragment
//     reads (ds_read_b128, 4 k of one row per lane) are bank-conflict free;
//   m/n-contiguous source -> [k][col] image, 128 columns (512 B) per k row, read with
//     ds_read_b32 (32 consecutive columns per half-wave: conflict free).
// Out-of-range rows / k chunks get the buffer offset BUF_OOB, which the descriptor's range
// check turns into zeros written to LDS: no predicates in the K loop.
//
// Pipeline: NBUF = 2 LDS stages; the DMA of K tile kt+1 is issued before tile kt's MFMAs
// and retired by `s_waitcnt vmcnt(0)` + one barrier after them (the only barrier per tile).
// Fragments of k-group g+1 are read from LDS while group g's MFMAs issue.
//
// Numerics: the MFMA k order is the family's (k-step s of group g: lane half h takes
// k = 8g + 4h + s), K is split at the same 32-element chunks, the bias-gradient row sums
// are accumulated in the register kernel's order (thread t: column quad t & 31, k rows
// t >> 5 + 8q, then the 8 partials in order) -- so these variants agree with 0..7 bit for
// bit and the per-shape autotune never changes a result.
#pragma once
#include <type_traits>

#include "common.h"
#include "gemm_core.h"

namespace mdemi {

typedef __attribute__((address_space(3))) void lds_void_t;

__device__ __forceinline__ void glds16(__amdgpu_buffer_rsrc_t r, const void* lds, int voff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (lds_void_t*)lds, 16, voff, 0, 0, 0);
}

template <int BK>
struct GSwz {  // chunk permutation of a [row][k] image
  static constexpr int CH = BK / 4;  // 16-B chunks per row
  __device__ static int of(int row) { return BK == 32 ? (row >> 1) & 7 : (row >> 2) & 3; }
};

// k-contiguous operand, one ROWS-row (128, or 192 for the B operand of the 192-column tile)
// [row][BK] image.  Wave w issues instructions q = w * NI + i (i < NI), each covering rows
// RPI*q .. RPI*q + RPI-1.
template <int BK, int ROWS = 128>
struct GLoadKC {
  static constexpr int CH = BK / 4, RPI = 64 / CH, NI = ROWS / RPI / 4;
  const float* base; int K;
  int voff[NI];  // byte offset of this lane's (row, chunk) within the tile, k0 = 0 (BUF_OOB: row out of range)
  int kch[NI];   // this lane's k chunk (the global chunk stored at its LDS slot)
  __device__ void init(const float* p, int64_t ld, int rows, int K_, int r0, int wid, int lane) {
    base = p + (int64_t)r0 * ld; K = K_;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int q = wid * NI + i, row = RPI * q + lane / CH;
      const int ch = (lane % CH) ^ GSwz<BK>::of(row);
      kch[i] = ch;
      voff[i] = r0 + row < rows ? (int)(((int64_t)row * ld + 4 * ch) * 4) : BUF_OOB;
    }
  }
  __device__ void issue(int k0, float* img, int wid) const {
    const auto rs = make_rsrc(base + k0);
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int q = wid * NI + i;
      glds16(rs, img + q * 256, k0 + 4 * kch[i] < K ? voff[i] : BUF_OOB);
    }
  }
  // 4 consecutive k (8g + 4h .. +3) of image row r
  __device__ static float4 frag(const float* img, int r, int g, int h) {
    return *reinterpret_cast<const float4*>(img + r * BK + 4 * ((2 * g + h) ^ GSwz<BK>::of(r)));
  }
};

// m/n-contiguous operand, one [BK][128] image.  Instruction q covers k rows 2q, 2q+1.
template <int BK>
struct GLoadMN {
  static constexpr int NI = BK / 2 / 4;
  const float* base; int64_t ld; int K;
  int voff, kl;  // this lane's byte offset at k0 = 0 of instruction 0 (BUF_OOB: columns out of range), k row
  __device__ void init(const float* p, int64_t ld_, int cols, int K_, int c0, int wid, int lane) {
    base = p + c0; ld = ld_; K = K_;
    const int col = 4 * (lane & 31);
    kl = 2 * (wid * NI) + (lane >> 5);
    voff = c0 + col < cols ? (int)(((int64_t)kl * ld + col) * 4) : BUF_OOB;
  }
  __device__ void issue(int k0, float* img, int wid) const {
    const auto rs = make_rsrc(base + (int64_t)k0 * ld);
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int q = wid * NI + i;
      const bool kin = k0 + kl + 2 * i < K;
      glds16(rs, img + q * 256, kin && voff != BUF_OOB ? voff + (int)(2 * i * ld * 4) : BUF_OOB);
    }
  }
  __device__ static float4 frag(const float* img, int r, int g, int h) {
    const float* p = img + (8 * g + 4 * h) * 128 + r;
    return make_float4(p[0], p[128], p[256], p[384]);
  }
};

// m/n-contiguous operand, columns 128 .. 191 of the 192-column tile: one [BK][64] image.
// Instruction q covers k rows 4q .. 4q+3 (lane j -> k row 4q + j/16, columns 4 (j%16) ..).
template <int BK>
struct GLoadMN64 {
  static constexpr int NI = BK / 4 / 4;
  const float* base; int64_t ld; int K;
  int voff, kl;
  __device__ void init(const float* p, int64_t ld_, int cols, int K_, int c0, int wid, int lane) {
    base = p + c0; ld = ld_; K = K_;
    const int col = 4 * (lane & 15);
    kl = 4 * (wid * NI) + (lane >> 4);
    voff = c0 + col < cols ? (int)(((int64_t)kl * ld + col) * 4) : BUF_OOB;
  }
  __device__ void issue(int k0, float* img, int wid) const {
    const auto rs = make_rsrc(base + (int64_t)k0 * ld);
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int q = wid * NI + i;
      const bool kin = k0 + kl + 4 * i < K;
      glds16(rs, img + q * 256, kin && voff != BUF_OOB ? voff + (int)(4 * i * ld * 4) : BUF_OOB);
    }
  }
};

// 4 consecutive k (8g + 4h ..) of column c of a [BK][pitch] image (pitch 128 or 64)
__device__ __forceinline__ float4 mn_frag_pitch(const float* img, int pitch, int c, int g, int h) {
  const float* p = img + (8 * g + 4 * h) * pitch + c;
  return make_float4(p[0], p[pitch], p[2 * pitch], p[3 * pitch]);
}

template <int L, int BK, int ROWS = 128>
using GLoad = typename std::conditional<L == MDEMI_L_KCONTIG, GLoadKC<BK, ROWS>, GLoadMN<BK>>::type;

// BMT: block-tile rows (128: 2x2 waves of 64x64; 256: 2x2 waves of 128x64, A as two
// 128-row images).  BNT: block-tile columns, 128, or 192 (2x2 waves of 64x96: the N = 192 /
// 576 GEMMs of the Swin stage 0, which a 128-column tile covers in 1.5 / 4.5 tiles; B as one
// 192-row k-contiguous image, or a 128- and a 64-column m/n-contiguous image).  BK: 16 or
// 32.  OCC: waves per SIMD the register budget targets.
template <int AL, int BL, int BMT, int BK, int OCC, int BNT = 128>
__global__ __launch_bounds__(GTHREADS) __attribute__((amdgpu_waves_per_eu(OCC, 8))) void gemm_glds_kernel(
    GemmParams p) {
  constexpr int STAGE = BMT * BK + BNT * BK;  // A images + the B image(s)
  // stage 0 is `smem` (the epilogue's split-K hand-off flag and the row-sum reduction reuse
  // it after the loop), stage 1 `smem1`
  __shared__ __attribute__((aligned(16))) float smem[STAGE];
  __shared__ __attribute__((aligned(16))) float smem1[STAGE];
  const int bid = blockIdx.x;
#include "gemm_glds_mainloop.inc"
}

// Two independent GEMMs of 128x128 tiles in one grid (mdemi_gemm_f32_pair): workgroups
// [0, nblocks0) run member 0's jobs, the rest member 1's (pair_job_of, gemm_plan.h), each
// member under its own GemmParams and its own plan, so every tile is computed exactly as
// its single launch computes it.  The choice of arm is wave-uniform (a scalar branch on the
// workgroup id); no workgroup waits for another.  Both arms stage through the same two
// LDS arrays.
template <int AL0, int BL0, int AL1, int BL1, int BK, int OCC>
__global__ __launch_bounds__(GTHREADS) __attribute__((amdgpu_waves_per_eu(OCC, 8))) void gemm_glds_kernel_pair(
    GemmParams p0, GemmParams p1, int nblocks0) {
  constexpr int BMT = 128, BNT = 128;
  constexpr int STAGE = BMT * BK + BNT * BK;
  __shared__ __attribute__((aligned(16))) float smem[STAGE];
  __shared__ __attribute__((aligned(16))) float smem1[STAGE];
  const PairJob pj = pair_job_of((int)blockIdx.x, nblocks0);
  if (pj.member == 0) {
    constexpr int AL = AL0, BL = BL0;
    const GemmParams& p = p0;
    const int bid = pj.bid;
#include "gemm_glds_mainloop.inc"
  } else {
    constexpr int AL = AL1, BL = BL1;
    const GemmParams& p = p1;
    const int bid = pj.bid;
#include "gemm_glds_mainloop.inc"
  }
}

// the dma variants of F32_VARIANTS (gemm_f32.hip pick_kernel), instantiated per layout pair in gemm_glds_inst*.hip
template <int AL, int BL>
static void (*pick_glds(int v))(GemmParams) {
  if constexpr (AL == MDEMI_L_CONV || BL == MDEMI_L_CONV) {
    return nullptr;
  } else {
    constexpr const GemmVariant* T = F32_VARIANTS;  // the tile: the host's table (gemm_plan.h)
    switch (v) {
      case 8: return gemm_glds_kernel<AL, BL, T[8].rows, T[8].bk, 2, T[8].cols>;
      case 9: return gemm_glds_kernel<AL, BL, T[9].rows, T[9].bk, 2, T[9].cols>;
      case 10: return gemm_glds_kernel<AL, BL, T[10].rows, T[10].bk, 1, T[10].cols>;
      case 11: return gemm_glds_kernel<AL, BL, T[11].rows, T[11].bk, 3, T[11].cols>;
      case 12: return gemm_glds_kernel<AL, BL, T[12].rows, T[12].bk, 2, T[12].cols>;
      default: return nullptr;
    }
  }
}

// the pair kernel at the variants that can share a grid (pair_variant), with the OCC of the
// single-launch variant each stands for; instantiated per layout quadruple in gemm_pair_inst*.hip
using KernelPairFn = void (*)(GemmParams, GemmParams, int);
template <int AL0, int BL0, int AL1, int BL1>
static KernelPairFn pick_glds_pair(int v) {
  constexpr const GemmVariant* T = F32_VARIANTS;
  static_assert(pair_variant(8) && pair_variant(11), "pair variants: 128x128 direct-to-LDS tiles");
  switch (v) {
    case 8: return gemm_glds_kernel_pair<AL0, BL0, AL1, BL1, T[8].bk, 2>;
    case 11: return gemm_glds_kernel_pair<AL0, BL0, AL1, BL1, T[11].bk, 3>;
    default: return nullptr;
  }
}

}  // namespace mdemi
