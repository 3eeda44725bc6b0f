// Body of the direct-to-LDS fp32 GEMM (gemm_glds_kernel.h): operand staging, the K loop, the
// bias-gradient row sums and the epilogue of ONE job, textually included by gemm_glds_kernel
// and by each arm of gemm_glds_kernel_pair -- for the reason gemm_epilogue.inc is an include:
// a shared device function made hipcc demote the accumulators to scratch.
// In scope: the constants AL, BL (operand layouts), BMT, BNT (block tile), BK; `p` (the
// GemmParams of this job's GEMM); `bid` (the job's index within that GEMM's grid,
// wave-uniform); and the two LDS stages `smem`, `smem1` (STAGE floats each), declared once
// per kernel.  The text may `return` from the kernel (gemm_epilogue.inc).
  static_assert(AL != MDEMI_L_CONV && BL != MDEMI_L_CONV, "dense operands only");
  static_assert(BK == 16 || BK == 32, "BK");
  static_assert(BNT == 128 || (BNT == 192 && BMT == 128), "192-column tiles: 128 rows");
  constexpr int NA = BMT / 128, IM = BMT / 64, WTM = BMT / 2;
  constexpr int WTN = BNT / 2, IN = WTN / 32;  // wave tile columns, 32-column accumulators
  constexpr int IMG = 128 * BK;               // floats per 128-row (or 128-column) image
  constexpr int NG = BK / 8;                  // k groups per tile

  const int t = threadIdx.x, lane = t & 63;
  const int wid = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wm = wid >> 1, wn = wid & 1;
  const GemmJob job = job_of(p, bid);
  const int b = job.b, sidx = job.sidx, tm = job.tm, tn = job.tn;
  const int bm = tm * BMT, bn = tn * BNT;

  using LA = GLoad<AL, BK>;
  using LB = GLoad<BL, BK, BNT>;
  constexpr bool B64 = BNT == 192 && BL == MDEMI_L_MNCONTIG;  // the extra 64-column B image
  LA la[NA];
  LB lb;
  GLoadMN64<BK> lb64;
#pragma unroll
  for (int a = 0; a < NA; ++a)
    la[a].init(p.A + boff(p, b, p.a_bs, p.a_bs2), p.lda, p.M, p.K, bm + 128 * a, wid, lane);
  lb.init(p.B + boff(p, b, p.b_bs, p.b_bs2), p.ldb, p.N, p.K, bn, wid, lane);
  if constexpr (B64) lb64.init(p.B + boff(p, b, p.b_bs, p.b_bs2), p.ldb, p.N, p.K, bn + 128, wid, lane);

  const int ktiles_total = (p.K + BK - 1) / BK;
  const int kt_begin = job.split ? sidx * p.ktile_per_split : 0;
  int kt_end = job.split ? min(ktiles_total, kt_begin + p.ktile_per_split) : ktiles_total;
  if (tile_rows_dead<BMT>(p, bm)) kt_end = kt_begin;  // nothing but the epilogue, on a zero accumulator

  floatx16 acc[IM][IN];
#pragma unroll
  for (int a = 0; a < IM; ++a)
#pragma unroll
    for (int c = 0; c < IN; ++c)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][c][r] = 0.f;

  auto issue = [&](int kt, float* st) {
#pragma unroll
    for (int a = 0; a < NA; ++a) la[a].issue(kt * BK, st + a * IMG, wid);
    lb.issue(kt * BK, st + NA * IMG, wid);
    if constexpr (B64) lb64.issue(kt * BK, st + NA * IMG + IMG, wid);
  };

  // bias-gradient row sums of an m-contiguous A, in the register kernel's order
  constexpr bool CAN_RSUM = AL == MDEMI_L_MNCONTIG;
  const bool do_rsum = CAN_RSUM && p.rowsum != nullptr && tn == 0;
  float4 rsum[NA];
#pragma unroll
  for (int a = 0; a < NA; ++a) rsum[a] = make_float4(0.f, 0.f, 0.f, 0.f);

  const int l31 = lane & 31, h = lane >> 5;
  int rA[IM];
#pragma unroll
  for (int i = 0; i < IM; ++i) rA[i] = (wm * WTM + 32 * i + l31) & 127;
  const int aimg = (wm * WTM) >> 7;
  // B fragment j: columns cb_j = wn * WTN + 32 j (+ l31); for the 192-column m/n-contiguous
  // tile, those >= 128 come from the 64-column image (a wave-uniform choice)
  auto fragB = [&](const float* b_s, int j, int g) -> float4 {
    const int cb = wn * WTN + 32 * j;
    if constexpr (B64) {
      if (cb >= 128) return mn_frag_pitch(b_s + IMG, 64, cb - 128 + l31, g, h);
      return mn_frag_pitch(b_s, 128, cb + l31, g, h);
    } else {
      return LB::frag(b_s, cb + l31, g, h);
    }
  };

  // One K tile: issue the DMA of the next live tile `nk` into `nxt`, then the row sums and
  // MFMAs of the tile staged in `cur`.  The two stages are separate __shared__ objects and
  // every call below names them at compile time (the loop is unrolled by two), so the LDS alias
  // scopes tell it a fragment read of one stage cannot depend on the DMA in flight into the
  // other: without that it waits vmcnt(0) before the first ds_read of every tile and the
  // load no longer overlaps the MFMAs.
  auto tile = [&](const float* cur, float* nxt, int nk) {
    if (nk < kt_end) issue(nk, nxt);
    if (CAN_RSUM && do_rsum) {
#pragma unroll
      for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int q = 0; q < BK / 8; ++q) {
          const float4 v = *reinterpret_cast<const float4*>(cur + a * IMG + ((t >> 5) + 8 * q) * 128 + 4 * (t & 31));
          rsum[a].x += v.x; rsum[a].y += v.y; rsum[a].z += v.z; rsum[a].w += v.w;
        }
    }
    const float* a_s = cur + aimg * IMG;
    const float* b_s = cur + NA * IMG;
    float4 fa[2][IM], fb[2][IN];
#pragma unroll
    for (int i = 0; i < IM; ++i) fa[0][i] = LA::frag(a_s, rA[i], 0, h);
#pragma unroll
    for (int j = 0; j < IN; ++j) fb[0][j] = fragB(b_s, j, 0);
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const int c = g & 1, n = c ^ 1;
      if (g + 1 < NG) {
#pragma unroll
        for (int i = 0; i < IM; ++i) fa[n][i] = LA::frag(a_s, rA[i], g + 1, h);
#pragma unroll
        for (int j = 0; j < IN; ++j) fb[n][j] = fragB(b_s, j, g + 1);
      }
      // keep the reads of group g+1 ahead of group g's MFMAs (the scheduler would otherwise
      // sink them behind the MFMAs and expose their latency at the next group)
      __builtin_amdgcn_sched_barrier(0);
#define MDEMI_GSTEP(X)                                                                             \
  _Pragma("unroll") for (int i = 0; i < IM; ++i)                                                   \
  _Pragma("unroll") for (int j = 0; j < IN; ++j)                                                   \
    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[c][i].X, fb[c][j].X, acc[i][j], 0, 0, 0);
      MDEMI_GSTEP(x) MDEMI_GSTEP(y) MDEMI_GSTEP(z) MDEMI_GSTEP(w)
#undef MDEMI_GSTEP
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's DMA of tile nk has landed
    __syncthreads();                                   // ... every wave's, and `cur` is no longer read
  };

  // the live K tiles only (k_live; every tile without it), each prefetching the next live one
  int kt = live_ktile<BK>(p, kt_begin, kt_end);
  if (kt < kt_end) issue(kt, smem);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  while (kt < kt_end) {
    const int nk = live_ktile<BK>(p, kt + 1, kt_end);
    tile(smem, smem1, nk);
    if (nk >= kt_end) break;
    kt = live_ktile<BK>(p, nk + 1, kt_end);
    tile(smem1, smem, kt);
  }
  if (CAN_RSUM && do_rsum) {  // the 8 k-row groups (t >> 5) of each A image, in order
    float4* red = reinterpret_cast<float4*>(smem);
#pragma unroll
    for (int a = 0; a < NA; ++a) red[a * 256 + t] = rsum[a];
    __syncthreads();
    if (t < 32 * NA) {
      const int a = t >> 5, tt = t & 31;
      float4 s4 = red[a * 256 + tt];
#pragma unroll
      for (int g = 1; g < 8; ++g) {
        const float4 o = red[a * 256 + tt + 32 * g];
        s4.x += o.x; s4.y += o.y; s4.z += o.z; s4.w += o.w;
      }
      store_rowsum4(p, sidx, bm + 128 * a + 4 * tt, s4);
    }
  }

#define EP_IM IM
#define EP_IN IN
#define EP_WTM WTM
#define EP_WTN WTN
#include "gemm_epilogue.inc"
