// Scale-invariant boundary F1 of a depth prediction against its ground truth (cfg eval.boundary,
// DESIGN.md §1c; after Depth Pro, Bochkovskii et al. 2024).  A pair is two horizontally or
// vertically adjacent pixels that are both valid (met_valid).  At threshold tau a pair (a, b) of
// a map d is an edge of kind "b is farther" when b > fl32(tau a) and of kind "a is farther" when
// a > fl32(tau b): one rounded fp32 multiply and a strict compare, so numpy fp32 agrees on every
// pair.  Per image the sweep counts, for each of the n thresholds and the four kinds (right,
// left, down, up is farther), the edges of g, of q and of both; q is the value the metrics
// kernels evaluate (aligned_value of metrics_kernel.h, then the clamp).
//   One sweep, grid (row chunks, B): each pixel owns its right and its down pair.  fl32(tau x)
// is monotone in tau for x >= 0, so the thresholds such a pair passes are a prefix and the two
// kinds of a direction exclude each other: the pair is one (kind, level m in 0..n) per map.  Most
// pairs have level 0 and touch nothing; the rest increment LDS histograms over the level (gt,
// pred, and both at min(m_g, m_q) when the kinds agree).  A pair with a negative value (an
// unclamped prediction) has neither property and is counted threshold by threshold into a
// second table.  Both are flushed with integer global atomics into the image's zeroed table:
// integer adds commute, two runs give the same bits.  boundary_final turns levels into counts
// with a suffix sum and forms the fp64 scores in a fixed order.
#include "common.h"
#include "image_reduce.h"
#include "mdemi_ext.h"
#include "metrics_kernel.h"

namespace mdemi {

constexpr int BD_MAXT = MDEMI_BOUNDARY_MAX_T;
constexpr int BD_PIXELS = 4096;  // per workgroup, in whole rows

// An image's table of uint32, for n thresholds: lev[j][k][m], j = gt / pred / both, k the kind,
// m the level in 0..n (slot 0 stays empty); then dir[j][k][i], the threshold-by-threshold
// counts of the pairs with a negative value; then the number of pairs.
__host__ __device__ inline int bd_lev(int n, int j, int k, int m) { return (j * 4 + k) * (n + 1) + m; }
__host__ __device__ inline int bd_dir(int n, int j, int k, int i) { return 12 * (n + 1) + (j * 4 + k) * n + i; }
__host__ __device__ inline int bd_pairs(int n) { return 24 * n + 12; }
__host__ __device__ inline int bd_stride(int n) { return 24 * n + 16; }

inline int bd_rows(int W) { return W >= BD_PIXELS ? 1 : BD_PIXELS / W; }

// what the sweep needs of an image to turn pred into q
struct BdQ {
  double s, t, inv_dmax;
  float dmin, dmax;
  int mode, clamp;
  bool failed;
  __device__ __forceinline__ float operator()(float p) const {
    float q = aligned_value(p, s, t, failed, mode, inv_dmax);
    if (clamp) q = fminf(fmaxf(q, dmin), dmax);
    return q;
  }
};

// the number of thresholds the ordered pair lo <= hi (lo >= 0) passes: a prefix of them
__device__ __forceinline__ int bd_level(float lo, float hi, const mdemi_boundary_thresholds& thr) {
  if (!(hi > thr.t[0] * lo)) return 0;
  int m = 1;
  for (int i = 1; i < thr.n; ++i) m += hi > thr.t[i] * lo ? 1 : 0;
  return m;
}

// one valid pair: a the pixel, b its right (dir 0) or lower (dir 1) neighbour
__device__ __forceinline__ void bd_pair(float ga, float gb, float qa, float qb, int dir,
                                        const mdemi_boundary_thresholds& thr, uint32_t* tab) {
  const int n = thr.n;
  if (fminf(fminf(ga, gb), fminf(qa, qb)) < 0.f) {  // no prefix, and both kinds may hold: count as defined
    for (int i = 0; i < n; ++i) {
      const float tau = thr.t[i];
      const bool eg0 = gb > tau * ga, eg1 = ga > tau * gb, eq0 = qb > tau * qa, eq1 = qa > tau * qb;
      if (eg0) atomicAdd(&tab[bd_dir(n, 0, 2 * dir, i)], 1u);
      if (eg1) atomicAdd(&tab[bd_dir(n, 0, 2 * dir + 1, i)], 1u);
      if (eq0) atomicAdd(&tab[bd_dir(n, 1, 2 * dir, i)], 1u);
      if (eq1) atomicAdd(&tab[bd_dir(n, 1, 2 * dir + 1, i)], 1u);
      if (eg0 && eq0) atomicAdd(&tab[bd_dir(n, 2, 2 * dir, i)], 1u);
      if (eg1 && eq1) atomicAdd(&tab[bd_dir(n, 2, 2 * dir + 1, i)], 1u);
    }
    return;
  }
  const int kg = 2 * dir + (gb > ga ? 0 : 1), kq = 2 * dir + (qb > qa ? 0 : 1);
  const int mg = bd_level(fminf(ga, gb), fmaxf(ga, gb), thr);
  const int mq = bd_level(fminf(qa, qb), fmaxf(qa, qb), thr);
  if (mg) atomicAdd(&tab[bd_lev(n, 0, kg, mg)], 1u);
  if (mq) atomicAdd(&tab[bd_lev(n, 1, kq, mq)], 1u);
  if (mg && mq && kg == kq) atomicAdd(&tab[bd_lev(n, 2, kg, min(mg, mq))], 1u);
}

// table[b] += the counts of rows [blockIdx.x * rows, + rows) of image b.  VEC: W % 4 == 0 and
// 16-byte aligned bases, a thread takes four pixels of a row with vector loads.
template <bool VEC>
__global__ __launch_bounds__(256) void boundary_sweep(const float* __restrict__ pred, const float* __restrict__ gt,
                                                      const double* __restrict__ coef, uint32_t* __restrict__ table,
                                                      int H, int W, int y0, int y1, int x0, int x1, float dmin,
                                                      float dmax, int clamp_pred, int mode, int rows,
                                                      mdemi_boundary_thresholds thr) {
  __shared__ uint32_t tab[24 * BD_MAXT + 16];
  const int b = blockIdx.y, n = thr.n;
  const int r0 = blockIdx.x * rows, r1 = min(H, r0 + rows);
  // rows above the crop or below it hold no valid pixel, and so no pair
  const int ya = max(r0, max(y0, 0)), yb = min(r1, y1);
  if (ya >= yb) return;
  BdQ Q{1.0, 0.0, 0.0, dmin, dmax, mode, clamp_pred, true};
  if (mode != 0) {
    Q.s = coef[b * 4 + 0];
    Q.t = coef[b * 4 + 1];
    Q.failed = coef[b * 4 + 3] != 0.0;
    Q.inv_dmax = 1.0 / (double)dmax;
  }
  rs_hist_zero(tab, bd_stride(n));
  const float* P = pred + (int64_t)b * H * W;
  const float* G = gt + (int64_t)b * H * W;
  uint32_t npair = 0;
  if (VEC) {
    const int wv = W >> 2, items = (yb - ya) * wv;
    for (int i = threadIdx.x; i < items; i += 256) {
      const int ry = i / wv, x = (i - ry * wv) * 4, y = ya + ry;
      if (x + 3 < x0 || x >= x1) continue;
      const int64_t o = (int64_t)y * W + x;
      const float4 g4 = *reinterpret_cast<const float4*>(G + o), p4 = *reinterpret_cast<const float4*>(P + o);
      const bool right = x + 4 < W, down = y + 1 < H;
      float g[5] = {g4.x, g4.y, g4.z, g4.w, 0.f}, p[5] = {p4.x, p4.y, p4.z, p4.w, 1.f};
      float gd[4] = {0.f, 0.f, 0.f, 0.f}, pd[4] = {1.f, 1.f, 1.f, 1.f};
      if (right) {
        g[4] = G[o + 4];
        p[4] = P[o + 4];
      }
      if (down) {
        const float4 a = *reinterpret_cast<const float4*>(G + o + W), c = *reinterpret_cast<const float4*>(P + o + W);
        gd[0] = a.x; gd[1] = a.y; gd[2] = a.z; gd[3] = a.w;
        pd[0] = c.x; pd[1] = c.y; pd[2] = c.z; pd[3] = c.w;
      }
      bool v[5];
#pragma unroll
      for (int j = 0; j < 5; ++j)
        v[j] = (j < 4 || right) && met_valid_at(y, x + j, g[j], y0, y1, x0, x1, dmin, dmax);
      float q[5];
#pragma unroll
      for (int j = 0; j < 5; ++j) q[j] = Q(p[j]);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (!v[j]) continue;
        if (v[j + 1]) {
          ++npair;
          bd_pair(g[j], g[j + 1], q[j], q[j + 1], 0, thr, tab);
        }
        if (down && met_valid_at(y + 1, x + j, gd[j], y0, y1, x0, x1, dmin, dmax)) {
          ++npair;
          bd_pair(g[j], gd[j], q[j], Q(pd[j]), 1, thr, tab);
        }
      }
    }
  } else {
    const int xa = max(x0, 0), xb = min(x1, W), wc = xb - xa;  // the crop's columns only
    const int items = wc > 0 ? (yb - ya) * wc : 0;
    for (int i = threadIdx.x; i < items; i += 256) {
      const int ry = i / wc, x = xa + (i - ry * wc), y = ya + ry;
      const int64_t o = (int64_t)y * W + x;
      const float g = G[o];
      if (!met_valid_at(y, x, g, y0, y1, x0, x1, dmin, dmax)) continue;
      const float q = Q(P[o]);
      if (x + 1 < W) {
        const float gr = G[o + 1];
        if (met_valid_at(y, x + 1, gr, y0, y1, x0, x1, dmin, dmax)) {
          ++npair;
          bd_pair(g, gr, q, Q(P[o + 1]), 0, thr, tab);
        }
      }
      if (y + 1 < H) {
        const float gl = G[o + W];
        if (met_valid_at(y + 1, x, gl, y0, y1, x0, x1, dmin, dmax)) {
          ++npair;
          bd_pair(g, gl, q, Q(P[o + W]), 1, thr, tab);
        }
      }
    }
  }
  if (npair) atomicAdd(&tab[bd_pairs(n)], npair);
  __syncthreads();
  rs_hist_flush(tab, table + (int64_t)b * bd_stride(n), bd_stride(n));
}

// One thread per image.  Levels to counts in place: count[i] = sum of the levels m > i (a pair of
// level m passes thresholds 0..m-1) plus the threshold-by-threshold count; afterwards slot
// bd_lev(j, k, i + 1) holds count[i][k][j].  Then, per threshold, in this order:
//   P = (sum over k = 0..3 of tp / max(pr, 1)) / 4, R the same over gt, F = 2 P R / (P + R) or 0
// and the three scores are the sums over i of w_i F_i, w_i P_i, w_i R_i, w_i = tau_i / sum tau.
__global__ void boundary_final(uint32_t* __restrict__ table, int64_t* __restrict__ counts, double* __restrict__ out,
                               int B, mdemi_boundary_thresholds thr) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int n = thr.n;
  uint32_t* tb = table + (int64_t)b * bd_stride(n);
  for (int j = 0; j < 3; ++j)
    for (int k = 0; k < 4; ++k) {
      uint32_t run = 0;
      for (int m = n; m >= 1; --m) {
        run += tb[bd_lev(n, j, k, m)];
        tb[bd_lev(n, j, k, m)] = run + tb[bd_dir(n, j, k, m - 1)];
      }
    }
  if (counts)
    for (int i = 0; i < n; ++i)
      for (int k = 0; k < 4; ++k)
        for (int j = 0; j < 3; ++j) counts[(((int64_t)b * n + i) * 4 + k) * 3 + j] = tb[bd_lev(n, j, k, i + 1)];
  double tsum = 0.0;
  for (int i = 0; i < n; ++i) tsum += (double)thr.t[i];
  double f1 = 0.0, prec = 0.0, rec = 0.0;
  uint32_t gt0 = 0;
  for (int k = 0; k < 4; ++k) gt0 += tb[bd_lev(n, 0, k, 1)];
  for (int i = 0; i < n; ++i) {
    double p = 0.0, r = 0.0;
    for (int k = 0; k < 4; ++k) {
      const uint32_t ng = tb[bd_lev(n, 0, k, i + 1)], np = tb[bd_lev(n, 1, k, i + 1)];
      const double tp = (double)tb[bd_lev(n, 2, k, i + 1)];
      p += tp / (double)(np > 1u ? np : 1u);
      r += tp / (double)(ng > 1u ? ng : 1u);
    }
    p *= 0.25;
    r *= 0.25;
    const double f = p + r > 0.0 ? 2.0 * p * r / (p + r) : 0.0;
    const double w = (double)thr.t[i] / tsum;
    f1 += w * f;
    prec += w * p;
    rec += w * r;
  }
  const bool scored = gt0 != 0;  // no ground-truth edge at the lowest threshold: no score
  double* o = out + (int64_t)b * 5;
  o[0] = scored ? f1 : 0.0;
  o[1] = scored ? prec : 0.0;
  o[2] = scored ? rec : 0.0;
  o[3] = (double)tb[bd_pairs(n)];
  o[4] = scored ? 0.0 : 1.0;
}

static bool bd_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace mdemi

using namespace mdemi;

extern "C" size_t mdemi_depth_boundary_workspace_size(int32_t B, int32_t n) {
  if (B <= 0 || n < 1 || n > BD_MAXT) return 0;
  return align_up((size_t)B * bd_stride(n) * sizeof(uint32_t), 256);
}

extern "C" int mdemi_depth_boundary_row_chunks(int32_t H, int32_t W) {
  if (H <= 0 || W <= 0) return 0;
  return (int)cdiv(H, bd_rows(W));
}

extern "C" int mdemi_depth_boundary(const float* pred, const float* gt, int32_t B, int32_t H, int32_t W, int32_t y0,
                                    int32_t y1, int32_t x0, int32_t x1, float min_depth, float max_depth,
                                    int32_t clamp_pred, int32_t mode, const double* coef,
                                    const mdemi_boundary_thresholds* thr, int64_t* counts, double* out,
                                    void* workspace, void* stream) {
  MDEMI_REQUIRE(pred && gt && thr && out && H > 0 && W > 0, "depth_boundary: bad args");
  MDEMI_REQUIRE(B > 0 && B <= 65535, "depth_boundary: B must be 1..65535, got %d", B);
  MDEMI_REQUIRE((int64_t)H * W < (1ll << 30), "depth_boundary: H * W = %lld must be below 2^30 (uint32 counters)",
                (long long)H * W);
  MDEMI_REQUIRE(mode >= 0 && mode <= MDEMI_ALIGN_LSTSQ_DISP,
                "depth_boundary: mode must be 0 (none), 1 (median), 2 (lstsq) or 3 (lstsq_disp), got %d", mode);
  MDEMI_REQUIRE((mode != 0) == (coef != nullptr), "depth_boundary: coef must be NULL exactly when mode is 0 (mode %d)",
                mode);
  MDEMI_REQUIRE(thr->n >= 1 && thr->n <= BD_MAXT, "depth_boundary: n thresholds must be 1..%d, got %d", BD_MAXT,
                thr->n);
  for (int i = 0; i < thr->n; ++i)
    MDEMI_REQUIRE(thr->t[i] > 1.f && thr->t[i] < 3.0e38f && (i == 0 || thr->t[i] >= thr->t[i - 1]),
                  "depth_boundary: thresholds must be finite, above 1 and non-decreasing (t[%d] = %g)", i,
                  (double)thr->t[i]);
  if (!workspace) { set_error("depth_boundary: workspace required"); return MDEMI_EWORKSPACE; }
  MDEMI_REQUIRE(((uintptr_t)workspace & 3) == 0, "depth_boundary: workspace must be 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  uint32_t* table = (uint32_t*)workspace;
  if (hipMemsetAsync(workspace, 0, mdemi_depth_boundary_workspace_size(B, thr->n), st) != hipSuccess)
    return check_launch("depth_boundary (clear)");
  const int rows = bd_rows(W);
  const dim3 grid((unsigned)cdiv(H, rows), (unsigned)B);
  if (W % 4 == 0 && bd_aligned16(pred) && bd_aligned16(gt))
    hipLaunchKernelGGL(boundary_sweep<true>, grid, dim3(256), 0, st, pred, gt, coef, table, H, W, y0, y1, x0, x1,
                       min_depth, max_depth, clamp_pred, mode, rows, *thr);
  else
    hipLaunchKernelGGL(boundary_sweep<false>, grid, dim3(256), 0, st, pred, gt, coef, table, H, W, y0, y1, x0, x1,
                       min_depth, max_depth, clamp_pred, mode, rows, *thr);
  hipLaunchKernelGGL(boundary_final, dim3((unsigned)cdiv(B, 64)), dim3(64), 0, st, table, counts, out, B, *thr);
  return check_launch("depth_boundary");
}
