/*
 * mdemi_ext.h — second part of the libmdemi.so C ABI: the ops of the AdaBins
 * and Depthformer-v8 rows of the hot path and the
 * evaluation metrics (A19).  Same conventions as mdemi.h: fp32 device
 * pointers owned by the caller, channels-last activations, `stream` is a
 * hipStream_t passed as void*, 0 / negative MDEMI_E* return, scratch through
 * *_workspace_size() queries, no allocation, no synchronisation.
 *
 * Reference call sites are cited per entry point (paths relative to the
 * reference root).  EfficientNet-B5 itself is third-party
 * (rwightman/gen-efficientnet-pytorch `tf_efficientnet_b5_ap`, fetched by
 * torch.hub at unet_adaptive_bins.py:129 / depthformer_v8.py:89); its ops are
 * restated from that published architecture.
 */
#ifndef MDEMI_EXT_H
#define MDEMI_EXT_H

#include "mdemi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------ */
/* Depthwise KxK convolution over NHWC (groups == C, no bias): the MBConv /  */
/* DepthwiseSeparable conv_dw of EfficientNet-B5 (encoder walked at          */
/* unet_adaptive_bins.py:65-73, depthformer_v8.py:15-24).  w is the          */
/* reference layout [C][1][K][K].  pad_t / pad_l are the top / left padding; */
/* the bottom / right padding follows from OH / OW, which is how TF 'same'   */
/* padding (asymmetric for stride 2) is expressed.                           */
/* ------------------------------------------------------------------------ */
int mdemi_dwconv_fwd(const float* x, const float* w, float* y, int32_t N, int32_t H, int32_t W, int32_t C,
                     int32_t K, int32_t stride, int32_t pad_t, int32_t pad_l, int32_t OH, int32_t OW,
                     void* stream);
size_t mdemi_dwconv_bwd_workspace_size(int32_t N, int32_t C, int32_t K, int32_t OH, int32_t OW);
/* dx and/or dw may be NULL to skip that gradient; dw is overwritten. */
int mdemi_dwconv_bwd(const float* dy, const float* x, const float* w, float* dx, float* dw, int32_t N,
                     int32_t H, int32_t W, int32_t C, int32_t K, int32_t stride, int32_t pad_t, int32_t pad_l,
                     int32_t OH, int32_t OW, void* workspace, void* stream);

/* ------------------------------------------------------------------------ */
/* Per-(image, channel) spatial reductions and channel scaling over NHWC:    */
/* global average pooling and the gate of EfficientNet's SqueezeExcite,      */
/* torch.mean(aux, dim=1) (decoder_v8.py:161).                               */
/*   out[n][c] = scale * sum_p a[n][p][c] * (b ? b[n][p][c] : 1)             */
/*   y[n][p][c] = x[n][p][c] * g[n][c] + (add ? add[n][c] : 0)               */
/* ------------------------------------------------------------------------ */
size_t mdemi_spatial_reduce_workspace_size(int32_t N, int64_t HW, int32_t C);
int mdemi_spatial_reduce(const float* a, const float* b, float* out, int32_t N, int64_t HW, int32_t C,
                         float scale, void* workspace, void* stream);
int mdemi_chan_scale(const float* x, const float* g, const float* add, float* y, int32_t N, int64_t HW,
                     int32_t C, void* stream);
/* the same with y16 (may be NULL): the RNE bf16 copy of y (SqueezeExcite's output, read by
 * the MBConv projection conv as a bf16 GEMM operand under precision "bf16") */
int mdemi_chan_scale16(const float* x, const float* g, const float* add, float* y, void* y16, int32_t N,
                       int64_t HW, int32_t C, void* stream);

/* SqueezeExcite gate MLP (conv_reduce 1x1 + bias, swish, conv_expand 1x1 +  */
/* bias, sigmoid) on pooled [N][C]; wr [R][C], we [C][R].  hid receives the  */
/* pre-activation of conv_reduce [N][R] (saved for the backward).            */
int mdemi_se_gate_fwd(const float* pooled, const float* wr, const float* br, const float* we, const float* be,
                      float* hid, float* gate, int32_t N, int32_t C, int32_t R, void* stream);
/* dgate [N][C] -> dpooled_scale x dpooled [N][C] (1/HW: the gradient each position of the  */
/* mean receives) and the four parameter gradients (overwritten).                           */
size_t mdemi_se_gate_bwd_workspace_size(int32_t N, int32_t C, int32_t R);
int mdemi_se_gate_bwd(const float* pooled, const float* wr, const float* we, const float* hid,
                      const float* gate, const float* dgate, float* dpooled, float* dwr, float* dbr, float* dwe,
                      float* dbe, int32_t N, int32_t C, int32_t R, float dpooled_scale, void* workspace,
                      void* stream);

/* ------------------------------------------------------------------------ */
/* Row softmax with a pre-scale, y = softmax(scale * x) along the last dim:  */
/* attention probabilities of nn.TransformerEncoderLayer (layers.py:8-9),    */
/* PreNormLunaBlock (luna_layer.py:213-215, 244-246), SelfAttentionBlock     */
/* (self_attention.py:72-74).  Backward: dx = scale * y * (dy - <dy, y>).    */
/* ------------------------------------------------------------------------ */
int mdemi_softmax_fwd(const float* x, float* y, int64_t rows, int32_t cols, float scale, void* stream);
int mdemi_softmax_bwd(const float* y, const float* dy, float* dx, int64_t rows, int32_t cols, float scale,
                      int32_t accumulate, void* stream);
/* The same two, also writing the RNE bf16 copy of the result (y16 / dx16, optional): the
 * attention probabilities feed P.V and the score gradient feeds dQ / dK as bf16 GEMM operands
 * (luna_layer.py:202-250 and self_attention.py:61-80 under torch.autocast, configs[4]). */
int mdemi_softmax_fwd16(const float* x, float* y, void* y16, int64_t rows, int32_t cols, float scale, void* stream);
int mdemi_softmax_bwd16(const float* y, const float* dy, float* dx, void* dx16, int64_t rows, int32_t cols,
                        float scale, int32_t accumulate, void* stream);
/* Softmax whose bf16 copy y16 (required) is the DROPPED-OUT probabilities: y16 = RNE bf16 of
 * mdemi_dropout_dev(y, p, seed_dev, seed_add, offset) element for element (the mask index is
 * the element's flat position in y), while y keeps the softmax itself for the backward.  The
 * attention dropout of luna_layer.py:213-215,244-246 / self_attention.py:72-74 fused into the
 * probabilities sweep: P.V reads y16, with no dropout launch and no fp32 copy of dropout(P). */
int mdemi_softmax_fwd_drop16(const float* x, float* y, void* y16, int64_t rows, int32_t cols, float scale, float p,
                             const uint64_t* seed_dev, uint64_t seed_add, uint64_t offset, void* stream);

/* y = act(x) elementwise (MDEMI_ACT_* code): the standalone activations of
 * UpscaleConcatAct (layer_utils.py:121) and the bin regressor
 * (decoder_v8.py:82-90).  The backward is mdemi_elementwise(MDEMI_EW_ACT_BWD). */
int mdemi_act_fwd(const float* x, float* y, int64_t n, int32_t act, void* stream);

/* Inverted dropout with a counter-based mask: y = x * keep(seed, offset+i) / (1-p).
 * The mask is a pure function of (seed, offset, i), so the backward is the
 * same call on dy (nn.Dropout in layers.py:8, luna_layer.py:172-173,
 * feed_forward.py:26, decoder_v8.py:84,87).  p == 0 is a copy. */
int mdemi_dropout(const float* x, float* y, int64_t n, float p, uint64_t seed, uint64_t offset, void* stream);
/* mdemi_dropout with the seed read from device memory (seed_dev[0] + seed_add):
 * the caller draws seed_dev on the GPU (torch's graph-safe Philox), so a
 * hipGraph-captured train step gets a fresh mask on every replay. */
int mdemi_dropout_dev(const float* x, float* y, int64_t n, float p, const uint64_t* seed_dev, uint64_t seed_add,
                      uint64_t offset, void* stream);
/* The same mask, also writing y16 (optional; n % 4 == 0, 16-B aligned x / y, 8-B aligned
 * y16): the RNE bf16 copy of y for a bf16 GEMM that reads it -- the dropout backward's
 * gradient feeding the linear before it (luna_layer.py:172-173 under torch.autocast). */
int mdemi_dropout_dev16(const float* x, float* y, void* y16, int64_t n, float p, const uint64_t* seed_dev,
                        uint64_t seed_add, uint64_t offset, void* stream);

/* ------------------------------------------------------------------------ */
/* Channels-last adaptive-bin head: logits [B][HW][K] (the 1x1 conv_out /    */
/* bin_predictor output, unet_adaptive_bins.py:88-91,97, decoder_v8.py:      */
/* 158-159), pred[b][p] = sum_k softmax(logits)[k] * centers[b][k]            */
/* (unet_adaptive_bins.py:107, depthformer_v8.py:73).  stats [B][HW][2] =    */
/* (max, 1/sum) for the backward.                                            */
/* ------------------------------------------------------------------------ */
int mdemi_binhead_nhwc_fwd(const float* logits, const float* centers, float* pred, float* stats, int32_t B,
                           int64_t HW, int32_t K, void* stream);
size_t mdemi_binhead_nhwc_bwd_workspace_size(int32_t B, int64_t HW, int32_t K);
int mdemi_binhead_nhwc_bwd(const float* logits, const float* centers, const float* pred, const float* stats,
                           const float* dpred, float* dlogits, float* dcenters, int32_t B, int64_t HW, int32_t K,
                           void* workspace, void* stream);

/* Bin widths -> edges -> centres (unet_adaptive_bins.py:99-105 with         */
/* miniViT.py:38-46; depthformer_v8.py:62-66 with decoder_v8.py:163-166):     */
/*   w = act(raw) (mode 0: relu(x)+0.1, 1: elu(x, 0.1)+0.1), wn = w / sum w,  */
/*   edges = cumsum(pad((max-min)*wn, (1,0), min)), centres = mid-points.    */
/* widths_n [B][K] (normalised widths, AdaBins' bin_widths_normed) and        */
/* edges [B][K+1] may be NULL.  Backward: dcenters (+ dedges, dwidths_n,    */
/* each may be NULL) -> draw.                                                */
#define MDEMI_BINS_RELU 0
#define MDEMI_BINS_ELU 1
int mdemi_bins_fwd(const float* raw, float* widths_n, float* edges, float* centers, int32_t B, int32_t K,
                   int32_t mode, float min_val, float max_val, void* stream);
int mdemi_bins_bwd(const float* raw, const float* dcenters, const float* dedges, const float* dwidths_n,
                   float* draw, int32_t B, int32_t K, int32_t mode, float min_val, float max_val, void* stream);

/* ------------------------------------------------------------------------ */
/* Layout helpers                                                            */
/* ------------------------------------------------------------------------ */
/* NCHW -> NHWC with the channel dim zero-padded to Cp >= C (the 3-channel    */
/* image feeding EfficientNet's conv_stem through the implicit-GEMM conv).   */
int mdemi_nchw_to_nhwc_pad(const float* x, float* y, int32_t N, int32_t C, int64_t HW, int32_t Cp, void* stream);
/* Input gradient of a stride == kernel conv (no padding) over NHWC, the
 * scatter of its im2col columns (mViT's 16x16/16 embedding_encoder,
 * layers.py:13-18): x[n][y][x][c] = cols[(n*OH + y/p)*OW + x/p][((y%p)*p + x%p)*C + c]
 * for y < OH*p, x < OW*p; other pixels (dropped by the floor) get 0. */
int mdemi_unpatchify_nhwc(const float* cols, float* x, int32_t N, int32_t H, int32_t W, int32_t C, int32_t p,
                          int32_t OH, int32_t OW, void* stream);
/* Adjoint of replicate padding by p (padding_mode="replicate",              */
/* layer_utils.py:18-22): dx[n][y][x] = sum of dxp over the padded positions */
/* that clamp to (y, x).  dxp is [N][H+2p][W+2p][C].                          */
int mdemi_pad_fold_replicate(const float* dxp, float* dx, int32_t N, int32_t H, int32_t W, int32_t C, int32_t p,
                             void* stream);

/* ------------------------------------------------------------------------ */
/* Evaluation metrics on the GPU (utils/depth_utils.py:4-54): per image,     */
/* over valid = crop rectangle [y0,y1) x [x0,x1) & gt > min_depth &          */
/* gt < max_depth, the 9 metrics of tcompute_errors in this order:           */
/*   a1, a2, a3, abs_rel, sq_rel, rmse, rmse_log, silog, log_10              */
/* plus the valid-pixel count: out [B][10] (fp64).  clamp_pred != 0 clamps   */
/* pred into [min_depth, max_depth] first.                                   */
/* ------------------------------------------------------------------------ */
size_t mdemi_depth_metrics_workspace_size(int32_t B, int32_t H, int32_t W);
int mdemi_depth_metrics(const float* pred, const float* gt, int32_t B, int32_t H, int32_t W, int32_t y0,
                        int32_t y1, int32_t x0, int32_t x1, float min_depth, float max_depth, int32_t clamp_pred,
                        double* out, void* workspace, void* stream);

/* ------------------------------------------------------------------------ */
/* Scale- and shift-aligned metrics (cfg eval.align; this framework's own    */
/* definition).  Per image, over the same valid set V (n       */
/* pixels, p the unclamped prediction, g the ground truth):                  */
/*   MEDIAN      s = median(g) / median(p), t = 0; numpy's median (even n:   */
/*               the mean of the two middle order statistics), the order     */
/*               statistics exact on the fp32 values, mean and quotient fp64 */
/*   LSTSQ       (s, t) minimise sum (s p + t - g)^2, every sum in fp64:     */
/*               det = n Spp - Sp^2, s = (n Spg - Sp Sg) / det,              */
/*               t = (Spp Sg - Sp Spg) / det                                 */
/*   LSTSQ_DISP  the same solve on x = 1/p, y = 1/g (fp64 reciprocals)       */
/* An image fails (status 1, s = 1, t = 0, evaluated unaligned) when n == 0, */
/* median(p) is not > 0 or det is not finite and > 0.                        */
/* mdemi_depth_align writes coef [B][4] = s, t, n, status (fp64).  It does   */
/* not synchronise or allocate; the workspace is cleared on the stream.      */
/* mdemi_depth_metrics_aligned reads coef on the device, forms               */
/*   q = (float)(s p + t)            (MEDIAN, LSTSQ)                         */
/*   q = (float)(1 / max(s / p + t, 1 / max_depth))   (LSTSQ_DISP)           */
/* in fp64 rounded once (q = p on a failed image), writes it to aligned      */
/* [B][H][W] on every pixel when that is not NULL, and reduces the metrics   */
/* of q exactly as mdemi_depth_metrics would (same bits): out [B][12] = its  */
/* ten columns, then s and t.  workspace: mdemi_depth_metrics_workspace_size.*/
/* ------------------------------------------------------------------------ */
#define MDEMI_ALIGN_MEDIAN 1
#define MDEMI_ALIGN_LSTSQ 2
#define MDEMI_ALIGN_LSTSQ_DISP 3
size_t mdemi_depth_align_workspace_size(int32_t B, int32_t H, int32_t W, int32_t mode);
int mdemi_depth_align(const float* pred, const float* gt, int32_t B, int32_t H, int32_t W, int32_t y0, int32_t y1,
                      int32_t x0, int32_t x1, float min_depth, float max_depth, int32_t mode, double* coef,
                      void* workspace, void* stream);
int mdemi_depth_metrics_aligned(const float* pred, const float* gt, int32_t B, int32_t H, int32_t W, int32_t y0,
                                int32_t y1, int32_t x0, int32_t x1, float min_depth, float max_depth,
                                int32_t clamp_pred, int32_t mode, const double* coef, float* aligned, double* out,
                                void* workspace, void* stream);

/* ------------------------------------------------------------------------ */
/* Scale-invariant boundary F1 (cfg eval.boundary; this framework's own      */
/* definition, DESIGN.md 1c, after Depth Pro).  Per image, g the ground      */
/* truth and q the fp32 value the metrics evaluate: pred, or with mode != 0  */
/* the aligned value mdemi_depth_metrics_aligned forms from coef (read on    */
/* the device), clamped into [min_depth, max_depth] when clamp_pred != 0.    */
/* A pair is two horizontally or vertically adjacent pixels both in the      */
/* valid set V above.  For thresholds t[0] <= ... <= t[n-1], all > 1, a      */
/* pair is an edge of a map d at t[i] of kind                                */
/*   0  right is farther   d[y][x+1] > fl32(t[i] d[y][x])                    */
/*   1  left is farther    d[y][x]   > fl32(t[i] d[y][x+1])                  */
/*   2  lower is farther   d[y+1][x] > fl32(t[i] d[y][x])                    */
/*   3  upper is farther   d[y][x]   > fl32(t[i] d[y+1][x])                  */
/* (one rounded fp32 multiply, a strict compare).  counts [B][n][4][3]       */
/* (int64, may be NULL) = the pairs that are such an edge in g, in q, in     */
/* both.  In fp64, in this order:                                            */
/*   P_i = (sum_k tp / max(pred, 1)) / 4, R_i = (sum_k tp / max(gt, 1)) / 4, */
/*   F_i = 2 P_i R_i / (P_i + R_i) (0 when P_i + R_i = 0),                   */
/*   w_i = t[i] / sum t;  f1 = sum w_i F_i, likewise precision and recall.   */
/* out [B][5] = f1, precision, recall, the number of pairs, status.  An      */
/* image whose ground truth has no edge at t[0] has no score: status 1,      */
/* the three scores 0.  Non-finite predictions are outside the contract.     */
/* thr is read on the host during the call.  The call does not synchronise   */
/* or allocate; the workspace (mdemi_depth_boundary_workspace_size bytes,    */
/* 4-byte aligned) is cleared on the stream; integer counters, so two runs   */
/* give the same bits.  H * W < 2^30, B is 1..65535.  Rows that are 16-byte  */
/* aligned (W % 4 == 0 and aligned bases) take the 4-pixel vector path.      */
/* mdemi_depth_boundary_row_chunks: the sweep's grid along the rows.         */
/* ------------------------------------------------------------------------ */
#define MDEMI_BOUNDARY_MAX_T 16
typedef struct mdemi_boundary_thresholds {
  int32_t n;
  float t[MDEMI_BOUNDARY_MAX_T];
} mdemi_boundary_thresholds;
size_t mdemi_depth_boundary_workspace_size(int32_t B, int32_t n);
int mdemi_depth_boundary_row_chunks(int32_t H, int32_t W);
int mdemi_depth_boundary(const float* pred, const float* gt, int32_t B, int32_t H, int32_t W, int32_t y0,
                         int32_t y1, int32_t x0, int32_t x1, float min_depth, float max_depth, int32_t clamp_pred,
                         int32_t mode, const double* coef, const mdemi_boundary_thresholds* thr, int64_t* counts,
                         double* out, void* workspace, void* stream);

/* ------------------------------------------------------------------------ */
/* Flip-eval (config eval.flip_eval): rows of W floats (an NCHW batch is     */
/* B*C*H rows).  flip_w: y[r][w] = x[r][W-1-w] (out of place).              */
/* flip_avg_w: y[r][w] = (a[r][w] + b[r][W-1-w]) / 2; y may alias a.        */
/* ------------------------------------------------------------------------ */
int mdemi_flip_w(const float* x, float* y, int64_t rows, int32_t W, void* stream);
int mdemi_flip_avg_w(const float* a, const float* b, float* y, int64_t rows, int32_t W, void* stream);

/* ------------------------------------------------------------------------ */
/* Prediction export (utils/visualize_utils.py:10-29 colorize, :32-51        */
/* visualization): one launch reads pred [B][h][w] once and writes every     */
/* non-NULL output once, each [B][H][W] (rgba: x4 bytes).  (h, w) != (H, W)  */
/* resamples with the align_corners=True taps of mdemi_bilinear_fwd.         */
/*   depth_out: the (resampled) fp32 depth d                                 */
/*   rgba: colorize(d, vmin, vmax) through lut (256 x RGBA8, device): all    */
/*     in fp32, x = (d - vmin) / (vmax - vmin) (the range formed in double   */
/*     from the two floats, rounded once; x = d * 0 when vmin == vmax),      */
/*     index = trunc(x * 256) with 256 -> 255; NaN -> (0,0,0,0); d > vmax or */
/*     d < vmin (+-inf included) -> (255,255,255,255)                        */
/*   raw16: min(65535, rint(d * png_scale)) (round half even), 0 for NaN and */
/*     d <= 0: the 16-bit depth PNG payload, png_scale 256 (KITTI) / 1000    */
/*     (NYU), so that png / png_scale reads back within 0.5 / png_scale      */
/* rgba and lut 4-byte aligned; 16-byte aligned pred / depth_out / rgba and  */
/* 8-byte aligned raw16 take the 4-pixel vector path.                        */
/* ------------------------------------------------------------------------ */
int mdemi_depth_export(const float* pred, int32_t B, int32_t h, int32_t w, int32_t H, int32_t W, float vmin,
                       float vmax, const uint8_t* lut, float png_scale, float* depth_out, uint8_t* rgba,
                       uint16_t* raw16, void* stream);

/* ------------------------------------------------------------------------ */
/* AdaBins bin-centre chamfer loss (cfg loss.chamfer_weight; upstream        */
/* BinsChamferLoss over pytorch3d chamfer_distance -- the reference's loss  */
/* module is absent, parity unpinned).  from_edges: edges [B][P+1] (AdaBins) */
/* else centres [B][P] (Depthformer v8); gt [B][HW]; targets              */
/* are gt >= thresh.  fwd writes the batch-mean loss (loss[0]) and          */
/* dloss/dcentres [B][P] (gcent); bwd: dedges = dloss[0] (device scalar) *   */
/* the centre gradients pushed onto both edges of each bin.                 */
/* ------------------------------------------------------------------------ */
size_t mdemi_bins_chamfer_workspace_size(int32_t B, int32_t P, int64_t HW);
int mdemi_bins_chamfer_fwd(const float* edges, const float* gt, int32_t B, int32_t P, int32_t from_edges, int64_t HW,
                           float thresh, float* loss, float* gcent, void* workspace, void* stream);
int mdemi_bins_chamfer_bwd(const float* gcent, const float* dloss, float* dedges, int32_t B, int32_t P,
                           int32_t from_edges, void* stream);

/* ------------------------------------------------------------------------ */
/* Conv weight re-layouts (reference [Cout][Cin][KH][KW] <-> GEMM operands): */
/* OHWI: out[co][ky][kx][c] = w[co][c][ky][kx]  (fwd, patch-conv dgrad)     */
/* OIHW: out[co][c][ky][kx] = w[co][ky][kx][c]  (wgrad -> parameter layout) */
/* DGRAD: out[ky][kx][co][c] = w[co][c][KH-1-ky][KW-1-kx] (input gradient)   */
/* Out of place; cout/cin/kh/kw always describe the conv.                   */
/* ------------------------------------------------------------------------ */
#define MDEMI_WL_OHWI 0
#define MDEMI_WL_OIHW 1
#define MDEMI_WL_DGRAD 2
int mdemi_conv_weight_layout(const float* w, float* out, int32_t cout, int32_t cin, int32_t kh, int32_t kw,
                             int32_t mode, void* stream);
/* The same re-layout also writing out16 (optional): the RNE bf16 copy of `out`, the operand a bf16
 * conv GEMM reads (bf16 storage, configs[4]) -- one sweep instead of the re-layout plus a cast of
 * the fresh re-laid-out weight every step (layer_utils.py:20-24 ConvBN under torch.autocast). */
int mdemi_conv_weight_layout16(const float* w, float* out, void* out16, int32_t cout, int32_t cin, int32_t kh,
                               int32_t kw, int32_t mode, void* stream);

/* ------------------------------------------------------------------------ */
/* Sample transform of dataset/depth_dataset.py (replaces DepthDataset.      */
/* __getitem__ :197-236 after file decoding, with random_crop :238-248,      */
/* train_preprocess/augment_image/hide_depth :250-284, ImageDepth2Tensor     */
/* :287-311 and RandomMasking :314-386) for a batch of decoded samples:      */
/* rgb [B][H0][W0][3] uint8, depth [B][H0][W0] uint16 -> image [B][3][h][w]  */
/* ImageNet-normalised fp32, depth [B][1][h][w] = raw / saving_factor.       */
/* The frame (top, left, Hs, Ws) is the KITTI KB crop or the whole image;   */
/* the rotation (Pillow's Image.rotate about the frame centre) and the crop */
/* act inside it.  params: B device entries drawn by the host in the        */
/* reference's order (mdemi/data.py).  nyu_mask applies depth_mask           */
/* [45:472, 43:608] before the rotation; nearest_generic selects Pillow's    */
/* I;16 nearest path (else the 16.16 fixed-point path of modes F and I).     */
/* train = 0 is the test transform (no clip, hide_depth or masking).         */
/* ------------------------------------------------------------------------ */
#define MDEMI_AUG_MAX_SPANS 8
typedef struct {
  double affine[6];  /* Image.rotate's inverse map (x, y) -> source, in double     */
  int32_t fixed[6];  /* the same map in Pillow's 16.16 fixed point (affine_fixed)  */
  int32_t rotate;    /* 0: angle % 360 == 0 (Pillow returns a copy)                */
  int32_t crop_x, crop_y, flip;
  float gamma, brightness, color[3];
  int32_t n_rows, n_cols, mask_keep; /* RandomMasking spans; mask_keep: drop_edge */
  int32_t rows[MDEMI_AUG_MAX_SPANS][2];
  int32_t cols[MDEMI_AUG_MAX_SPANS][2];
} mdemi_aug_sample;
int mdemi_augment(const uint8_t* rgb, const uint16_t* depth, int32_t B, int32_t H0, int32_t W0, int32_t top,
                  int32_t left, int32_t Hs, int32_t Ws, int32_t h, int32_t w, const mdemi_aug_sample* params,
                  int32_t nyu_mask, int32_t nearest_generic, int32_t train, float saving_factor, float clip_depth,
                  float* image, float* depth_out, void* stream);

/* ------------------------------------------------------------------------ */
/* ODA2 ordered-swin2 (model/ODA2)                          */
/* ------------------------------------------------------------------------ */
/* Window shuffle of PreNormOrderedSwinSA (oda2_red_order_swin2_decoder.py:  */
/* 83-85,103,126-131): roll by -shift + window_partition as one gather       */
/* (inverse = 0): dst row r = ((n*nWh + wy)*nWw + wx)*ws^2 + ty*ws + tx       */
/* takes src[n][(wy*ws+ty+shift) % H][(wx*ws+tx+shift) % W]; inverse = 1 is  */
/* the scatter back (window_reverse + roll by +shift), optionally + add (the */
/* residual `out + identity`, natural layout).  H, W multiples of ws.         */
int mdemi_window_shuffle(const float* src, float* dst, const float* add, int32_t N, int32_t H, int32_t W,
                         int32_t C, int32_t ws, int32_t shift, int32_t inverse, void* stream);
/* the same gather for the int32 depth-index map [N][H][W] (:85,88) */
int mdemi_window_shuffle_i32(const int32_t* src, int32_t* dst, int32_t N, int32_t H, int32_t W, int32_t ws,
                             int32_t shift, void* stream);
/* Ordered window softmax (:87-92,116-119): S, P are [nwin][heads][T][T]     */
/* (T = ws^2 = 64 or 256), idx the window-major depth indices [nwin][T],     */
/* table the depth_embedding [2*num_emb-1][heads] (NULL: bias_type "none").  */
/*   P[w][h][i][j] = softmax_j(scale*S + table[idx_i - idx_j + num_emb-1][h]) */
/* S == P is allowed.  Backward: dS = scale * P o (dP - rowsum(P o dP)) and, */
/* when d_table != NULL, d_table[k][h] = sum of P o (dP - ...) over the     */
/* entries whose relative index is k (overwritten).                          */
int mdemi_ordered_softmax_fwd(const float* S, float* P, const int32_t* idx, const float* table, int32_t nwin,
                              int32_t heads, int32_t T, int32_t num_emb, float scale, void* stream);
size_t mdemi_ordered_softmax_bwd_workspace_size(int32_t nwin, int32_t heads, int32_t num_emb);
int mdemi_ordered_softmax_bwd(const float* P, const float* dP, float* dS, const int32_t* idx, float* d_table,
                              int32_t nwin, int32_t heads, int32_t T, int32_t num_emb, float scale, void* workspace,
                              void* stream);
/* nn.GLU(dim=-1) (oda2_red_order_reg_decoder.py:61,78): x [M][2F] ->        */
/* y [M][F] = x[:, :F] * sigmoid(x[:, F:]); bwd writes dx [M][2F].  F % 4 == 0 */
int mdemi_glu_fwd(const float* x, float* y, int64_t M, int32_t F, void* stream);
int mdemi_glu_bwd(const float* x, const float* dy, float* dx, int64_t M, int32_t F, void* stream);
/* Replicate padding / cropping as one clamp-gather over NHWC (the reference */
/* pads with F.pad(mode="replicate"): oda2_swin_transformer.py:258,327,491,  */
/* and the depthwise conv's padding_mode, oda2_red_order_reg_decoder.py:65): */
/*   y[n][oy][ox] = x[n][clamp(oy-pt, 0, H-1)][clamp(ox-pl, 0, W-1)], y is   */
/* [N][OH][OW][C].  inverse = 1 is the adjoint: x is the [N][OH][OW][C]       */
/* gradient, y the [N][H][W][C] sum over the positions that clamp to each   */
/* pixel.  An NCHW image is the NHWC map [N*C][H][W][1].                      */
int mdemi_pad_replicate(const float* x, float* y, int32_t N, int32_t H, int32_t W, int32_t C, int32_t OH,
                        int32_t OW, int32_t pt, int32_t pl, int32_t inverse, void* stream);

/* ------------------------------------------------------------------------ */
/* Step telemetry for the training driver (mdemi.run / mdemi.train.loop)     */
/* ------------------------------------------------------------------------ */
/* sumsq[0] = sum_t ||param_t||^2 over a tensor table (the norm the reference */
/* logged: utils/common_utils.py:65-75 compute_param_norm).  Same (tensor,   */
/* chunk) item maps and workspace as mdemi_grad_sumsq                        */
/* (mdemi_grad_norm_workspace_size): fp32 partial per item, fp64 final sum   */
/* in a fixed order -- deterministic.  Only `param` and `numel` of each      */
/* entry are read.                                                           */
int mdemi_param_sumsq(const mdemi_tensor_ref* tensors_dev, int32_t ntensors, int64_t nitems, float* sumsq,
                      void* workspace, void* stream);

/* One record per optimizer step, appended on the device.                    */
#define MDEMI_STEP_LOSS_NONFINITE 1u
#define MDEMI_STEP_GRAD_NONFINITE 2u
typedef struct mdemi_step_record {
  float loss;
  float grad_sumsq; /* ||grad_scale * grad||^2 before the clip; -1 when not given */
  int32_t index;    /* 0-based push count */
  uint32_t flags;   /* MDEMI_STEP_* */
} mdemi_step_record;
typedef struct mdemi_telemetry_state {
  int32_t pushed;          /* records appended so far */
  int32_t nonfinite_steps; /* records with a flag set */
  int32_t first_nonfinite; /* index of the first of them; the host initialises -1 */
  int32_t _pad;
} mdemi_telemetry_state;
/* A one-thread kernel: ring[state->pushed % capacity] = {loss[0], grad_sumsq */
/* ? grad_sumsq[0] : -1, pushed, flags}, then the counters advance.  ring,   */
/* state, loss and grad_sumsq (may be NULL) are device pointers; the counter */
/* lives on the device, so a captured hipGraph advances it on every replay.  */
int mdemi_telemetry_push(mdemi_step_record* ring, int32_t capacity, mdemi_telemetry_state* state,
                         const float* loss, const float* grad_sumsq, void* stream);

/* ------------------------------------------------------------------------ */
/* Guarded AdamW steps (train.nonfinite: "skip"): mdemi_adamw_step16 /       */
/* mdemi_adamw_step_dev16 (mdemi.h) that drop a step with non-finite         */
/* gradients on the device, with no host in the loop.                        */
/*   ok = isfinite(sumsq[0])                                                 */
/* sumsq is the scalar mdemi_grad_sumsq left over the SAME table and         */
/* grad_scale; it is required here, also when max_norm == 0 (NULL gives      */
/* MDEMI_EINVAL and nothing is launched).  Squares are non-negative and the  */
/* final sum is fp64, so a NaN or inf in any gradient element reaches it and */
/* nothing cancels it.  A finite gradient whose fp32 sum of squares          */
/* overflows (an element beyond ~1.8e19, or a work item whose squares add up */
/* to more than FLT_MAX) is skipped as well.  The loss is not part of the    */
/* predicate: under data parallelism it is rank-local, while sumsq is taken  */
/* after the all-reduce and is the same on every rank.                       */
/* ok:      every byte written -- param, exp_avg, exp_avg_sq, the bf16 copy, */
/*          tensor_steps, *step_dev -- is what the unguarded call writes.    */
/* not ok:  every block of the update returns after reading the scalar; no   */
/*          byte of param, exp_avg, exp_avg_sq, the bf16 copies or           */
/*          tensor_steps is written.  *step_dev, the schedule position,      */
/*          still advances by one.                                           */
/* tensor_steps (the per-parameter bias-correction counts) and guard_dev are */
/* required.  guard_dev points at one mdemi_guard_state in device memory     */
/* that the trailing tick kernel updates; the host zero-initialises it with  */
/* last_skipped = -1.  It lives at a fixed address, so a captured hipGraph   */
/* advances it on every replay.                                              */
/* ------------------------------------------------------------------------ */
typedef struct mdemi_guard_state {
  int32_t skipped;      /* steps dropped so far */
  int32_t consecutive;  /* length of the current streak of dropped steps; 0 after an applied step */
  int32_t last_skipped; /* 0-based index of the last dropped step: *step_dev before the call */
                        /* (capturable form) or `calls` before the call (host form) */
  int32_t calls;        /* guarded calls so far */
} mdemi_guard_state;
int mdemi_adamw_step_guarded16(const mdemi_tensor_ref* tensors_dev, int32_t ntensors,
                               const mdemi_adamw_group* groups_host, int32_t ngroups, const float* sumsq,
                               float max_norm, float grad_scale, int32_t* tensor_steps, int64_t nitems,
                               void* const* param16_dev, mdemi_guard_state* guard_dev, void* workspace,
                               void* stream);
int mdemi_adamw_step_dev_guarded16(const mdemi_tensor_ref* tensors_dev, int32_t ntensors,
                                   const mdemi_adamw_group* sched_dev, int32_t nsteps, int32_t ngroups,
                                   int32_t* step_dev, int32_t* tensor_steps, const float* sumsq, float max_norm,
                                   float grad_scale, int64_t nitems, void* const* param16_dev,
                                   mdemi_guard_state* guard_dev, void* workspace, void* stream);

/* ------------------------------------------------------------------------ */
/* AdamW steps that also keep an exponential moving average of the weights   */
/* (train.ema_decay): mdemi_adamw_step16 / mdemi_adamw_step_dev16 with the   */
/* average updated in the same sweep, on the value just written to param:    */
/*   n = ema_state_dev->updates            (read before the tick)            */
/*   d = ema_warmup ? min(ema_decay, (1 + n) / (10 + n)) : ema_decay  (fp32) */
/*   e = fmaf(1 - d, p_new - e, e)                                           */
/* ema_dev: ntensors device pointers in device memory, one per table entry;  */
/* a NULL entry means that tensor keeps no average.  An average that is not  */
/* 16-byte aligned is read and written one float at a time; it does not      */
/* change which path param, exp_avg and exp_avg_sq take, so those stay bit   */
/* for bit what the step without an average writes.                          */
/* ema_state_dev points at one mdemi_ema_state in device memory              */
/* (the host zero-initialises it); the trailing tick kernel adds one to      */
/* `updates` per applied call.                                               */
/* guard_dev NULL: p, m, v, the bf16 copies, tensor_steps and *step_dev are  */
/* written exactly as by mdemi_adamw_step16 / mdemi_adamw_step_dev16.        */
/* guard_dev non-NULL: exactly as by the guarded entry points above, with    */
/* their requirements (sumsq, tensor_steps); `step` is not read.  A skipped  */
/* call writes no byte of any average and leaves `updates` alone.            */
/* ema_dev or ema_state_dev NULL, or ema_decay outside [0, 1), gives         */
/* MDEMI_EINVAL and nothing is launched.                                     */
/* ------------------------------------------------------------------------ */
typedef struct mdemi_ema_state {
  int32_t updates; /* applied calls so far */
} mdemi_ema_state;
int mdemi_adamw_step_ema16(const mdemi_tensor_ref* tensors_dev, int32_t ntensors,
                           const mdemi_adamw_group* groups_host, int32_t ngroups, const float* sumsq, float max_norm,
                           float grad_scale, int32_t step, int32_t* tensor_steps, int64_t nitems,
                           void* const* param16_dev, float* const* ema_dev, float ema_decay, int32_t ema_warmup,
                           mdemi_ema_state* ema_state_dev, mdemi_guard_state* guard_dev, void* workspace,
                           void* stream);
int mdemi_adamw_step_dev_ema16(const mdemi_tensor_ref* tensors_dev, int32_t ntensors,
                               const mdemi_adamw_group* sched_dev, int32_t nsteps, int32_t ngroups,
                               int32_t* step_dev, int32_t* tensor_steps, const float* sumsq, float max_norm,
                               float grad_scale, int64_t nitems, void* const* param16_dev, float* const* ema_dev,
                               float ema_decay, int32_t ema_warmup, mdemi_ema_state* ema_state_dev,
                               mdemi_guard_state* guard_dev, void* workspace, void* stream);

/* ------------------------------------------------------------------------ */
/* Multi-scale gradient-matching loss (cfg loss.grad_weight / grad_scales;   */
/* this framework's own definition, DESIGN.md 1c -- no reference parity).    */
/* pred, gt [B][H][W]; R = log(pred) - log(gt) where gt > min_depth.  Scale  */
/* k < scales (1..4) works on R[::s, ::s], s = 2^k: S_bk sums |R(y,x+s) -     */
/* R(y,x)| and |R(y+s,x) - R(y,x)| over grid pairs valid at both ends, N_bk  */
/* counts the valid grid pixels.  per_image 0: loss = sum_k sum_b S_bk /     */
/* sum_b N_bk; 1: the mean over images with N_b0 > 0 of sum_k S_bk / N_bk;   */
/* an empty scale adds 0, no valid pixel at all gives 0.                     */
/* fwd writes loss[0] and wk [B][4] = dloss/dS_bk (0 for k >= scales); bwd:  */
/* dpred = dloss[0] (device scalar) * sum_k wk[b][k] * c_k / pred with c_k   */
/* the sum over the pixel's scale-k neighbours n of sign(R - R(n)), sign(0)  */
/* = 0; exactly 0 where gt <= min_depth.  A gather without atomics: both     */
/* passes are bit-deterministic.  Any H, W; rows that are 16-byte aligned    */
/* (W % 4 == 0 and aligned bases) take the 4-pixel vector path.              */
/* workspace: mdemi_gradmatch_workspace_size bytes, 16-byte aligned.         */
/* ------------------------------------------------------------------------ */
size_t mdemi_gradmatch_workspace_size(int32_t B, int32_t H, int32_t W);
int mdemi_gradmatch_fwd(const float* pred, const float* gt, float* loss, float* wk, int32_t B, int32_t H, int32_t W,
                        float min_depth, int32_t scales, int32_t per_image, void* workspace, void* stream);
int mdemi_gradmatch_bwd(const float* pred, const float* gt, const float* wk, const float* dloss, float* dpred,
                        int32_t B, int32_t H, int32_t W, float min_depth, int32_t scales, void* stream);

/* ------------------------------------------------------------------------ */
/* Scale- and shift-invariant loss (cfg loss.ssi_weight / ssi_space /        */
/* ssi_trim / ssi_norm; this framework's own definition, DESIGN.md 1c -- no  */
/* reference parity).  pred, gt [B][H][W].  Per image, on V = gt > min_depth */
/* (n pixels): x, y = p, g (DEPTH) or 1/p, 1/g (DISP, fp64 reciprocals);     */
/* Sx, Sy, Sxx, Sxy, Syy in fp64; det = n Sxx - Sx^2, s = (n Sxy - Sx Sy) /  */
/* det, t = (Sxx Sy - Sx Sxy) / det (mdemi_depth_align's LSTSQ solve);       */
/* r = s x + t - y in fp64, rho = |(float) r|.  Trimming, trim in [0, 0.5]:  */
/* u = n - floor((double) trim * n), tau = the u-th smallest rho (exact, on  */
/* the fp32 values), K = {rho <= tau} with every tie kept, U = |K|,          */
/* Q = sum_K r^2, A = sum_K r x, Bt = sum_K r; trim == 0: K = V, U = n and   */
/* A = Bt = 0 by definition.  norm GT_VAR: v = Syy / n - (Sy / n)^2, else    */
/* v = 1.  An image is skipped -- loss 0, gradient exactly 0, out of the     */
/* per-image mean -- when n == 0, det is finite and <= 0, or v is finite and */
/* <= 0; a non-finite det (a NaN / inf prediction, p = 0 under DISP) is not: */
/* the loss is NaN.  per_image 0: loss = sum_b (Q_b / v_b) / (2 sum_b U_b),  */
/* w_b = 1 / (v_b sum U); 1: the mean over the images used of                */
/* Q_b / (2 U_b v_b), w_b = 1 / (U_b v_b images used); none used gives 0.    */
/* fwd writes loss[0] and coef [B][8] (fp64) = s, t, tau, a = w s, e0, e1,   */
/* e2, status (1: skipped); bwd recomputes r and rho with the forward's      */
/* arithmetic, so K is the forward's bit for bit, and writes                 */
/*   dpred = dloss[0] * (k r a + e0 + e1 x + e2 y) * dx/dp,  dx/dp = 1 or    */
/*   -1 / p^2; e0 + e1 x + e2 y = w [(A - Bt Sx / n)(n y - Sy - 2 s (n x -   */
/*   Sx)) / det - Bt s / n], the dependence of (s, t) on pred, exactly 0     */
/*   without trimming; exactly 0 where gt <= min_depth.                      */
/* Neither synchronises or allocates; the select's counters are cleared on   */
/* the stream; fp64 partials combine in a fixed order and only integer       */
/* atomics are used: two runs give the same bits.  Any H, W and base; H * W  */
/* % 4 == 0 with 16-byte aligned bases takes the 4-pixel vector path.        */
/* workspace: mdemi_ssi_workspace_size bytes (trimmed = trim > 0 adds a      */
/* [B][H][W] plane of rho), 16-byte aligned.  B is 1..65535.                 */
/* ------------------------------------------------------------------------ */
#define MDEMI_SSI_DEPTH 0
#define MDEMI_SSI_DISP 1
#define MDEMI_SSI_NORM_NONE 0
#define MDEMI_SSI_NORM_GT_VAR 1
size_t mdemi_ssi_workspace_size(int32_t B, int32_t H, int32_t W, int32_t trimmed);
int mdemi_ssi_fwd(const float* pred, const float* gt, float* loss, double* coef, int32_t B, int32_t H, int32_t W,
                  float min_depth, int32_t space, float trim, int32_t norm, int32_t per_image, void* workspace,
                  void* stream);
int mdemi_ssi_bwd(const float* pred, const float* gt, const double* coef, const float* dloss, float* dpred, int32_t B,
                  int32_t H, int32_t W, float min_depth, int32_t space, void* stream);

/* ------------------------------------------------------------------------ */
/* Tiled inference (cfg eval.tile / tile_overlap / tile_align; this          */
/* framework's own definition, DESIGN.md 1c -- no reference parity).  The    */
/* plan is two ascending host arrays of tile origins, ys [ny] and xs [nx],   */
/* ny, nx in 1..MDEMI_TILE_MAX_AXIS, for tiles of th x tw inside the H x W   */
/* image (H * W < 2^31); they are copied into the kernel arguments, so every */
/* call can be captured.  Tile k = iy * nx + ix, T = ny * nx; image b's tile */
/* k sits at index b * T + k.  oy, ox in [0, th), [0, tw) are the overlaps   */
/* the ramps are built from: wy(u) = min(u + 1, th - u, max(1, oy)) on row u */
/* of a tile, wx the same, w = wy * wx (an exact integer in fp64).           */
/*   mdemi_tile_extract: out [B*T][C][th][tw] = the tiles of img             */
/*     [B][C][H][W], bit for bit, one launch; T * C <= 65535.  16-byte       */
/*     accesses where the pointer, W, tw and the tile's x origin allow.      */
/*   mdemi_tile_blend: out [B][H][W] = (float)(sum_k w_k q_k / sum_k w_k)    */
/*     over the tiles that cover the pixel, in ascending k, every operation  */
/*     in fp64, rounded once; one launch, a gather without atomics.  The     */
/*     tiles must cover the image (first origin 0, last H - th, no gap).     */
/*     tiles [B*T][th][tw] holds the predictions p.  mode MDEMI_TILE_NONE:   */
/*     q = p, coef may be NULL.  MDEMI_ALIGN_LSTSQ: q = s p + t with         */
/*     (s, t) = coef[b][k].  MDEMI_ALIGN_LSTSQ_DISP: q = s / p + t (fp64     */
/*     reciprocal) and out = (float)(1 / max(blend, 1 / max_depth)).  NaN    */
/*     and inf propagate (the max too keeps a NaN).                          */
/*   mdemi_tile_align: coef [B][T][4] = s, t, n, status (fp64).  Tile 0 is   */
/*     the anchor (1, 0, 0, 0).  For k = 1 .. T-1 in order, over the pixels  */
/*     of tile k that some tile j < k covers: x = p_k (LSTSQ) or 1 / p_k     */
/*     (LSTSQ_DISP), y = the fp64 blend (formula above) of the q_j, j < k;   */
/*     pairs with a non-finite x or y, and under LSTSQ_DISP with p_k <= 0,   */
/*     are left out; (s, t) minimise sum (s x + t - y)^2 (the LSTSQ solve of */
/*     mdemi_depth_align).  A tile fails -- status 1, s = 1, t = 0 -- when   */
/*     n < 2, det is not finite and > 0, or s is not > 0.  An axis with      */
/*     several tiles needs an overlap > 0.  1 + 2 (T - 1) launches enqueued  */
/*     by the call: the anchor rows, then per tile one statistics kernel     */
/*     (per-chunk fp64 partials) and one one-wave-per-image solve.           */
/* None synchronises or allocates; every sum is fp64 in a fixed order: two   */
/* runs give the same bits.  workspace: mdemi_tile_align_workspace_size      */
/* bytes, 8-byte aligned.  B is 1..65535.                                    */
/* ------------------------------------------------------------------------ */
#define MDEMI_TILE_MAX_AXIS 32
#define MDEMI_TILE_NONE 0
int mdemi_tile_extract(const float* img, float* out, int32_t B, int32_t C, int32_t H, int32_t W, int32_t th,
                       int32_t tw, const int32_t* ys, int32_t ny, const int32_t* xs, int32_t nx, void* stream);
size_t mdemi_tile_align_workspace_size(int32_t B, int32_t th, int32_t tw);
int mdemi_tile_align(const float* tiles, int32_t B, int32_t H, int32_t W, int32_t th, int32_t tw, int32_t oy,
                     int32_t ox, const int32_t* ys, int32_t ny, const int32_t* xs, int32_t nx, int32_t mode,
                     double* coef, void* workspace, void* stream);
int mdemi_tile_blend(const float* tiles, const double* coef, int32_t B, int32_t H, int32_t W, int32_t th, int32_t tw,
                     int32_t oy, int32_t ox, const int32_t* ys, int32_t ny, const int32_t* xs, int32_t nx,
                     int32_t mode, float max_depth, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MDEMI_EXT_H */
