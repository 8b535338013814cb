// train.h — internal interface of the head-training kernels (train.hip): the Fast R-CNN loss, the backward pass of the three
// Linear layers behind the ROI pooling and the SGD step, all on the layouts of dense.h (C8 matrices, packed linear weights).
// Used by the mpn_frcnn_train_* entry points (train_driver.hip).  DESIGN.md section 13.
#pragma once
#include "mpn_internal.h"

namespace mpn {

// train.lua:154-158 + BBoxRegressionCriterion.lua on B rows, ONE launch:
//   d_head [B, (K+4)C] row-major = [cls_0 | .. | cls_{K-1} | raw box outputs t^] (what linear_c8 writes as y_rm for the fused head);
//   z = the logits of classifier k, columns [kC, (k+1)C) — the integral loss trains one of its K classifiers per minibatch
//   (model_utils.lua:275-317, train.lua:288-294); K = 1, k = 0: the plain head [z | t^];
//   d_rois, d_gt [B,4] boxes of the original image, d_labels [B] (0 = background; values outside [0, C) are clamped into it);
//   targets t = (convertTo(roi, gt) - mean) / std for labels > 0 (utils.lua:171-184; norm == 0: no normalisation);
//   d_loss[0] = (1/B) sum_i (logsumexp(z_i) - z_i[y_i]),  d_loss[1] = (bbox_weight/B) sum_{i: y_i > 0} sum_j smoothL1(t^_{i,4y_i+j} - t_{i,j});
//   d_g_c8 [ceil((K+4)C/8)][Mp][8] = the gradient w.r.t. d_head as a C8 matrix, rows < B (pad lanes (K+4)C.. of the last chunk +0):
//     (softmax - onehot)/B on classifier k's columns, (bbox_weight/B) clamp(d, -1, 1) on the four target columns KC + 4y + j,
//     exactly +0.0 elsewhere — the K - 1 other classifiers' columns included.
// The two sums are reduced in a fixed order (one block: per-thread row-ascending partial sums, then a fixed LDS tree): deterministic.
struct LossCfg { float mean[4], std[4]; int norm; float bbox_weight; };
int train_loss(const float *d_head, int B, int C, int K, int k, const float *d_rois, const float *d_gt, const int *d_labels, const LossCfg &cfg,
               float *d_g_c8, int Mp, float *d_loss, hipStream_t s);

// The same loss for a head of TWO GEMMs (the tower models: K classifiers on the Foveal towers' concat, the box regressor on the het
// tower): d_cls [B, K*C] and d_bbox [B, 4C] row-major, the gradient in two C8 matrices d_g_cls_c8 [ceil(KC/8)][Mp][8] and d_g_bbox_c8
// [ceil(4C/8)][Mp][8] (pad lanes +0.0) — K*C is in general no multiple of 8, so the fused matrix cannot be cut by a pointer offset.
// The same kernel (one template): every value and both sums are train_loss's.
int train_loss_split(const float *d_cls, const float *d_bbox, int B, int C, int K, int k, const float *d_rois, const float *d_gt, const int *d_labels,
                     const LossCfg &cfg, float *d_g_cls_c8, float *d_g_bbox_c8, int Mp, float *d_loss, hipStream_t s);

// Weight gradient fused with optim.sgd (engines/Optim.lua: dampening 0, no Nesterov) on a packed linear weight [K64/8][NP][8]:
//   dW[n,k] = sum_{m < B} g[m,n] x[m,k]   (v_mfma_f32_32x32x2_f32, rows ascending in pairs: one fixed order, no split, no atomics)
//   g' = dW + wd * w;  v = momentum * v + g';  w = w - lr * v        (each operation rounded on its own)
// applied in registers to the tile the block owns; dW never reaches memory.  d_g_c8 [>= ceil(N/8)][g_Mp][8], d_x_c8 [K64/8][x_Mp][8].
// Rows >= B of both operands are never read.  Lanes n >= N and k outside the layer (inner: pack_linear_weights' K permutation) are
// not touched: the packing's +0.0 stays.  d_vpk: the momentum buffer, same layout as d_wpk.
int sgd_wgrad_c8(const float *d_g_c8, int g_Mp, const float *d_x_c8, int x_Mp, int B, int N, int K, int inner, float *d_wpk, float *d_vpk,
                 float lr, float momentum, float wd, hipStream_t s);
// Bias: db[n] = sum_{m < B} g[m,n] (a fixed pairwise-style order), v = momentum * v + db, b = b - lr * v (biases never decay, Optim.lua:66-68)
int sgd_bias_c8(const float *d_g_c8, int g_Mp, int B, int N, float *d_bpk, float *d_vb, float lr, float momentum, hipStream_t s);
// The two gradients of a layer whose valid rows are SEGMENTS (MultiPathNet's 1x1 mix: rows = (bin, roi) pairs): both operands are C8
// matrices at row pitch nseg * Mp, the valid rows are seg * Mp + m, m < B, seg < nseg; every other row is stale, may be NaN and is never read.
//   dW[n,k] = sum_seg sum_{m < B} g[seg * Mp + m, n] x[seg * Mp + m, k]
// One block per (32 k-chunks x 32 n tile, segment) — sgd_wgrad_c8's record mapping; the block's four waves take a quarter of the B rows each
// (round_up(ceil(B / 4), 2) rows, ascending in pairs from zero) and add their sums pairwise, (q0 + q1) + (q2 + q3) — writes its tile to slab
// seg of d_part (seg_wgrad_part_elems floats); a second launch adds the slabs in ascending order in groups of kWgradSegGroup, the group
// sums in ascending order, and takes the optim.sgd step on the packed weight [K64/8][NP][8] (inner = 1) in registers.  No atomics: the
// order depends on (nseg, B) alone.  d_x_c8 [K64/8][nseg * Mp][8], d_g_c8 [>= ceil(N/8)][nseg * Mp][8].  Pad lanes of the packing stay +0.0.
size_t seg_wgrad_part_elems(int K, int N, int nseg);
int sgd_wgrad_seg_c8(const float *d_g_c8, const float *d_x_c8, int Mp, int nseg, int B, int N, int K, float *d_part, float *d_wpk, float *d_vpk,
                     float lr, float momentum, float wd, hipStream_t s);
// db[n] = the column sums over the same rows: per segment sgd_bias_c8's order, the segment sums through a fixed tree of 64 leaves (more
// segments: the trees' roots in ascending order); fused with the bias step
int sgd_bias_seg_c8(const float *d_g_c8, int Mp, int nseg, int B, int N, float *d_bpk, float *d_vb, float lr, float momentum, hipStream_t s);
// Input gradient through y = relu(x W^T + b): dx[m,k] = (sum_{n < N} g[m,n] W[n,k]) * [act[m,k] > 0] * scale, reading the packed W with the
// roles of its two dimensions swapped (the contraction runs over NP, n ascending in pairs).  d_act_c8 = the forward activation x (post-ReLU)
// and d_dx_c8, both [>= ceil(K/8)][x_Mp][8]; rows < B are written.  scale: 1 / (1 - rate) where act is what dropout_c8 left (a dropped
// element is +0.0, so [act > 0] already is keep mask x ReLU mask); with 1.0f the product is exact: the bits of the unscaled gradient.
// d_act_c8 == nullptr: no activation behind the layer, every element passes (dx = scale * g W).
int linear_dgrad_c8(const float *d_g_c8, int g_Mp, int B, int N, const float *d_wpk, int K, const float *d_act_c8, float *d_dx_c8, int x_Mp,
                    hipStream_t s, float scale = 1.0f);
// nn.Dropout (v2) in place on the C8 matrix [>= ceil(N/8)][Mp][8] linear_c8 has just written, rows < B only (rows >= B are neither read nor
// written).  The mask is stored nowhere: element (row, col) is KEPT iff word col & 3 of Philox4x32-10(counter = (row, col >> 2, layer,
// step), key = (seed_lo, seed_hi)) is >= threshold = floor(rate * 2^32); kept: fl(x * scale), scale = 1.0f / (1.0f - rate); dropped: +0.0f.
// Lanes col >= N of the last record are written +0.0.  One thread per 32-byte record.  DESIGN.md section 13.6.
struct DropoutCfg { uint32_t threshold, seed_lo, seed_hi, layer, step; float scale; };
int dropout_c8(float *d_y_c8, int Mp, int B, int N, const DropoutCfg &cfg, hipStream_t s);
// dfdx:mul(factor) on one momentum buffer (train.lua:321-335, the learning-rate drop): v[i] = fl(v[i] * factor) for i < n, in place, one
// rounding per element, pad lanes of a packed buffer included (factor finite and >= 0 keeps their +0.0).  One grid-stride launch: float4
// records over the first n & ~3 elements, a scalar tail for the rest; d_v is 16-byte aligned (every allocation is).  Each byte is read
// and written once: the kernel is bound by HBM.  DESIGN.md section 13.13.
int scale_momentum(float *d_v, size_t n, float factor, hipStream_t s);
// rows < M of a C8 matrix at row pitch Mp -> row-major [M, N] (c8_to_rowmajor with the pitch given)
int c8_rows_to_rowmajor(const float *d_c8, int Mp, int M, int N, float *d_y, hipStream_t s);
// The inverse of pack_linear_weights for output rows [n0, n1): d_w [n1 - n0, K] Torch layout, d_b [n1 - n0]; either may be null.
int unpack_linear_weights(const float *d_wpk, const float *d_bpk, int K, int N, int inner, int n0, int n1, float *d_w, float *d_b, hipStream_t s);

// ---------------------------------------------------------------------------------------------------------------------------------
// The conv block above the last pooling layer (MPN_TRAIN_CONV(k)): ROI-pooling backward, the 3x3 convolution's
// weight / bias / input gradients and optim.sgd on a packed conv weight.  Maps are C8P activations (dense.h), weights `wpk` packs.
// ---------------------------------------------------------------------------------------------------------------------------------
// inn.ROIPooling:updateGradInput as a per-cell GATHER: out[b][c][y][x] = sum of g[n][c][bin] over the rows n of map b ascending and,
// inside a row, the bins ascending (ph * PW + pw), wherever argmax[n][c][bin] == y * W + x — fp32 adds from +0.0, no atomics, so the
// order is the same in every run.  Every cell of every map is written (cells nothing pooled from get +0.0); a C8P destination's halo
// and pad lanes are the caller's.  The two operand layouts are given by strides:
//   g[n * g_n + (c / 8) * g_cb + (c % 8) * g_c + bin * g_bin],  out[b * o_b + (c / 8) * o_cb + (c % 8) * o_c + y * o_y + x * o_x].
// Rows: by_batch != 0 — all N rows, a row belongs to map clamp((int)rois[n][0] - 1, 0, B - 1) (the forward's rule); otherwise the rows
// [n0, n1) all belong to the ONE map (B == 1).  d_rois is [N,5] (the projected ROIs); with windows != 0 only the bins whose window
// (roi_bin_bounds with `scale`, `rr`: the forward's) holds the cell are visited — the same sum, fewer argmax reads (PH, PW <= 32).
struct RoiBwd {
  const float *g; const int32_t *argmax; const float *rois;
  int by_batch, n0, n1, B, C, H, W, PH, PW, windows;
  long g_n, g_cb, g_c, g_bin, o_b, o_cb, o_c, o_y, o_x;
  float scale; RoiRule rr;
  float *out;
};
int roi_pool_backward(const RoiBwd &a, hipStream_t s);

struct Act;
constexpr int kWgradSegPx = 512;  // pixels per partial sum of the weight gradient
constexpr int kWgradSegGroup = 8; // segments per group of the segment sum (a 150 x 250 map has 74 segments: chains of 8 and 10, not 74)
// floats of the partial-sum buffer conv3x3_wgrad needs for an H x W map
size_t conv_wgrad_part_elems(int Cin, int Cout, int H, int W);
// dW[co][ci][ky][kx] (+)= sum_{y,x} G[co][y][x] * X[ci][y + ky - 1][x + kx - 1] in the `wpk` layout [Cin8/8][9][CoutP][8], pad lanes +0.0.
// v_mfma_f32_32x32x2_f32 over the pixels in row-major pairs, cut into segments of kWgradSegPx pixels, each accumulated from zero by its
// own block into d_part; conv_wgrad_reduce_kernel then adds the segments in ascending order in groups of kWgradSegGroup, adds the group
// sums in ascending order (up to kWgradSegGroup segments: one group, the plain ascending sum) and (accumulate) adds that sum to d_dw:
// the order depends on (Cin, Cout, H, W) alone.  X's halo must be zero (it is the padding); G's halo and the pad channels of its last
// block are never read.  d_part: slab s = segment s in the `wpk` layout, whole 32-byte records of the couts < Cout only — a pad cout's
// records are not written, the pad-cin lanes of a written record hold the sums over X's pad channels (+0.0 for a real map); the
// segment sum reads neither.
int conv3x3_wgrad(const Act &x, const Act &g, float *d_part, float *d_dw, int accumulate, hipStream_t s);
// db[co] (+)= sum_{y,x} G[co][y][x]: 32 interleaved pixel-ascending partial sums, then a fixed tree (as sgd_bias_kernel)
int conv_bias_grad(const Act &g, float *d_db, int accumulate, hipStream_t s);
// g .*= [x > 0] on the interior of the planes (x: the post-ReLU output of the layer the gradient flows into)
int relu_mask_c8p(const Act &g, const Act &x, hipStream_t s);
// nn.SpatialMaxPooling(2,2,2,2):ceil():updateGradInput fused (relu_mask != 0) with the ReLU mask of the layer the gradient flows into
// (include/mpn.h mpn_maxpool2x2_ceil_backward states the contract): per window the maximum is recomputed from X with the forward's
// scan (from -inf, v > m, row-major, cells outside the map skipped) and dY's value goes to the cell the scan ends on — with relu_mask
// only where that cell is > 0 —, every other cell of the window gets +0.0.  Pure routing: every interior cell of dX is written exactly
// once, nothing is added.  The three operands are given by strides, in floats, over (channel block, row, column):
//   X[cb * x_cb + y * x_y + x * x_x + e],  dY[cb * g_cb + Y * g_y + X * g_x + e],  dX[cb * d_cb + y * d_y + x * d_x + e],  e < vec
// with vec = 8 for C8P maps (a channel block is a plane, a cell a 32-byte record read and written as two float4; the pointers are those
// of the interior's first record) and vec = 1 for NCHW (a channel block is one channel).  One thread per (channel block, window),
// windows along x fastest.  Only the H x W interior is stored: halo and pitch padding stay the caller's zeros; the pad lanes
// (channels >= C) of a C8P map's last block are written +0.0, as conv3x3_c8p does.  No LDS.
struct PoolBwd {
  const float *x, *dy;
  float *dx;
  int vec, CB, C, H, W, relu_mask;   // CB channel blocks of `vec` channels, C channels in all
  long x_cb, x_y, x_x, g_cb, g_y, g_x, d_cb, d_y, d_x;
};
int maxpool2x2_backward(const PoolBwd &a, hipStream_t s);
// the C8P form: x, dx [C, H, W], dy [C, ceil(H/2), ceil(W/2)]
int maxpool2x2_backward_c8p(const Act &x, const Act &dy, const Act &dx, int relu_mask, hipStream_t s);
// optim.sgd on a packed conv weight: g' = dW + wd * w, v = momentum * v + g', w = w - lr * v (each rounded on its own), pad lanes untouched
int conv_sgd(float *d_wpk, float *d_vpk, const float *d_dw, int Cin, int Cout, float lr, float momentum, float wd, hipStream_t s);
int vec_sgd(float *d_b, float *d_vb, const float *d_db, int n, float lr, float momentum, hipStream_t s);
// the exact inverse of pack_conv_weights: d_w [Cout,Cin,3,3], d_b [Cout]; either may be null
int unpack_conv_weights(const float *d_wpk, const float *d_bpk, int Cin, int Cout, float *d_w, float *d_b, hipStream_t s);
// the input gradient's weights W'[ci][co][2 - ky][2 - kx] = W[co][ci][ky][kx] in the `wpk` layout of a Cout -> Cin convolution (pack_conv_w_dgrad_kernel),
// its zero bias [conv_coutp(Cin)] and — d_wino_t non-null — the Winograd form of W' (d_tmp: Cout * Cin * 9 floats, W' in Torch layout).
// dX = conv3x3_c8p(G, d_wpk_t, d_zero_b, Cin, relu 0, ..., d_wino_t): the forward's kernels.
int pack_conv_weights_dgrad(const float *d_w, int Cin, int Cout, float *d_tmp, float *d_wpk_t, float *d_zero_b, float *d_wino_t, hipStream_t s);

// ---------------------------------------------------------------------------------------------------------------------------------
// MultiPathNet's conv5 block through the skip pooling (mpn_mpnet_train_begin_conv): the backward of
// nn.Normalize(2) x mul on one tower's conv5 slab and the Foveal ROI poolings' backward summed over the towers.
// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int kNormBwdThreads = 256;
// Per row n < B of ONE tower's conv5 slab — C channels x PP bins as C8 records [ceil(C/8)][PP][Mp][8], record r = cb * PP + bin at
// (r * Mp + n) * 8 (Mp here is the operand's row pitch between two bins) — with x the raw pooled values, y = s x the stored operand,
// s = mul / sqrt(sum x^2 + 1e-10) and g the gradient at y:
//   dx = s * (g - y * (sum_e y_e g_e) / mul^2)       (d_dx_c8: g's layout, a buffer of its own).
// Both sums run over the entries e = r * 8 + lane, e < ceil(C/8) * PP * 8, lanes of channels >= C skipped, in ONE order that depends on
// (C, PP) alone: thread t of kNormBwdThreads adds its entries e = t, t + 256, t + 512, ... ascending from +0.0 with one fused
// multiply-add per entry (fma(x, x, acc); fma(y, g, acc)), then the 256 partial sums go through the tree
//   for (h = 128; h >= 1; h /= 2) part[t] += part[t + h]   (t < h).
// One block per row: one reduction pass and one elementwise pass over the row's slab.  Rows >= B are neither read nor written.
int normalize_backward_c8(const float *d_x_c8, const float *d_y_c8, const float *d_g_c8, float *d_dx_c8, int Mp, int B, int C, int PP, float mul, hipStream_t s);

// inn.ROIPooling:updateGradInput of ONE tower's Foveal region as roi_pool_backward's per-cell gather, ADDED to what the map holds:
//   out[c][y][x] = out[c][y][x] + sum over the rows n in [n0, n1) ascending and, inside a row, the bins ascending of g[n][c][bin] wherever
//   argmax[n][c][bin] == y * W + x — one fp32 chain per cell that starts at the cell's current value.  Called tower after tower on a
// zeroed map it IS the chain "towers ascending, rows ascending, bins ascending from +0.0" of the step's contract; no atomics.
// The operands are roi_pool_backward's (by_batch = 0, B = 1: every field of `a` means what it means there), but row n's window is
// a.rois + n * roi_stride (a Foveal table row holds four regions of 5 floats: roi_stride = 20, a.rois shifted to the region).
int roi_pool_backward_add(const RoiBwd &a, int roi_stride, hipStream_t s);

// out[i] = (float)in[i] (an argmax tensor as a debug tensor: exact below 2^24)
int int_to_float(const int32_t *d_in, size_t n, float *d_out, hipStream_t s);

}  // namespace mpn
