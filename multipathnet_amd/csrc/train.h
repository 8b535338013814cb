// train.h — internal interface of the head-training kernels (train.hip): the Fast R-CNN loss, the backward pass of the three
// Linear layers behind the ROI pooling and the SGD step, all on the layouts of dense.h (C8 matrices, packed linear weights).
// Used by the mpn_frcnn_train_* entry points (pipeline.hip).  DESIGN.md section 13.
#pragma once
#include "mpn_internal.h"

namespace mpn {

// train.lua:154-158 + BBoxRegressionCriterion.lua on B rows, ONE launch:
//   d_head [B, 5C] row-major = [cls logits z | raw box outputs t^] (what linear_c8 writes as y_rm for the fused head);
//   d_rois, d_gt [B,4] boxes of the original image, d_labels [B] (0 = background; values outside [0, C) are clamped into it);
//   targets t = (convertTo(roi, gt) - mean) / std for labels > 0 (utils.lua:171-184; norm == 0: no normalisation);
//   d_loss[0] = (1/B) sum_i (logsumexp(z_i) - z_i[y_i]),  d_loss[1] = (bbox_weight/B) sum_{i: y_i > 0} sum_j smoothL1(t^_{i,4y_i+j} - t_{i,j});
//   d_g_c8 [ceil(5C/8)][Mp][8] = the gradient w.r.t. d_head as a C8 matrix, rows < B (pad lanes 5C.. of the last chunk +0):
//     (softmax - onehot)/B on the class columns, (bbox_weight/B) clamp(d, -1, 1) on the four target columns, 0 elsewhere.
// The two sums are reduced in a fixed order (one block: per-thread row-ascending partial sums, then a fixed LDS tree): deterministic.
struct LossCfg { float mean[4], std[4]; int norm; float bbox_weight; };
int train_loss(const float *d_head, int B, int C, const float *d_rois, const float *d_gt, const int *d_labels, const LossCfg &cfg,
               float *d_g_c8, int Mp, float *d_loss, hipStream_t s);

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
// Input gradient through y = relu(x W^T + b): dx[m,k] = (sum_{n < N} g[m,n] W[n,k]) * [act[m,k] > 0], reading the packed W with the roles
// of its two dimensions swapped (the contraction runs over NP, n ascending in pairs).  d_act_c8 = the forward activation x (post-ReLU)
// and d_dx_c8, both [>= ceil(K/8)][x_Mp][8]; rows < B are written.
int linear_dgrad_c8(const float *d_g_c8, int g_Mp, int B, int N, const float *d_wpk, int K, const float *d_act_c8, float *d_dx_c8, int x_Mp,
                    hipStream_t s);
// The inverse of pack_linear_weights for output rows [n0, n1): d_w [n1 - n0, K] Torch layout, d_b [n1 - n0]; either may be null.
int unpack_linear_weights(const float *d_wpk, const float *d_bpk, int K, int N, int inner, int n0, int n1, float *d_w, float *d_b, hipStream_t s);

}  // namespace mpn
