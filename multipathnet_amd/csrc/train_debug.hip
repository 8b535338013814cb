// train_debug.hip — the state-free mpn_debug_* pass-throughs to the training kernels (debug flavour only).  They
// touch no training state: the hooks that read one (mpn_debug_bench_train_*) stay beside it in train_driver.hip.
#include "dense.h"
#include "train.h"

#ifdef MPN_DEBUG_HOOKS
using namespace mpn;

// tests/test_gpu_train_kernels_numerics.py (debug flavour only): train.h's head-training kernels one launch at a time, on raw device
// pointers in the kernels' own layouts, through the product's host wrappers (their grids, their MPN_CHECK_ARG) on the null stream.  Every
// buffer comes with its element count and a buffer smaller than the footprint of its layout is refused before anything is launched — a
// layout mistake of a test becomes MPN_EINVAL, never an access outside the test's allocation.  Footprints: K64 / 8 * NP * 8 for a packed
// linear weight (K64 = K rounded up to 64), chunks * Mp * 8 for a C8 matrix, conv_wpk_elems for a packed conv weight, the whole
// padded planes for a C8P map.  Dimensions a footprint cannot be computed from (<= 0) go to the wrapper, which refuses them.
static bool dbg_short(const char *fn, const char *name, size_t have, size_t want) {
  if (have >= want) return false;
  set_error("%s: %s holds %zu elements, the launch's footprint is %zu", fn, name, have, want);
  return true;
}
#define DBG_NEED(buf, have, want) do { if (dbg_short(__func__, #buf, (size_t)(have), (size_t)(want))) return MPN_EINVAL; } while (0)
static size_t dbg_c8(int cols, int Mp) { return (size_t)cdiv(cols, 8) * Mp * 8; }
static size_t dbg_lin_pack(int K, int N) { return (size_t)(round_up(K, 64) / 8) * lin_np(N) * 8; }

extern "C" int mpn_debug_train_loss(const float *d_head, size_t n_head, int B, int C, int K, int k, const float *d_rois, size_t n_rois, const float *d_gt,
                                    size_t n_gt, const int *d_labels, size_t n_labels, const float *mean4, const float *std4, int norm,
                                    float bbox_weight, float *d_g_c8, size_t n_g, int Mp, float *d_loss, size_t n_loss) {
  MPN_CHECK_ARG(mean4 && std4);
  if (B > 0 && C > 1 && K >= 1 && Mp >= B) {
    DBG_NEED(d_head, n_head, (size_t)B * (K + 4) * C);
    DBG_NEED(d_rois, n_rois, (size_t)B * 4);
    DBG_NEED(d_gt, n_gt, (size_t)B * 4);
    DBG_NEED(d_labels, n_labels, (size_t)B);
    DBG_NEED(d_g_c8, n_g, dbg_c8((K + 4) * C, Mp));
    DBG_NEED(d_loss, n_loss, 2);
  }
  LossCfg cfg{};
  for (int j = 0; j < 4; ++j) { cfg.mean[j] = mean4[j]; cfg.std[j] = std4[j]; }
  cfg.norm = norm; cfg.bbox_weight = bbox_weight;
  return train_loss(d_head, B, C, K, k, d_rois, d_gt, d_labels, cfg, d_g_c8, Mp, d_loss, nullptr);
}

extern "C" int mpn_debug_sgd_wgrad_c8(const float *d_g_c8, size_t n_g, int g_Mp, const float *d_x_c8, size_t n_x, int x_Mp, int B, int N, int K, int inner,
                                      float *d_wpk, size_t n_w, float *d_vpk, size_t n_v, float lr, float momentum, float wd) {
  if (B > 0 && N > 0 && K > 0 && g_Mp >= B && x_Mp >= B) {
    DBG_NEED(d_g_c8, n_g, dbg_c8(N, g_Mp));
    DBG_NEED(d_x_c8, n_x, dbg_c8(round_up(K, 64), x_Mp));
    DBG_NEED(d_wpk, n_w, dbg_lin_pack(K, N));
    DBG_NEED(d_vpk, n_v, dbg_lin_pack(K, N));
  }
  return sgd_wgrad_c8(d_g_c8, g_Mp, d_x_c8, x_Mp, B, N, K, inner, d_wpk, d_vpk, lr, momentum, wd, nullptr);
}

extern "C" int mpn_debug_sgd_bias_c8(const float *d_g_c8, size_t n_g, int g_Mp, int B, int N, float *d_bpk, size_t n_b, float *d_vb, size_t n_vb, float lr,
                                     float momentum) {
  if (B > 0 && N > 0 && g_Mp >= B) {
    DBG_NEED(d_g_c8, n_g, dbg_c8(N, g_Mp));
    DBG_NEED(d_bpk, n_b, (size_t)N);
    DBG_NEED(d_vb, n_vb, (size_t)N);
  }
  return sgd_bias_c8(d_g_c8, g_Mp, B, N, d_bpk, d_vb, lr, momentum, nullptr);
}

extern "C" int mpn_debug_linear_dgrad_c8(const float *d_g_c8, size_t n_g, int g_Mp, int B, int N, const float *d_wpk, size_t n_w, int K, const float *d_act_c8,
                                         size_t n_act, float *d_dx_c8, size_t n_dx, int x_Mp, float scale) {
  if (B > 0 && N > 0 && K > 0 && g_Mp >= B && x_Mp >= B) {
    DBG_NEED(d_g_c8, n_g, dbg_c8(N, g_Mp));
    DBG_NEED(d_wpk, n_w, dbg_lin_pack(K, N));
    if (d_act_c8) DBG_NEED(d_act_c8, n_act, dbg_c8(K, x_Mp));  // (null: the unmasked form)
    DBG_NEED(d_dx_c8, n_dx, dbg_c8(K, x_Mp));
  }
  return linear_dgrad_c8(d_g_c8, g_Mp, B, N, d_wpk, K, d_act_c8, d_dx_c8, x_Mp, nullptr, scale);
}

// the segmented forms (MultiPathNet's mix layer): operands at row pitch nseg * Mp
extern "C" int mpn_debug_sgd_wgrad_seg_c8(const float *d_g_c8, size_t n_g, const float *d_x_c8, size_t n_x, int Mp, int nseg, int B, int N, int K, float *d_part,
                                          size_t n_part, float *d_wpk, size_t n_w, float *d_vpk, size_t n_v, float lr, float momentum, float wd) {
  if (B > 0 && N > 0 && K > 0 && Mp >= B && nseg > 0 && nseg <= 65535) {
    DBG_NEED(d_g_c8, n_g, dbg_c8(N, nseg * Mp));
    DBG_NEED(d_x_c8, n_x, dbg_c8(round_up(K, 64), nseg * Mp));
    DBG_NEED(d_part, n_part, seg_wgrad_part_elems(K, N, nseg));
    DBG_NEED(d_wpk, n_w, dbg_lin_pack(K, N));
    DBG_NEED(d_vpk, n_v, dbg_lin_pack(K, N));
  }
  return sgd_wgrad_seg_c8(d_g_c8, d_x_c8, Mp, nseg, B, N, K, d_part, d_wpk, d_vpk, lr, momentum, wd, nullptr);
}

extern "C" int mpn_debug_sgd_bias_seg_c8(const float *d_g_c8, size_t n_g, int Mp, int nseg, int B, int N, float *d_bpk, size_t n_b, float *d_vb, size_t n_vb,
                                         float lr, float momentum) {
  if (B > 0 && N > 0 && Mp >= B && nseg > 0) {
    DBG_NEED(d_g_c8, n_g, dbg_c8(N, nseg * Mp));
    DBG_NEED(d_bpk, n_b, (size_t)N);
    DBG_NEED(d_vb, n_vb, (size_t)N);
  }
  return sgd_bias_seg_c8(d_g_c8, Mp, nseg, B, N, d_bpk, d_vb, lr, momentum, nullptr);
}

extern "C" int mpn_debug_dropout_c8(float *d_y_c8, size_t n_y, int Mp, int B, int N, uint32_t threshold, uint32_t seed_lo, uint32_t seed_hi, uint32_t layer,
                                    uint32_t step, float scale) {
  if (B > 0 && N > 0 && Mp >= B) DBG_NEED(d_y_c8, n_y, dbg_c8(N, Mp));
  DropoutCfg cfg{};
  cfg.threshold = threshold; cfg.seed_lo = seed_lo; cfg.seed_hi = seed_hi; cfg.layer = layer; cfg.step = step; cfg.scale = scale;
  return dropout_c8(d_y_c8, Mp, B, N, cfg, nullptr);
}

extern "C" int mpn_debug_c8_rows_to_rowmajor(const float *d_c8, size_t n_c8, int Mp, int M, int N, float *d_y, size_t n_y) {
  if (M > 0 && N > 0 && Mp >= M) {
    DBG_NEED(d_c8, n_c8, dbg_c8(N, Mp));
    DBG_NEED(d_y, n_y, (size_t)M * N);
  }
  return c8_rows_to_rowmajor(d_c8, Mp, M, N, d_y, nullptr);
}

extern "C" int mpn_debug_pack_linear_weights(const float *d_w, size_t n_w, const float *d_b, size_t n_b, int K, int N, int inner, float *d_wpk, size_t n_wpk,
                                             float *d_bpk, size_t n_bpk) {
  if (K > 0 && N > 0) {
    DBG_NEED(d_w, n_w, (size_t)K * N);
    if (d_b) DBG_NEED(d_b, n_b, (size_t)N);
    DBG_NEED(d_wpk, n_wpk, dbg_lin_pack(K, N));
    DBG_NEED(d_bpk, n_bpk, (size_t)lin_np(N));
  }
  return pack_linear_weights(d_w, d_b, K, N, inner, d_wpk, d_bpk, nullptr);
}

extern "C" int mpn_debug_unpack_linear_weights(const float *d_wpk, size_t n_wpk, const float *d_bpk, size_t n_bpk, int K, int N, int inner, int n0, int n1,
                                               float *d_w, size_t n_w, float *d_b, size_t n_b) {
  if (K > 0 && N > 0 && n0 >= 0 && n1 > n0 && n1 <= N) {
    DBG_NEED(d_wpk, n_wpk, dbg_lin_pack(K, N));
    DBG_NEED(d_bpk, n_bpk, (size_t)lin_np(N));
    if (d_w) DBG_NEED(d_w, n_w, (size_t)(n1 - n0) * K);
    if (d_b) DBG_NEED(d_b, n_b, (size_t)(n1 - n0));
  }
  return unpack_linear_weights(d_wpk, d_bpk, K, N, inner, n0, n1, d_w, d_b, nullptr);
}

extern "C" int mpn_debug_conv_sgd(float *d_wpk, size_t n_w, float *d_vpk, size_t n_v, const float *d_dw, size_t n_dw, int Cin, int Cout, float lr,
                                  float momentum, float wd) {
  if (Cin > 0 && Cout > 0) {
    DBG_NEED(d_wpk, n_w, conv_wpk_elems(Cin, Cout));
    DBG_NEED(d_vpk, n_v, conv_wpk_elems(Cin, Cout));
    DBG_NEED(d_dw, n_dw, conv_wpk_elems(Cin, Cout));
  }
  return conv_sgd(d_wpk, d_vpk, d_dw, Cin, Cout, lr, momentum, wd, nullptr);
}

extern "C" int mpn_debug_vec_sgd(float *d_b, size_t n_b, float *d_vb, size_t n_vb, const float *d_db, size_t n_db, int n, float lr, float momentum) {
  if (n > 0) {
    DBG_NEED(d_b, n_b, (size_t)n);
    DBG_NEED(d_vb, n_vb, (size_t)n);
    DBG_NEED(d_db, n_db, (size_t)n);
  }
  return vec_sgd(d_b, d_vb, d_db, n, lr, momentum, nullptr);
}

// the two maps as make_act lays a C x H x W map out (mpn_debug_conv3x3_form's rule)
extern "C" int mpn_debug_relu_mask_c8p(float *d_g, size_t n_g, const float *d_x, size_t n_x, int C, int H, int W) {
  MPN_CHECK_ARG(C > 0 && H > 0 && W > 0);
  DBG_NEED(d_g, n_g, act_bytes(C, H, W) / sizeof(float));
  DBG_NEED(d_x, n_x, act_bytes(C, H, W) / sizeof(float));
  return relu_mask_c8p(make_act(d_g, C, H, W), make_act(const_cast<float *>(d_x), C, H, W), nullptr);
}

extern "C" int mpn_debug_unpack_conv_weights(const float *d_wpk, size_t n_wpk, const float *d_bpk, size_t n_bpk, int Cin, int Cout, float *d_w, size_t n_w,
                                             float *d_b, size_t n_b) {
  if (Cin > 0 && Cout > 0) {
    DBG_NEED(d_wpk, n_wpk, conv_wpk_elems(Cin, Cout));
    if (d_b) { DBG_NEED(d_bpk, n_bpk, (size_t)Cout); DBG_NEED(d_b, n_b, (size_t)Cout); }
    if (d_w) DBG_NEED(d_w, n_w, (size_t)Cout * Cin * 9);
  }
  return unpack_conv_weights(d_wpk, d_bpk, Cin, Cout, d_w, d_b, nullptr);
}
// tests/test_gpu_train_conv_kernels_numerics.py (debug flavour only): the conv-block half of train.h, the split
// loss and scale_momentum under the same rules.
static size_t dbg_act(int C, int H, int W) { return act_bytes(C, H, W) / sizeof(float); }

extern "C" int mpn_debug_train_loss_split(const float *d_cls, size_t n_cls, const float *d_bbox, size_t n_bbox, int B, int C, int K, int k, const float *d_rois,
                                          size_t n_rois, const float *d_gt, size_t n_gt, const int *d_labels, size_t n_labels, const float *mean4,
                                          const float *std4, int norm, float bbox_weight, float *d_g_cls_c8, size_t n_g_cls, float *d_g_bbox_c8,
                                          size_t n_g_bbox, int Mp, float *d_loss, size_t n_loss) {
  MPN_CHECK_ARG(mean4 && std4);
  if (B > 0 && C > 1 && K >= 1 && Mp >= B) {
    DBG_NEED(d_cls, n_cls, (size_t)B * K * C);
    DBG_NEED(d_bbox, n_bbox, (size_t)B * 4 * C);
    DBG_NEED(d_rois, n_rois, (size_t)B * 4);
    DBG_NEED(d_gt, n_gt, (size_t)B * 4);
    DBG_NEED(d_labels, n_labels, (size_t)B);
    DBG_NEED(d_g_cls_c8, n_g_cls, dbg_c8(K * C, Mp));
    DBG_NEED(d_g_bbox_c8, n_g_bbox, dbg_c8(4 * C, Mp));
    DBG_NEED(d_loss, n_loss, 2);
  }
  LossCfg cfg{};
  for (int j = 0; j < 4; ++j) { cfg.mean[j] = mean4[j]; cfg.std[j] = std4[j]; }
  cfg.norm = norm; cfg.bbox_weight = bbox_weight;
  return train_loss_split(d_cls, d_bbox, B, C, K, k, d_rois, d_gt, d_labels, cfg, d_g_cls_c8, d_g_bbox_c8, Mp, d_loss, nullptr);
}

extern "C" int mpn_debug_scale_momentum(float *d_v, size_t n_v, size_t n, float factor) {
  DBG_NEED(d_v, n_v, n);
  return scale_momentum(d_v, n, factor, nullptr);
}

// layout 0: mpn_roi_pool_backward's NCHW strides (g [N, C, PH, PW], out [B, C, H, W]).  layout 1: train_conv_backward's — g the C8 matrix
// whose record (c / 8) * PP + bin holds row n at n * 8 (pitch Mp >= N), out the interior of ONE C8P map (B == 1).  The rows the kernel may
// visit are [n0, n1) in both row modes, so n1 <= N is checked here: the wrapper does not know N.
extern "C" int mpn_debug_roi_pool_backward(const float *d_g, size_t n_g, const int32_t *d_argmax, size_t n_argmax, const float *d_rois, size_t n_rois, int N,
                                           int layout, int Mp, int by_batch, int n0, int n1, int B, int C, int H, int W, int PH, int PW, int windows,
                                           float scale, int bin_rule, float *d_out, size_t n_out) {
  MPN_CHECK_ARG(N > 0 && n0 >= 0 && n1 >= n0 && n1 <= N && (layout == 0 || layout == 1) && (bin_rule == 0 || bin_rule == 1));
  MPN_CHECK_ARG(layout == 0 || (B == 1 && Mp >= N));
  RoiBwd a{};
  if (B > 0 && C > 0 && H > 0 && W > 0 && PH > 0 && PW > 0) {
    const size_t PP = (size_t)PH * PW;
    DBG_NEED(d_rois, n_rois, (size_t)(N - 1) * 5 + 5);
    DBG_NEED(d_argmax, n_argmax, (size_t)N * C * PP);
    if (layout == 0) {
      DBG_NEED(d_g, n_g, (size_t)N * C * PP);
      DBG_NEED(d_out, n_out, (size_t)B * C * H * W);
      a.g_n = (long)(C * PP); a.g_cb = (long)(8 * PP); a.g_c = (long)PP; a.g_bin = 1;
      a.o_b = (long)C * H * W; a.o_cb = 8L * H * W; a.o_c = (long)H * W; a.o_y = W; a.o_x = 1;
      a.out = d_out;
    } else {
      DBG_NEED(d_g, n_g, (size_t)cdiv(C, 8) * PP * Mp * 8);  // whole records: (C / 8 rounded up) * PP of them, not ceil(C * PP / 8)
      DBG_NEED(d_out, n_out, dbg_act(C, H, W));
      const Act G = make_act(d_out, C, H, W);
      a.g_n = 8; a.g_cb = (long)PP * Mp * 8; a.g_c = 1; a.g_bin = (long)Mp * 8;
      a.o_b = 0; a.o_cb = (long)G.plane(); a.o_c = 1; a.o_y = (long)G.Wp * 8; a.o_x = 8;
      a.out = d_out ? G.p + ((size_t)G.Wp + 1) * 8 : nullptr;
    }
  }
  a.g = d_g; a.argmax = d_argmax; a.rois = d_rois; a.by_batch = by_batch; a.n0 = n0; a.n1 = n1; a.B = B; a.C = C; a.H = H; a.W = W; a.PH = PH; a.PW = PW;
  a.windows = windows; a.scale = scale; a.rr = RoiRule{1.0f, 0, bin_rule};
  return roi_pool_backward(a, nullptr);
}

extern "C" int mpn_debug_conv3x3_wgrad(const float *d_x, size_t n_x, const float *d_g, size_t n_g, int Cin, int Cout, int H, int W, float *d_part, size_t n_part,
                                       float *d_dw, size_t n_dw, int accumulate) {
  MPN_CHECK_ARG(Cin > 0 && Cout > 0 && H > 0 && W > 0);
  DBG_NEED(d_x, n_x, dbg_act(Cin, H, W));
  DBG_NEED(d_g, n_g, dbg_act(Cout, H, W));
  DBG_NEED(d_part, n_part, conv_wgrad_part_elems(Cin, Cout, H, W));
  DBG_NEED(d_dw, n_dw, conv_wpk_elems(Cin, Cout));
  return conv3x3_wgrad(make_act(const_cast<float *>(d_x), Cin, H, W), make_act(const_cast<float *>(d_g), Cout, H, W), d_part, d_dw, accumulate, nullptr);
}

extern "C" int mpn_debug_conv_bias_grad(const float *d_g, size_t n_g, int Cout, int H, int W, float *d_db, size_t n_db, int accumulate) {
  MPN_CHECK_ARG(Cout > 0 && H > 0 && W > 0);
  DBG_NEED(d_g, n_g, dbg_act(Cout, H, W));
  DBG_NEED(d_db, n_db, (size_t)Cout);
  return conv_bias_grad(make_act(const_cast<float *>(d_g), Cout, H, W), d_db, accumulate, nullptr);
}

// x, dx [C, H, W] and dy [C, ceil(H/2), ceil(W/2)] as make_act lays them out
extern "C" int mpn_debug_maxpool2x2_backward_c8p(const float *d_x, size_t n_x, const float *d_dy, size_t n_dy, float *d_dx, size_t n_dx, int C, int H, int W,
                                                 int relu_mask) {
  MPN_CHECK_ARG(C > 0 && H > 0 && W > 0);
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  DBG_NEED(d_x, n_x, dbg_act(C, H, W));
  DBG_NEED(d_dy, n_dy, dbg_act(C, Ho, Wo));
  DBG_NEED(d_dx, n_dx, dbg_act(C, H, W));
  return maxpool2x2_backward_c8p(make_act(const_cast<float *>(d_x), C, H, W), make_act(const_cast<float *>(d_dy), C, Ho, Wo), make_act(d_dx, C, H, W),
                                 relu_mask, nullptr);
}

// d_w [Cout, Cin, 3, 3]; the outputs are those of the Cout -> Cin convolution; d_tmp / d_wino_t may both be null
extern "C" int mpn_debug_pack_conv_weights_dgrad(const float *d_w, size_t n_w, int Cin, int Cout, float *d_tmp, size_t n_tmp, float *d_wpk_t, size_t n_wpk_t,
                                                 float *d_zero_b, size_t n_zero_b, float *d_wino_t, size_t n_wino_t) {
  if (Cin > 0 && Cout > 0) {
    DBG_NEED(d_w, n_w, (size_t)Cout * Cin * 9);
    if (d_tmp) DBG_NEED(d_tmp, n_tmp, (size_t)Cout * Cin * 9);
    DBG_NEED(d_wpk_t, n_wpk_t, conv_wpk_elems(Cout, Cin));
    DBG_NEED(d_zero_b, n_zero_b, (size_t)conv_coutp(Cin));
    if (d_wino_t) DBG_NEED(d_wino_t, n_wino_t, conv_wino_elems(Cout, Cin));
  }
  return pack_conv_weights_dgrad(d_w, Cin, Cout, d_tmp, d_wpk_t, d_zero_b, d_wino_t, nullptr);
}

// the forward's Winograd packer on d_w [Cout, Cin, 3, 3]
extern "C" int mpn_debug_pack_conv_weights_wino(const float *d_w, size_t n_w, int Cin, int Cout, float *d_wino, size_t n_wino) {
  if (Cin > 0 && Cout > 0) {
    DBG_NEED(d_w, n_w, (size_t)Cout * Cin * 9);
    DBG_NEED(d_wino, n_wino, conv_wino_elems(Cin, Cout));
  }
  return pack_conv_weights_wino(d_w, Cin, Cout, d_wino, nullptr);
}

// tests/test_gpu_train_phase2_kernels_numerics.py (debug flavour only): the kernels between the mix layers and
// the conv block (mpn_mpnet_train_begin_conv) under the same rules.
// x, y, g, dx: one tower's conv5 slab [ceil(C/8)][PP][Mp][8] each
extern "C" int mpn_debug_normalize_backward_c8(const float *d_x_c8, size_t n_x, const float *d_y_c8, size_t n_y, const float *d_g_c8, size_t n_g, float *d_dx_c8,
                                               size_t n_dx, int Mp, int B, int C, int PP, float mul) {
  if (B > 0 && Mp >= B && C > 0 && PP > 0) {
    const size_t slab = (size_t)cdiv(C, 8) * PP * Mp * 8;
    DBG_NEED(d_x_c8, n_x, slab);
    DBG_NEED(d_y_c8, n_y, slab);
    DBG_NEED(d_g_c8, n_g, slab);
    DBG_NEED(d_dx_c8, n_dx, slab);
  }
  return normalize_backward_c8(d_x_c8, d_y_c8, d_g_c8, d_dx_c8, Mp, B, C, PP, mul, nullptr);
}

// The trainer's layout alone (layout 1 of mpn_debug_roi_pool_backward): g the C8 matrix at pitch Mp >= N, out the interior of ONE C8P map
// as make_act lays it out; row n's window is d_rois + n * roi_stride.  B = 1 and by_batch = 0 are set here and n1 <= N is checked here
// (the wrapper does not know N); a roi_stride below 5 and the window limits are the wrapper's to refuse.
extern "C" int mpn_debug_roi_pool_backward_add(const float *d_g, size_t n_g, const int32_t *d_argmax, size_t n_argmax, const float *d_rois, size_t n_rois, int N,
                                               int roi_stride, int Mp, int n0, int n1, int C, int H, int W, int PH, int PW, int windows, float scale,
                                               int bin_rule, float *d_out, size_t n_out) {
  MPN_CHECK_ARG(N > 0 && n0 >= 0 && n1 >= n0 && n1 <= N && Mp >= N && (bin_rule == 0 || bin_rule == 1));
  RoiBwd a{};
  if (C > 0 && H > 0 && W > 0 && PH > 0 && PW > 0) {
    const size_t PP = (size_t)PH * PW;
    if (roi_stride >= 5) DBG_NEED(d_rois, n_rois, (size_t)(N - 1) * roi_stride + 5);
    DBG_NEED(d_argmax, n_argmax, (size_t)N * C * PP);
    DBG_NEED(d_g, n_g, (size_t)cdiv(C, 8) * PP * Mp * 8);
    DBG_NEED(d_out, n_out, dbg_act(C, H, W));
    const Act G = make_act(d_out, C, H, W);
    a.g_n = 8; a.g_cb = (long)PP * Mp * 8; a.g_c = 1; a.g_bin = (long)Mp * 8;
    a.o_b = 0; a.o_cb = (long)G.plane(); a.o_c = 1; a.o_y = (long)G.Wp * 8; a.o_x = 8;
    a.out = d_out ? G.p + ((size_t)G.Wp + 1) * 8 : nullptr;
  }
  a.g = d_g; a.argmax = d_argmax; a.rois = d_rois; a.by_batch = 0; a.n0 = n0; a.n1 = n1; a.B = 1; a.C = C; a.H = H; a.W = W; a.PH = PH; a.PW = PW;
  a.windows = windows; a.scale = scale; a.rr = RoiRule{1.0f, 0, bin_rule};
  return roi_pool_backward_add(a, roi_stride, nullptr);
}

extern "C" int mpn_debug_int_to_float(const int32_t *d_in, size_t n_in, size_t n, float *d_out, size_t n_out) {
  DBG_NEED(d_in, n_in, n);
  DBG_NEED(d_out, n_out, n);
  return int_to_float(d_in, n, d_out, nullptr);
}
#undef DBG_NEED

#endif
